"""Per-launch tracing for the roofline leg of bench.py: the state (TRACE, TRACE_RANGES, set_trace) and ONE open / close
pair around a launch.  A record is the 8-tuple (tag, kind, flops, bytes, ev0, ev1, shape, owner); tools/bench_extras.py
aligns the records with the profiler's kernel records by position and name.  The state is read and set HERE (a copy
imported into another module would go stale): `TRACE is None` is the product state and all an untraced launch tests.
"""
import torch

from . import lib as L

TRACE = None   # profiling only (set_trace): (tag, kind, flops, bytes, ev0, ev1, shape, module) per launch
TRACE_RANGES = False   # each traced launch also opens a torch.profiler range "evt#<record index>"


def set_trace(rec, ranges=False):
    """profiling aid of bench.py's roofline leg: a list switches per-launch records (and the library's kernel-name tags)
    on, None switches both off (the product state).  ranges=True wraps every traced launch in a torch.profiler
    record_function range, so that a surrounding torch.profiler session attributes the launch's kernels (durations from
    the same tracer rocprofv3 uses) to the record -- HIP-event pairs add a few microseconds to every small launch."""
    global TRACE, TRACE_RANGES
    TRACE = rec
    TRACE_RANGES = bool(ranges) and rec is not None
    L.lib().evt_debug_kernel_tags(1 if rec is not None else 0)


def t0():
    """open a record in front of a launch: None when tracing is off, else what t1 takes"""
    if TRACE is None:
        return None
    rf = None
    if TRACE_RANGES:
        rf = torch.profiler.record_function(f"evt#{len(TRACE)}")
        rf.__enter__()
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e, rf


def t1(e0, tag, kind, flops, nbytes, shape, owner):
    """close the record behind the launch: the closing event, the profiler range, the record.  tag None = the name of the
    kernel the library launched last; `owner` = a module of the model the launch belongs to (bench.py attributes
    HiFi-GAN's element-wise launches to `dec` through it)"""
    e0, rf = e0
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    if rf is not None:
        rf.__exit__(None, None, None)
    if tag is None:
        tag = L.lib().evt_last_kernel_tag().decode()
    TRACE.append((tag, kind, flops, nbytes, e0, e1, shape, owner))


def t1_elt(e0, name, nbytes, owner):
    """an element-wise launch (leaky-relu copy, stage mean, activation derivative): no flops, bytes = operands in + out"""
    t1(e0, name, "elt", 0, nbytes, name, owner)


def t1_conv(e0, kind, m, nseq, lin, extra_elems):
    """one convolution launch (kind: fwd / bwd_data / bwd_weight) of module m on [nseq, lin, cin]"""
    lq = lin if m.transposed else m.lout(lin)
    macs = nseq * lq * m.cin * m.cout * m.k // m.groups
    sz = 2 if L.is_half(m._slot.bank.dtype) else 4
    act = nseq * (lin * m.cin + m.lout(lin) * m.cout) + extra_elems
    wbytes = m.v.numel() * (4 if kind == "bwd_weight" else sz)
    shape = (f"{'T' if m.transposed else ''}{m.cin}>{m.cout} k{m.k} s{m.stride} d{m.dil} g{m.groups} "
             f"n{nseq} L{lin}")
    t1(e0, None, kind, 2 * macs, act * sz + wbytes, shape, m)
