"""Single launches on prepared slots, without autograd: forward / backward-data convolution and the element-wise helpers
beside them; hip/conv.py (ConvFn) and hip/resunit.py (the ResBlock units) are built on these."""
import ctypes as C

import torch

from . import lib as L
from . import trace as T


def _bias(m):
    return m.bias.data if m.bias is not None else None


def _dptr(t):
    return t.data_ptr() if t is not None else None


def _fwd(slot, x, res, in_slope, out_act, out_slope, out=None):
    """`out`: optional preallocated contiguous [nseq, Lout, Cout] destination (e.g. one plane of a q|k|v buffer)"""
    m = slot.module
    if x.dim() != 3 or x.size(2) != m.cin or x.dtype != slot.bank.dtype or not x.is_contiguous():
        raise L.EvtError(f"conv input must be contiguous [nseq, L, {m.cin}] {slot.bank.dtype}, got "
                         f"{tuple(x.shape)} {x.dtype} contiguous={x.is_contiguous()}")
    nseq, lin = x.size(0), x.size(1)
    y = out if out is not None else torch.empty((nseq, m.lout(lin), m.cout), dtype=x.dtype, device=x.device)
    if y.shape != (nseq, m.lout(lin), m.cout) or y.dtype != x.dtype or not y.is_contiguous():
        raise L.EvtError("conv output buffer must be contiguous [nseq, Lout, Cout] in the compute dtype")
    if res is not None and (res.shape != y.shape or not res.is_contiguous() or res.dtype != x.dtype):
        raise L.EvtError("residual must match the output")
    p = slot.params(nseq, lin, in_slope, out_act, out_slope)
    e0 = T.t0()
    L.check(L.lib().evt_conv1d_fwd(C.byref(p), L.ptr(x), L.ptr(slot.reg), L.ptr(slot.alt), L.ptr(_bias(m)), L.ptr(res),
                                   L.ptr(y), L.stream_ptr()), "evt_conv1d_fwd")
    if e0 is not None:
        T.t1_conv(e0, "fwd", m, nseq, lin, y.numel() if res is not None else 0)
    return y


def _bwd_data(slot, dy, y, x, dx_add, nseq, lin, in_slope, out_act, out_slope):
    m = slot.module
    dx = torch.empty((nseq, lin, m.cin), dtype=dy.dtype, device=dy.device)
    p = slot.params(nseq, lin, in_slope, out_act, out_slope)
    e0 = T.t0()
    L.check(L.lib().evt_conv1d_bwd_data(C.byref(p), L.ptr(dy), L.ptr(y if out_act != L.ACT_NONE else None),
                                        L.ptr(slot.reg), L.ptr(slot.alt), L.ptr(x if in_slope != 1.0 else None),
                                        L.ptr(dx_add), L.ptr(dx), L.stream_ptr()), "evt_conv1d_bwd_data")
    if e0 is not None:
        extra = (dy.numel() if out_act != L.ACT_NONE else 0) + (dx.numel() if in_slope != 1.0 else 0) + \
                (dx.numel() if dx_add is not None else 0)
        T.t1_conv(e0, "bwd_data", m, nseq, lin, extra)
    return dx


def _lrelu(x, slope, owner=None):
    out = torch.empty_like(x)
    e0 = T.t0()
    L.check(L.lib().evt_leaky_relu(L.dt_of(x), L.ptr(x), float(slope), L.ptr(out), x.numel(), L.stream_ptr()),
            "evt_leaky_relu")
    if e0 is not None:
        T.t1_elt(e0, "lrelu_kernel", 2 * x.numel() * x.element_size(), owner)
    return out


def _add3(a, b, c, scale, out, owner):
    e0 = T.t0()
    L.check(L.lib().evt_add3_scale(L.dt_of(a), L.ptr(a), L.ptr(b), L.ptr(c), float(scale), L.ptr(out), a.numel(),
                                   L.stream_ptr()), "evt_add3_scale")
    if e0 is not None:
        T.t1_elt(e0, "add3_scale_kernel", (2 + (b is not None) + (c is not None)) * a.numel() * a.element_size(), owner)
    return out


def mask_tail(x, lens, mul=1, owner=None):
    """x[s, t, :] = 0 for t >= lens[s] * mul, IN PLACE (x contiguous [nseq, L, C], lens int32 [nseq] on x's device): the dead
    tails of a ragged batch in front of a consumer that has no masked load (csrc/elementwise.hip::evt_mask_tail)"""
    if x.dim() != 3 or not x.is_contiguous():
        raise L.EvtError("mask_tail takes a contiguous [nseq, L, C] tensor")
    L.check_lens("mask_tail", x, lens, mul)
    e0 = T.t0()
    L.check(L.lib().evt_mask_tail(L.dt_of(x), L.ptr(x), L.ptr(lens), int(mul), x.size(0), x.size(1), x.size(2),
                                  L.stream_ptr()), "evt_mask_tail")
    if e0 is not None:
        T.t1_elt(e0, "mask_tail_kernel", x.numel() * x.element_size(), owner)
    return x


def resample_rows(x, in_lens, out_lens, Lout, owner=None):
    """x [nseq, Lin, C] contiguous -> y [nseq, Lout, C]: row s resampled linearly from in_lens[s] to out_lens[s] positions
    (F.interpolate(mode="linear") on the row alone, evaluated in fp32), zero behind out_lens[s]; in_lens / out_lens int32
    [nseq] on x's device.  x is not read behind a row's in_lens and all of y is written
    (csrc/elementwise.hip::evt_resample_rows)"""
    if x.dim() != 3 or not x.is_contiguous() or int(Lout) < 1:
        raise L.EvtError("resample_rows takes a contiguous [nseq, Lin, C] tensor and Lout >= 1")
    L.check_lens("resample_rows", x, in_lens)
    L.check_lens("resample_rows", x, out_lens)
    y = torch.empty(x.size(0), int(Lout), x.size(2), dtype=x.dtype, device=x.device)
    e0 = T.t0()
    L.check(L.lib().evt_resample_rows(L.dt_of(x), L.ptr(x), L.ptr(in_lens), L.ptr(out_lens), x.size(0), x.size(1),
                                      int(Lout), x.size(2), L.ptr(y), L.stream_ptr()), "evt_resample_rows")
    if e0 is not None:
        T.t1_elt(e0, "resample_rows_kernel", (x.numel() + y.numel()) * x.element_size(), owner)
    return y
