"""HiFi-GAN ResBlock1 steps and stages on the fused kernels (csrc/resunit.hip, resunit_wide.hip, resunit_bwd.hip): which
kernel covers a step, the autograd Functions, the no-grad paths for ragged batches."""
import ctypes as C

import torch

from . import lib as L
from . import trace as T
from .launch import _add3, _bias, _bwd_data, _dptr, _fwd, _lrelu, mask_tail
from .wgrad import WgJob, _bwd_weight, _dbias_of

NARROW, WIDE = "narrow", "wide"    # C = 16 / 32 (csrc/resunit.hip) and C = 64 / 128 (csrc/resunit_wide.hip)
_FWD_ENTRY = {NARROW: "evt_resunit_fwd", WIDE: "evt_resunit_wide_fwd"}


def _unit_kind(s1, s2, x, slope):
    """(evt_resunit_params, NARROW | WIDE) when a fused ResBlock step covers this pair of convolutions and input, else
    (None, None).  Narrow is asked first."""
    m1, m2 = s1.module, s2.module
    if (not L.is_half(x.dtype) or not x.is_cuda or not x.is_contiguous() or x.dim() != 3 or m1.cin != m1.cout
            or m2.cin != m2.cout or m1.cin != m2.cin or m1.k != m2.k or m2.dil != 1 or m1.stride != 1 or m2.stride != 1
            or m1.groups != 1 or m2.groups != 1 or m1.transposed or m2.transposed
            or m1.pad != m1.dil * (m1.k - 1) // 2 or m2.pad != (m2.k - 1) // 2 or s1.bank.impl != L.IMPL_AUTO):
        return None, None
    p = L.ResUnitParams(L.dt_code(x.dtype), x.size(0), x.size(1), m1.cin, m1.k, m1.dil, float(slope))
    if L.lib().evt_resunit_supported(C.byref(p)):
        return p, NARROW
    if L.lib().evt_resunit_wide_supported(C.byref(p)):
        return p, WIDE
    return None, None


def _resunit_params(s1, s2, x, slope, kind=NARROW):
    """evt_resunit_params when the fused step of this kind covers the pair of convolutions and input, else None"""
    p, k = _unit_kind(s1, s2, x, slope)
    return p if k == kind else None


def _resunit_wide_params(s1, s2, x, slope):
    return _resunit_params(s1, s2, x, slope, WIDE)


def _fwd_job(jb, p, x, s1, s2, xa, mid_a, y):
    """fill one evt_resunit_fwd_job (xa / mid_a None: a no-grad launch keeps nothing for a backward)"""
    jb.p = p
    jb.x, jb.w1_reg, jb.w2_reg = x.data_ptr(), s1.reg.data_ptr(), s2.reg.data_ptr()
    jb.b1, jb.b2 = _dptr(_bias(s1.module)), _dptr(_bias(s2.module))
    jb.xa, jb.mid_a, jb.y = _dptr(xa), _dptr(mid_a), y.data_ptr()


def _t1_units(e0, kind, pairs, x, wg, single=False):
    """trace record of one fused launch over the steps `pairs`: flops of both convolutions of every step (+ both weight
    gradients: wg); bytes = per step x in and xa / mid_a / y out (backward: dy, xa, mid_a in, dx out), both weight images
    (+ both fp32 gradient images)"""
    n, ln, c = x.shape
    macs = sum(n * ln * c * c * (s1.module.k + s2.module.k) for s1, s2 in pairs) * (2 if wg else 1)
    wb = sum(s1.module.v.numel() + s2.module.v.numel() for s1, s2 in pairs) * (2 + (4 if wg else 0))
    m1 = pairs[0][0].module
    if single:
        shape = f"unit {c}>{c} k{m1.k} d{m1.dil} n{n} L{ln}"
    else:
        shape = f"units x{len(pairs)} {c}>{c} k" + "/".join(str(s1.module.k) for s1, _ in pairs) + f" d{m1.dil} n{n} L{ln}"
    T.t1(e0, None, kind, 2 * macs, len(pairs) * 4 * x.numel() * 2 + wb, shape, m1)


def _unit_wgrads(s1, s2, xa, mid_a, dy, dmid):
    nseq, lin = xa.size(0), xa.size(1)
    _bwd_weight(s2, mid_a, dy, None, nseq, lin, 1.0, L.ACT_NONE, 1.0)
    _bwd_weight(s1, xa, dmid, None, nseq, lin, 1.0, L.ACT_NONE, 1.0)


class ResUnitFn(torch.autograd.Function):
    """HiFi-GAN ResBlock1 inner step  y = x + c2(lrelu(c1(lrelu(x))))  (modules.py:299-308).
    Forward: xa = lrelu(x) (one element-wise launch), mid_a = lrelu(c1(xa)) (activation = c1's epilogue),
    y = c2(mid_a) + x (residual = c2's epilogue).  Every convolution and weight gradient therefore sees PLAIN operands
    and runs on the LDS-DMA kernels; the two leaky-relu derivatives are the gate epilogues of the backward-data
    launches (the sign of lrelu(v) is the sign of v), the residual gradient is the second one's add epilogue."""

    @staticmethod
    def forward(ctx, x, anchor, s1, s2, slope):
        p, kind = _unit_kind(s1, s2, x, slope)
        if p is not None:
            # one launch, which also writes the two activated tensors the backward launches below take: narrow stages
            # (C = 16 / 32) csrc/resunit.hip; wide (C = 64 / 128) csrc/resunit_wide.hip, the intermediate stays in LDS
            m1, m2 = s1.module, s2.module
            xa, mid_a, y = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            entry = _FWD_ENTRY[kind]
            e0 = T.t0()
            L.check(getattr(L.lib(), entry)(C.byref(p), L.ptr(x), L.ptr(s1.reg), L.ptr(s2.reg), L.ptr(_bias(m1)),
                                            L.ptr(_bias(m2)), L.ptr(xa), L.ptr(mid_a), L.ptr(y), L.stream_ptr()), entry)
            if e0 is not None:
                _t1_units(e0, "fwd", [(s1, s2)], x, False, single=True)
        else:
            xa = _lrelu(x, slope, s1.module)
            mid_a = _fwd(s1, xa, None, 1.0, L.ACT_LRELU, slope)
            y = _fwd(s2, mid_a, x, 1.0, L.ACT_NONE, 1.0)
        ctx.s1, ctx.s2, ctx.slope = s1, s2, slope
        ctx.save_for_backward(xa, mid_a)
        return y

    @staticmethod
    def backward(ctx, dy):
        xa, mid_a = ctx.saved_tensors
        s1, s2, slope = ctx.s1, ctx.s2, ctx.slope
        dy = dy.contiguous()
        nseq, lin = xa.size(0), xa.size(1)
        if ctx.needs_input_grad[0]:
            p, kind = _unit_kind(s1, s2, xa, slope)
            if kind == NARROW:
                dx = _narrow_bwd(p, s1, s2, dy, xa, mid_a, 1.0)
                if dx is not None:
                    return dx, None, None, None, None
            elif kind == WIDE:
                dmid, dx = torch.empty_like(dy), torch.empty_like(dy)
                e0 = T.t0()
                L.check(L.lib().evt_resunit_wide_bwd_data(C.byref(p), L.ptr(dy), 1.0, L.ptr(xa), L.ptr(mid_a),
                                                          L.ptr(s1.alt), L.ptr(s2.alt), L.ptr(dmid), L.ptr(dx),
                                                          L.stream_ptr()), "evt_resunit_wide_bwd_data")
                if e0 is not None:
                    _t1_units(e0, "bwd_unit", [(s1, s2)], xa, False, single=True)
                if s2.bank.weight_grads:
                    _unit_wgrads(s1, s2, xa, mid_a, dy, dmid)
                return dx, None, None, None, None
        if s2.bank.weight_grads:
            _bwd_weight(s2, mid_a, dy, None, nseq, lin, 1.0, L.ACT_NONE, 1.0)
        # d(c1 output before its activation) = (W2^T dy) * lrelu'(mid): gate epilogue on mid_a
        dmid = _bwd_data(s2, dy, None, mid_a, None, nseq, lin, slope, L.ACT_NONE, 1.0)
        if s1.bank.weight_grads:
            _bwd_weight(s1, xa, dmid, None, nseq, lin, 1.0, L.ACT_NONE, 1.0)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _bwd_data(s1, dmid, None, xa, dy, nseq, lin, slope, L.ACT_NONE, 1.0)
        return dx, None, None, None, None


def resunit_bwd(s1, s2, dy, xa, mid_a, slope, dy_scale=1.0):
    """The whole backward of one ResBlock1 step in one launch (csrc/resunit_bwd.hip) when the shape is covered: returns
    dx (and leaves the weight / bias gradients of both convolutions in their gradient images / .grad), else None.
    Where the kernel takes the data gradients but not the weight gradients (C = 32 with 11 taps: the accumulators do
    not fit the register file) it also writes dmid and the two weight gradients run as their own launches."""
    fused = _resunit_params(s1, s2, xa, slope)
    return _narrow_bwd(fused, s1, s2, dy, xa, mid_a, dy_scale) if fused is not None else None


def _narrow_bwd(fused, s1, s2, dy, xa, mid_a, dy_scale):
    lib = L.lib()
    bank = s1.bank
    wg = bool(bank.weight_grads)
    wg_in = wg and bool(lib.evt_resunit_bwd_supported(C.byref(fused), 1))
    if not lib.evt_resunit_bwd_supported(C.byref(fused), 0):
        return None
    if wg and not wg_in and dy_scale != 1.0:
        return None
    m1, m2 = s1.module, s2.module
    dx = torch.empty_like(dy)
    dmid = torch.empty_like(dy) if (wg and not wg_in) else None
    dw1 = dw2 = db1 = db2 = ws = None
    if wg_in:
        dw1, dw2 = s1.dw, s2.dw
        db1, db2 = _dbias_of(m1), _dbias_of(m2)
        ws = bank.scratch()
    e0 = T.t0()
    L.check(lib.evt_resunit_bwd(C.byref(fused), L.ptr(dy), float(dy_scale), L.ptr(xa), L.ptr(mid_a), L.ptr(s1.alt),
                                L.ptr(s2.alt), L.ptr(dx), L.ptr(dmid), L.ptr(dw1), L.ptr(dw2), L.ptr(db1), L.ptr(db2),
                                L.ptr(ws), ws.numel() if ws is not None else 0, L.stream_ptr()),
            "evt_resunit_bwd")
    if e0 is not None:
        _t1_units(e0, "bwd_unit", [(s1, s2)], xa, wg_in, single=True)
        if wg_in:
            T.t1_elt(T.t0(), "fold_partials_multi", (s1.layout.reg_elems + s2.layout.reg_elems) * 4 * 256, m1)
    if wg_in:
        s1.wg_dirty = s2.wg_dirty = True
    elif wg:
        _unit_wgrads(s1, s2, xa, mid_a, dy, dmid)
    return dx


def _res_unit_lens(x, s1, s2, slope, lens, mul):
    """res_unit on a ragged batch, no grad: row s is live on [0, lens[s] * mul) and comes out with a zero tail.  Narrow, wide
    or unfused exactly as ResUnitFn.forward chooses; the unfused path expects x with a zero tail already (the fused kernels
    mask their loads) and masks behind each of its two convolutions, whose biases fill the tail."""
    L.check_lens("res_unit", x, lens, mul)
    m1, m2 = s1.module, s2.module
    lib = L.lib()
    p, kind = _unit_kind(s1, s2, x, slope)
    if p is not None:
        y = torch.empty_like(x)
        e0 = T.t0()
        if kind == NARROW:
            jobs = (L.ResUnitFwdJob * 1)()
            _fwd_job(jobs[0], p, x, s1, s2, None, None, y)
            L.check(lib.evt_resunit_fwd_multi_lens(jobs, 1, L.ptr(lens), int(mul), L.stream_ptr()),
                    "evt_resunit_fwd_multi_lens")
        else:
            L.check(lib.evt_resunit_wide_fwd_lens(C.byref(p), L.ptr(x), L.ptr(s1.reg), L.ptr(s2.reg), L.ptr(_bias(m1)),
                                                  L.ptr(_bias(m2)), L.ptr(None), L.ptr(None), L.ptr(y), L.ptr(lens), int(mul),
                                                  L.stream_ptr()), "evt_resunit_wide_fwd_lens")
        if e0 is not None:
            _t1_units(e0, "fwd", [(s1, s2)], x, False, single=True)
        return y
    xa = _lrelu(x, slope, m1)
    mid_a = mask_tail(_fwd(s1, xa, None, 1.0, L.ACT_LRELU, slope), lens, mul, m1)
    return mask_tail(_fwd(s2, mid_a, x, 1.0, L.ACT_NONE, 1.0), lens, mul, m2)


def res_unit(x, c1, c2, slope: float, lens=None, mul: int = 1):
    """c1, c2: the step's two EvtConv1d.  lens (int32 [nseq], in units of `mul` positions): the no-grad path for a ragged
    batch, see _res_unit_lens"""
    if lens is not None:
        return _res_unit_lens(x, c1._slot, c2._slot, float(slope), lens, mul)
    return ResUnitFn.apply(x, c1._slot.bank.anchor, c1._slot, c2._slot, float(slope))


def _stage_plan(x, blocks, slope):
    """[(slot pairs of unit j over the blocks)] when every step of the stage is covered by the grouped kernels: the blocks
    have kernel sizes 3 / 7 / 11 (one each), equally many steps, and every step passes _resunit_params"""
    if not x.is_cuda or not L.is_half(x.dtype) or len(blocks) != 3:
        return None
    nunits = len(blocks[0].convs1)
    if any(len(b.convs1) != nunits or len(b.convs2) != nunits for b in blocks):
        return None
    if sorted(b.convs1[0].k for b in blocks) != [3, 7, 11]:
        return None
    plan = []
    for j in range(nunits):
        pairs = [(b.convs1[j]._slot, b.convs2[j]._slot) for b in blocks]
        if any(s1 is None or s2 is None for s1, s2 in pairs):
            return None
        ps = [_resunit_params(s1, s2, x, slope) for s1, s2 in pairs]
        if any(p is None for p in ps):
            return None
        plan.append((pairs, ps))
    return plan


class ResStageFn(torch.autograd.Function):
    """One HiFi-GAN stage after its up-sampling convolution (models.py:457-466): the three ResBlock1 of kernel sizes
    3 / 7 / 11 applied to the same input and averaged.  Step j of all three blocks is ONE grouped launch each way
    (csrc/resunit.hip, resunit_bwd.hip), so a stage is 3 + 1 launches forward and 3 + 1 (+ 1 fold each) backward instead
    of 9 + 1 and 36 + 2.  The 1 / 3 of the mean is folded into the first backward launch's load of dy."""

    @staticmethod
    def forward(ctx, x, anchor, plan, slope, scale):
        saved = []
        out = _stage_fwd(x, plan, scale, saved)
        ctx.plan, ctx.slope, ctx.scale = plan, slope, scale
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        plan, slope, scale = ctx.plan, ctx.slope, ctx.scale
        saved = ctx.saved_tensors
        dy = dy.contiguous()
        nb = len(plan[0][0])
        bank = plan[0][0][0][0].bank
        wg = bool(bank.weight_grads)
        # which jobs accumulate their weight gradients in the launch (all but C = 32 with 11 taps)
        in_k = [[wg and bool(lib.evt_resunit_bwd_supported(C.byref(p), 1)) for p in ps] for _, ps in plan]
        fold_scale = all(all(r) for r in in_k) or not wg
        owner = plan[0][0][0][0].module
        if not fold_scale:
            dy = _add3(dy, None, None, scale, torch.empty_like(dy), owner)
        d = [dy] * nb
        ws = bank.scratch() if wg else None
        nseq, lin = dy.size(0), dy.size(1)
        for j in range(len(plan) - 1, -1, -1):
            pairs, ps = plan[j]
            jobs = (L.ResUnitBwdJob * nb)()
            outs, later = [], []
            for i, ((s1, s2), p) in enumerate(zip(pairs, ps)):
                xa, mid_a = saved[2 * (j * nb + i)], saved[2 * (j * nb + i) + 1]
                dx = torch.empty_like(dy)
                jb = jobs[i]
                jb.p = p
                jb.dy_scale = scale if (fold_scale and j == len(plan) - 1) else 1.0
                jb.dy, jb.xa, jb.mid_a = d[i].data_ptr(), xa.data_ptr(), mid_a.data_ptr()
                jb.w1_alt, jb.w2_alt, jb.dx = s1.alt.data_ptr(), s2.alt.data_ptr(), dx.data_ptr()
                if in_k[j][i]:
                    jb.dw1, jb.dw2 = s1.dw.data_ptr(), s2.dw.data_ptr()
                    jb.db1, jb.db2 = _dptr(_dbias_of(s1.module)), _dptr(_dbias_of(s2.module))
                    s1.wg_dirty = s2.wg_dirty = True
                elif wg:
                    dmid = torch.empty_like(dy)
                    jb.dmid = dmid.data_ptr()
                    later += [WgJob(s2, mid_a, d[i], None, nseq, lin, 1.0, L.ACT_NONE, 1.0),
                              WgJob(s1, xa, dmid, None, nseq, lin, 1.0, L.ACT_NONE, 1.0)]
                outs.append(dx)
            e0 = T.t0()
            L.check(lib.evt_resunit_bwd_multi(jobs, nb, L.ptr(ws), ws.numel() if ws is not None else 0,
                                              L.stream_ptr()), "evt_resunit_bwd_multi")
            if e0 is not None:
                _t1_units(e0, "bwd_unit", pairs, dy, wg)
                if any(in_k[j]):       # the second launch of the call: the partial rows added into the gradient images
                    rows = sum(s1.layout.reg_elems + s2.layout.reg_elems for (s1, s2), k_ in zip(pairs, in_k[j]) if k_)
                    T.t1_elt(T.t0(), "fold_partials_multi", rows * 4 * 256, owner)
            for job in later:
                _bwd_weight(*job)
            d = outs
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _add3(d[0], d[1], d[2], 1.0, torch.empty_like(dy), owner)
        return dx, None, None, None, None


def _stage_fwd(x, plan, scale, saved=None, lens=None, mul=1):
    """the grouped forward launches of a stage and its mean.  saved: a list that receives xa / mid_a of every step (the
    autograd path).  lens: a ragged batch, no grad -- the launches mask their loads of x by the rows' lengths and store zero
    tails, so the stage mean has a zero tail too; nothing is kept for a backward"""
    lib = L.lib()
    cur = [x] * len(plan[0][0])
    for pairs, ps in plan:
        jobs = (L.ResUnitFwdJob * len(pairs))()
        outs = []
        for i, ((s1, s2), p) in enumerate(zip(pairs, ps)):
            keep = [torch.empty_like(x), torch.empty_like(x)] if saved is not None else [None, None]
            outs.append(torch.empty_like(x))
            _fwd_job(jobs[i], p, cur[i], s1, s2, keep[0], keep[1], outs[-1])
            if saved is not None:
                saved += keep
        e0 = T.t0()
        if lens is None:
            L.check(lib.evt_resunit_fwd_multi(jobs, len(pairs), L.stream_ptr()), "evt_resunit_fwd_multi")
        else:
            L.check(lib.evt_resunit_fwd_multi_lens(jobs, len(pairs), L.ptr(lens), int(mul), L.stream_ptr()),
                    "evt_resunit_fwd_multi_lens")
        if e0 is not None:
            _t1_units(e0, "fwd", pairs, x, False)
        cur = outs
    return _add3(cur[0], cur[1], cur[2], scale, torch.empty_like(x), plan[0][0][0][0].module)


def res_stage(x, blocks, slope: float, scale: float, lens=None, mul: int = 1):
    """mean over `blocks` (ResBlock1 modules) of block(x), through the grouped kernels; None when the stage is not covered
    (the caller then runs the blocks one by one).  lens (int32 [nseq], in units of `mul` positions): the no-grad path for a
    ragged batch, chosen by the same plan."""
    plan = _stage_plan(x, blocks, slope)
    if plan is None:
        return None
    lib = L.lib()
    # the grouped backward exists for every job shape the forward takes (data gradients at least)
    if not all(lib.evt_resunit_bwd_supported(C.byref(p), 0) for _, ps in plan for p in ps):
        return None
    # jobs are handed over in kernel-size order 3 / 7 / 11
    order = sorted(range(len(blocks)), key=lambda i: blocks[i].convs1[0].k)
    plan = [([pairs[i] for i in order], [ps[i] for i in order]) for pairs, ps in plan]
    if lens is not None:
        L.check_lens("res_stage", x, lens, mul)
        return _stage_fwd(x, plan, float(scale), None, lens, mul)
    return ResStageFn.apply(x, plan[0][0][0][0].bank.anchor, plan, float(slope), float(scale))
