"""GPU: seg_flat_kernel (csrc/elementwise.hip) through its four entry points evt_l1_multi_fwd / _bwd and evt_lsgan_multi_fwd /
_bwd, on tables built with L.Seg / struct_to_device, and the wrappers of module/losses.py on top of them.

Exact where it can be (tests/loss_refs.py): with dyadic operands every term times its scale is a multiple of one unit and
the whole sum stays below 2^24 units (tests/test_loss_refs_cpu.py), so fp32 accumulation is exact in any order and the
forward has to equal the float64 sum bit for bit -- across the head / 16-byte body / tail split, the scalar path of
misaligned bases, chunks of 2048 (or 4096) elements that cut segments anywhere, NULL gradients and the 64-segment limit.
The L1 gradient is +-float32(dloss * scale) rounded to the stored type or an exact 0, for any scale; the LSGAN gradient is
exact on dyadic operands and within 1 ulp of the stored type of the float32 op-by-op value on random ones.  Every gradient
buffer has 256 sentinel elements on either side.

The wrappers run on random operands rounded to the stored type: forward |d| <= 600 u loss (u = 2^-24; all terms are
non-negative and the summation depth across thread, block tree and 512 atomics stays below 600), backward as above.
"""
import ctypes as C

import pytest
import torch

import loss_refs as R

pytestmark = pytest.mark.gpu

G = 256                 # sentinel elements on either side (a multiple of 16 bytes in every type)
SENT = -4096.0          # exact in every stored type, outside the operands' and the gradients' range
ENOTSUP = 95
DTYPES = [torch.float32, torch.bfloat16]


class _Buf:
    """n elements at a 16-byte boundary (off = 0) or one element past it (off = 1), sentinels all around"""

    def __init__(self, n, dtype, dev, off=0, values=None):
        self.whole = torch.full((n + 2 * G + 1,), SENT, dtype=dtype, device=dev)
        self.lo, self.hi = G + off, G + off + n
        self.view = self.whole[self.lo:self.hi]
        assert (self.view.data_ptr() % 16 == 0) == (off == 0)
        if values is not None:
            self.view.copy_(values.to(dtype))

    def guards_intact(self):
        return bool((self.whole[:self.lo] == SENT).all()) and bool((self.whole[self.hi:] == SENT).all())

    def untouched(self):
        return bool((self.whole == SENT).all())


def _launch(L, dev, dtype, mode, a_list, b_list, scales, target=0.0, bwd=False, offs=(0, 0, 0), null_da=(), preset=0.0,
            dloss=R.SEG_DLOSS, expect=0):
    """one launch over the table; forward -> out as a python float, backward -> the list of gradient buffers"""
    lib, nseg = L.lib(), len(a_list)
    a_bufs = [_Buf(a.numel(), dtype, dev, offs[0], a) for a in a_list]
    b_bufs = [_Buf(b.numel(), dtype, dev, offs[1], b) for b in b_list] if mode == 0 else [None] * nseg
    da_bufs = [_Buf(a.numel(), dtype, dev, offs[2]) for a in a_list] if bwd else [None] * nseg
    segs = [L.Seg(a.view.data_ptr(), b.view.data_ptr() if b is not None else None,
                  da.view.data_ptr() if da is not None and i not in null_da else None, a.view.numel(), sc, 0)
            for i, (a, b, da, sc) in enumerate(zip(a_bufs, b_bufs, da_bufs, scales))]
    tab = L.struct_to_device(segs, dev)
    dt = L.dt_code(dtype)
    out = torch.full((1,), preset, dtype=torch.float32, device=dev)
    dl = torch.full((1,), dloss, dtype=torch.float32, device=dev)
    if mode == 0:
        rc = lib.evt_l1_multi_bwd(dt, L.ptr(tab), nseg, L.ptr(dl), L.stream_ptr()) if bwd else \
            lib.evt_l1_multi_fwd(dt, L.ptr(tab), nseg, L.ptr(out), L.stream_ptr())
    else:
        rc = lib.evt_lsgan_multi_bwd(dt, L.ptr(tab), nseg, C.c_float(target), L.ptr(dl), L.stream_ptr()) if bwd else \
            lib.evt_lsgan_multi_fwd(dt, L.ptr(tab), nseg, C.c_float(target), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, rc
    for b in a_bufs + [b for b in b_bufs if b is not None]:
        assert b.guards_intact()
    return da_bufs if bwd else float(out[0])


def _expect_l1_grad(a, b, dloss, scale, dtype):
    dl = R.f32_product(dloss, scale)
    return (torch.sign(a - b) * dl).float().to(dtype)


def _expect_lsgan_grad(a, target, dloss, scale, dtype):
    return R.lsgan_grad_f32(a, target, R.f32_product(dloss, scale)).to(dtype)


def _assert_grads(da_bufs, want_list, null_da=(), max_ulp=0, what=""):
    for i, (buf, want) in enumerate(zip(da_bufs, want_list)):
        assert buf.guards_intact(), f"{what} segment {i}: a sentinel around da was overwritten"
        if i in null_da:
            assert buf.untouched(), f"{what} segment {i}: da = NULL, yet its buffer was written"
            continue
        got = buf.view.cpu()
        if max_ulp == 0:
            bad = torch.nonzero(got != want).flatten()
            assert bad.numel() == 0, (f"{what} segment {i} (n = {want.numel()}): {bad.numel()} elements differ, first at "
                                      f"{bad[:6].tolist()}: got {got[bad[:6]].tolist()} want {want[bad[:6]].tolist()}")
        else:
            d = R.ulps_of(got, want)
            assert int(d.max()) <= max_ulp, f"{what} segment {i}: {int(d.max())} ulp at {int(d.argmax())}"


# ---- case bodies (also called with torch.float16 by tests/test_fp16_ops_gpu.py) -------------------------------------------
def dyadic_case(dev, dtype, name):
    from easevoice_trainer_amd.hip import lib as L

    a_list, b_list = R.seg_operands(name)
    scales = R.seg_scales(name)
    nseg = len(a_list)
    runs = [(0, 0.0)] + [(1, t) for t in R.SEG_TARGETS]
    for mode, target in runs:
        count, unit = R.seg_units(name, mode, target)
        assert count < R.F32_EXACT
        want = R.seg_loss64(name, mode, target)
        # forward: the float64 sum bit for bit; `out` accumulates
        got = _launch(L, dev, dtype, mode, a_list, b_list, scales, target)
        assert got == want, f"{name} mode {mode} target {target}: {got!r} against {want!r} ({(got - want) / unit} units)"
        got = _launch(L, dev, dtype, mode, a_list, b_list, scales, target, preset=R.SEG_PRESET)
        assert got == R.SEG_PRESET + want, f"{name} mode {mode} target {target}: preset + loss {got!r}"
        # backward, with every second gradient NULL
        null_da = set(range(1, nseg, 2))
        for nulls in ((), null_da):
            das = _launch(L, dev, dtype, mode, a_list, b_list, scales, target, bwd=True, null_da=nulls)
            if mode == 0:
                wants = [_expect_l1_grad(a, b, R.SEG_DLOSS, sc, dtype) for a, b, sc in zip(a_list, b_list, scales)]
            else:
                wants = [(-2.0 * (target - a) * (R.SEG_DLOSS * sc)).to(dtype) for a, sc in zip(a_list, scales)]
                for w, a, sc in zip(wants, a_list, scales):
                    assert torch.equal(w.double(), -2.0 * (target - a) * (R.SEG_DLOSS * sc))    # exact in the stored type
            _assert_grads(das, wants, nulls, 0, f"{name} mode {mode} target {target}")
    # an all-zero loss leaves `out` alone (L1 of a with itself, LSGAN of the target itself)
    assert _launch(L, dev, dtype, 0, a_list, a_list, scales, preset=0.375) == 0.375
    ones = [torch.ones_like(a) for a in a_list]
    assert _launch(L, dev, dtype, 1, ones, ones, scales, 1.0, preset=0.375) == 0.375
    # the L1 gradient with any scales: 2 / numel and an odd dloss; exactly 0 where a == b (loss_refs.seg_planted: head, body and tail elements)
    odd = [2.0 / a.numel() for a in a_list]
    das = _launch(L, dev, dtype, 0, a_list, b_list, odd, bwd=True, dloss=0.7)
    wants = [_expect_l1_grad(a, b, 0.7, sc, dtype) for a, b, sc in zip(a_list, b_list, odd)]
    for w, pos in zip(wants, R.seg_planted(R.SEG_LISTS[name]["sizes"])):
        assert bool((w[pos] == 0).all())
    _assert_grads(das, wants, (), 0, f"{name} L1, scales 2 / numel")


def alignment_case(dev, dtype, name="cuts"):
    """a, b and da each based at a 16-byte boundary or one element past it: a misaligned operand sends the segment down the
    scalar path, and the result has to be the aligned run's"""
    from easevoice_trainer_amd.hip import lib as L

    a_list, b_list = R.seg_operands(name)
    scales = R.seg_scales(name)
    for mode, target in [(0, 0.0), (1, 1.0)]:
        want = R.seg_loss64(name, mode, target)
        ref_grads = None
        for oa in (0, 1):
            for ob in ((0, 1) if mode == 0 else (0,)):
                got = _launch(L, dev, dtype, mode, a_list, b_list, scales, target, offs=(oa, ob, 0))
                assert got == want, f"mode {mode} offsets a {oa} b {ob}: {got!r} against {want!r}"
                for oda in (0, 1):
                    das = _launch(L, dev, dtype, mode, a_list, b_list, scales, target, bwd=True, offs=(oa, ob, oda))
                    grads = [d.view.cpu() for d in das]
                    assert all(d.guards_intact() for d in das), f"mode {mode} offsets {(oa, ob, oda)}: sentinel overwritten"
                    if ref_grads is None:
                        ref_grads = grads
                        if mode == 0:
                            wants = [_expect_l1_grad(a, b, R.SEG_DLOSS, sc, dtype) for a, b, sc in zip(a_list, b_list, scales)]
                        else:
                            wants = [(-2.0 * (target - a) * (R.SEG_DLOSS * sc)).to(dtype) for a, sc in zip(a_list, scales)]
                        _assert_grads(das, wants, (), 0, f"mode {mode} aligned")
                    for i, (g, r) in enumerate(zip(grads, ref_grads)):
                        assert torch.equal(g, r), f"mode {mode} offsets {(oa, ob, oda)} segment {i} differs from the aligned run"


# ---- tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SEG_LISTS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_dyadic_operands_are_exact(gpu, dtype, name):
    dyadic_case(gpu, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_alignment_combinations(gpu, dtype):
    alignment_case(gpu, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_lsgan_backward_random_operands(gpu, dtype):
    from easevoice_trainer_amd.hip import lib as L

    sizes = R.SEG_LISTS["cuts"]["sizes"]
    a_list, _ = R.seg_random(sizes, dtype)
    scales = [1.0 / n for n in sizes]
    for target in R.SEG_TARGETS:
        das = _launch(L, gpu, dtype, 1, a_list, a_list, scales, target, bwd=True, dloss=0.7, null_da={2})
        wants = [_expect_lsgan_grad(a, target, 0.7, sc, dtype) for a, sc in zip(a_list, scales)]
        _assert_grads(das, wants, {2}, 1, f"random LSGAN target {target}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_segment_limit(gpu, dtype):
    """64 segments are served (test_dyadic_operands_are_exact[many]); 65 are refused and nothing is written"""
    from easevoice_trainer_amd.hip import lib as L

    a_list, b_list = R.seg_operands("many")
    a65, b65 = a_list + a_list[:1], b_list + b_list[:1]
    sc = R.seg_scales("many") + [1.0]
    assert len(a_list) == 64
    for mode in (0, 1):
        assert _launch(L, gpu, dtype, mode, a65, b65, sc, 1.0, preset=R.SEG_PRESET, expect=ENOTSUP) == R.SEG_PRESET
        das = _launch(L, gpu, dtype, mode, a65, b65, sc, 1.0, bwd=True, expect=ENOTSUP)
        assert all(d.untouched() for d in das)


WRAP_SIZES = [7, 9, 2047, 2049, 4099]


def _leaves(vals, dtype, dev):
    return [v.to(dtype).to(dev).requires_grad_(True) for v in vals]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_wrappers_against_float64(gpu, dtype):
    from easevoice_trainer_amd.module import losses as ML

    a64, b64 = R.seg_random(WRAP_SIZES, dtype)
    up = 0.75                                               # dloss: the loss is scaled before backward()
    tol = 600 * R.U

    def close(got, want, what):
        got = float(got.detach())
        assert abs(got - want) <= tol * want, f"{what}: {got!r} against {want!r}"

    # feature_loss: 2 sum_i mean|r_i - g_i|, two discriminators' maps
    g = _leaves(a64, dtype, gpu)
    r = [v.to(dtype).to(gpu) for v in b64]
    loss = ML.feature_loss([r[:2], r[2:]], [g[:2], g[2:]])
    close(loss, 2.0 * sum(float((a - b).abs().mean()) for a, b in zip(a64, b64)), "feature_loss")
    (loss * up).backward()
    for t, a, b in zip(g, a64, b64):
        assert torch.equal(t.grad.cpu(), _expect_l1_grad(a, b, up, 2.0 / a.numel(), dtype))

    # l1_mean_scaled: scale * mean|a - b|
    g = _leaves(a64[4:], dtype, gpu)
    loss = ML.l1_mean_scaled(g[0], r[4], 45.0)
    close(loss, 45.0 * float((a64[4] - b64[4]).abs().mean()), "l1_mean_scaled")
    (loss * up).backward()
    assert torch.equal(g[0].grad.cpu(), _expect_l1_grad(a64[4], b64[4], up, 45.0 / a64[4].numel(), dtype))

    # generator_loss: sum_i mean((1 - dg_i)^2)
    g = _leaves(a64, dtype, gpu)
    loss = ML.generator_loss(g)
    close(loss, sum(float(((1.0 - a) ** 2).mean()) for a in a64), "generator_loss")
    (loss * up).backward()
    for t, a in zip(g, a64):
        assert int(R.ulps_of(t.grad.cpu(), _expect_lsgan_grad(a, 1.0, up, 1.0 / a.numel(), dtype)).max()) <= 1

    # discriminator_loss: sum_i mean((1 - dr_i)^2) + mean(dg_i^2)
    dr, dg = _leaves(b64, dtype, gpu), _leaves(a64, dtype, gpu)
    loss = ML.discriminator_loss(dr, dg)
    close(loss, sum(float(((1.0 - b) ** 2).mean()) + float((a ** 2).mean()) for a, b in zip(a64, b64)), "discriminator_loss")
    (loss * up).backward()
    for t, v, target in [(t, b, 1.0) for t, b in zip(dr, b64)] + [(t, a, 0.0) for t, a in zip(dg, a64)]:
        assert int(R.ulps_of(t.grad.cpu(), _expect_lsgan_grad(v, target, up, 1.0 / v.numel(), dtype)).max()) <= 1

    # discriminator_loss_batched: logits [real ; generated]; 3 x 37 elements per half: in 16 bits the second half starts
    # off a 16-byte boundary
    o64, _ = R.seg_random([6 * 37, 6 * 5], dtype, seed=1)
    outs = [t.reshape(6, 1, -1) for t in _leaves(o64, dtype, gpu)]
    for o in outs:
        o.retain_grad()
    loss = ML.discriminator_loss_batched(outs)
    halves = [(v[: v.numel() // 2], v[v.numel() // 2:]) for v in o64]
    close(loss, sum(float(((1.0 - re) ** 2).mean()) + float((ge ** 2).mean()) for re, ge in halves), "discriminator_loss_batched")
    (loss * up).backward()
    for o, (re, ge) in zip(outs, halves):
        got = o.grad.reshape(-1).cpu()
        want = torch.cat([_expect_lsgan_grad(re, 1.0, up, 1.0 / re.numel(), dtype),
                          _expect_lsgan_grad(ge, 0.0, up, 1.0 / ge.numel(), dtype)])
        assert int(R.ulps_of(got, want).max()) <= 1
