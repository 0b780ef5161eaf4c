"""GPU: evt_resample_rows (csrc/elementwise.hip) -- the per-row linear resampler behind decode_batch(speed=...): row s of
x [nseq, Lin, C] goes from in_lens[s] to out_lens[s] positions as F.interpolate(mode="linear") does for the row alone, the
rest of y [nseq, Lout, C] is stored as zero, x is never read behind a row's end.

Rows of 64 (= Lin), 37, 2 and 1 positions, C = 8 (one 16-byte vector of a 16-bit type) and 192 (the model's), three
dtypes through the two builds.  x holds 1e4 behind every row's end, y 77 before the launch: a read of the tail, or an
element that was not written, shows."""
import ctypes as C

import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu
BIG = 1e4
FILL = 77.0
LIN = 64
TI = [64, 37, 2, 1]
SPEEDS = [0.5, 0.8, 1.25, 3.0]
EINVAL = 22
# (storage dtype, 16-bit type of the build that serves it): fp32 goes through both builds
CASES = [(torch.float32, torch.bfloat16), (torch.float32, torch.float16), (torch.bfloat16, torch.bfloat16),
         (torch.float16, torch.float16)]
IDS = ["f32", "f32-f16build", "bf16", "f16"]


def _x(gpu, dtype, C_):
    g = torch.Generator().manual_seed(1000 + C_)
    x = torch.randn(len(TI), LIN, C_, generator=g).to(dtype)
    for s, n in enumerate(TI):
        x[s, n:] = BIG
    return x.to(gpu)


def _launch(x, in_lens, out_lens, Lout, C_=None, x_ptr=None):
    """the C entry point on a y pre-filled with 77 -> (return code, y)"""
    from easevoice_trainer_amd.hip import lib as L

    nseq, Lin, Cx = x.shape
    y = torch.full((nseq, max(Lout, 1), Cx), FILL, dtype=x.dtype, device=x.device)
    il = torch.tensor(in_lens, dtype=torch.int32, device=x.device)
    ol = torch.tensor(out_lens, dtype=torch.int32, device=x.device)
    rc = L.lib().evt_resample_rows(L.dt_of(x), L.ptr(x) if x_ptr is None else x_ptr, L.ptr(il), L.ptr(ol), nseq, Lin,
                                   int(Lout), Cx if C_ is None else C_, L.ptr(y), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, y


def _out_lens(speed):
    return [int(n / speed) + 1 for n in TI]


@pytest.mark.parametrize("C_", [8, 192])
@pytest.mark.parametrize("dtype,half", CASES, ids=IDS)
def test_rows_against_float64_and_tails(gpu, dtype, half, C_):
    """Every row against F.interpolate(mode="linear") on the row alone in float64 (the reference model's operator,
    models.py:246-248), output lengths int(Ti / speed) + 1 for speed 0.5, 0.8, 1.25 and 3.

    Bound, fp32: |got - want| <= 2^-24 * (6 * Lin + 4) * max|x_row|.  The kernel evaluates
    src = max(scale * (j + 0.5) - 0.5, 0) with three fp32 roundings (the quotient scale = Ti / To, the product, the
    difference); each moves src by at most half a unit in the last place of a number <= Lin, i.e. Lin * 2^-24, so src
    is off by at most 3 * Lin * 2^-24.  The interpolant is continuous and piecewise linear in src with slope
    |x1 - x0| <= 2 * max|x|: 6 * Lin * 2^-24 * max|x|.  The weights 1 - l1 and l1, the two products and the sum add four
    roundings of numbers <= max|x|: 4 * 2^-24 * max|x|.  (l1 = src - i0 is exact.)  The 16-bit types add the one rounding
    of the result to storage, half a unit in its last place: 2^-8 * |want| for bfloat16, 2^-11 * |want| for float16.

    Tails: y[s, To:] is exactly zero, no 77 is left, and no |y| exceeds the largest live |x| of its row -- a linear
    interpolation is a convex combination, so a single tap on the 1e4 behind the row's end would show."""
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(half)
    x = _x(gpu, dtype, C_)
    xc = x.cpu()
    half_ulp = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    for speed in SPEEDS:
        to = _out_lens(speed)
        Lout = max(to) + 5
        rc, y = _launch(x, TI, to, Lout)
        assert rc == 0
        yc = y.cpu()
        assert int((yc == FILL).sum()) == 0, "every element of y is written"
        for s, (ti, n) in enumerate(zip(TI, to)):
            row = xc[s:s + 1, :ti].double()
            want = F.interpolate(row.transpose(1, 2), size=n, mode="linear").transpose(1, 2)[0]
            xmax = float(row.abs().max())
            err = (yc[s, :n].double() - want).abs()
            bound = 2.0 ** -24 * (6 * LIN + 4) * xmax + half_ulp * want.abs()
            print(f"{dtype} C={C_} speed={speed} row {s}: {ti} -> {n}, max err {float(err.max()):.3e}, "
                  f"bound at that place {float(bound.flatten()[err.argmax()]):.3e}")
            assert bool((err <= bound).all()), (speed, s, float(err.max()))
            assert int((yc[s, n:] != 0).sum()) == 0, ("tail of y must be stored as zero", speed, s)
            assert float(yc[s].abs().max()) <= xmax * (1 + 2.0 ** -20), ("x was read behind the row's end", speed, s)
            if ti == 1:
                assert torch.equal(yc[s, :n], xc[s, :1].expand(n, -1)), "one input position: every output is that position"


@pytest.mark.parametrize("dtype,half", CASES, ids=IDS)
def test_same_length_is_a_copy_and_one_position_repeats(gpu, dtype, half):
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(half)
    for C_ in (8, 192):
        x = _x(gpu, dtype, C_)
        rc, y = _launch(x, TI, TI, LIN + 6)
        assert rc == 0
        for s, ti in enumerate(TI):
            assert torch.equal(y[s, :ti], x[s, :ti]), (C_, s)
            assert int((y[s, ti:] != 0).sum()) == 0, (C_, s)
        # Ti = 1 stretched to 9 positions, Ti = 0 and To = 0 rows: all zero; lengths beyond the buffers are clamped
        rc, y = _launch(x, [1, 0, 37, 1000], [9, 9, 0, 1000], 9)
        assert rc == 0
        assert torch.equal(y[0], x[0, :1].expand(9, -1))
        assert int((y[1] != 0).sum()) == 0 and int((y[2] != 0).sum()) == 0
        rc, y3 = _launch(x[3:4], [LIN], [9], 9)
        assert rc == 0 and torch.equal(y[3], y3[0]), "in_lens / out_lens are clamped to Lin / Lout on the device"


@pytest.mark.parametrize("dtype,half", CASES, ids=IDS)
def test_row_of_a_batch_equals_the_row_alone(gpu, dtype, half):
    """row s of the batched launch is bit for bit the launch with nseq = 1, Lin = Ti, Lout = To on that row alone"""
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(half)
    for C_ in (8, 192):
        x = _x(gpu, dtype, C_)
        for speed in SPEEDS:
            to = _out_lens(speed)
            rc, y = _launch(x, TI, to, max(to) + 5)
            assert rc == 0
            for s, (ti, n) in enumerate(zip(TI, to)):
                rc, y1 = _launch(x[s:s + 1, :ti].contiguous(), [ti], [n], n)
                assert rc == 0 and torch.equal(y[s, :n], y1[0]), (C_, speed, s)


def test_argument_errors_launch_nothing(gpu):
    from easevoice_trainer_amd.hip import lib as L

    for half in (torch.bfloat16, torch.float16):
        L.set_half(half)
        x = torch.randn(2, 16, 24, device=gpu).to(half)
        for kw in (dict(C_=12), dict(x_ptr=C.c_void_p(0)), dict(Lout=0)):
            rc, y = _launch(x, [16, 5], [8, 8], kw.pop("Lout", 8), **kw)
            assert rc == EINVAL, kw
            assert bool((y == FILL).all()), "nothing was launched"
        # a base that is not 16-byte aligned: one element into a buffer that is long enough
        x8 = torch.randn(2 * 16 * 8 + 8, device=gpu).to(half)
        rc, y = _launch(x8[:256].view(2, 16, 8), [16, 5], [8, 8], 8, x_ptr=C.c_void_p(x8.data_ptr() + 2))
        assert rc == EINVAL and bool((y == FILL).all())
        # the other build's 16-bit code
        other = 2 if half == torch.bfloat16 else 1
        y = torch.full((2, 8, 24), FILL, dtype=half, device=gpu)
        il = torch.tensor([16, 5], dtype=torch.int32, device=gpu)
        rc = L.lib().evt_resample_rows(other, L.ptr(x), L.ptr(il), L.ptr(il), 2, 16, 8, 24, L.ptr(y), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL and bool((y == FILL).all())
