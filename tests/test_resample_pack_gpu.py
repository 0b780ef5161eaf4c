"""GPU: evt_resample_pack_rows (csrc/resample_poly.hip) -- the finishing launch of a ragged decode: every row resampled from
32 kHz to the requested rate, converted to fp32 or int16 and packed, with a gap of zeros behind each row, into one buffer.

One batch of rows with n = 1, 2, 37, 641 and 3 * tile + 5 live samples (tile = the kernel's 2048 outputs per block) in one
x that holds 1e4 behind every row's end; the packed buffer holds 77 before the launch.  Seven rates, three storage types
(fp32 through both builds).  The float64 oracle (tests/resample_oracle.py) is computed once per (rate, storage type)."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_oracle as O

pytestmark = pytest.mark.gpu
BIG, FILL, EINVAL = 1e4, 77, 22
TILE = 2048
NS = [1, 2, 37, 641, 3 * TILE + 5]
LEN = NS[-1] + 11
ORDER = [3, 0, 4, 1, 2]
CASES = [(torch.float32, torch.bfloat16), (torch.float32, torch.float16), (torch.bfloat16, torch.bfloat16),
         (torch.float16, torch.float16)]
IDS = ["f32", "f32-f16build", "bf16", "f16"]
F32, S16 = 0, 1
_ORACLE = {}


def _x_host(dtype):
    g = torch.Generator().manual_seed(4242)
    x = (torch.rand(len(NS), LEN, generator=g) * 1.9 - 0.95).to(dtype)         # inside (-1, 1)
    for s, n in enumerate(NS):
        x[s, n:] = BIG
    return x


def _oracle(rate, dtype):
    """per row (want, A, Jm) in float64 from the stored values of x"""
    key = (rate, dtype)
    if key not in _ORACLE:
        up, down = O.ratio(rate)
        x = _x_host(dtype).double().numpy()
        _ORACLE[key] = [O.resample(x[s, :n], up, down) for s, n in enumerate(NS)]
    return _ORACLE[key]


def _launch(x, lens, rate, fmt, order=None, gap=0, mul=1, over=None):
    """the C entry point on a buffer pre-filled with 77 -> (return code, buffer, offsets, lengths); over: arguments to replace"""
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.hip import lib as L

    up, down = O.ratio(rate)
    nseq, length = x.shape
    lengths = [(min(n * mul, length) * up) // down for n in lens]
    offsets, total = [0] * nseq, 0
    for b in (order or range(nseq)):
        offsets[b] = total
        total += lengths[b] + gap
    out = torch.full((max(total, 1),), FILL, dtype=torch.float32 if fmt == F32 else torch.int16, device=x.device)
    ld = torch.tensor(lens, dtype=torch.int32, device=x.device)
    od = torch.tensor(offsets, dtype=torch.int64, device=x.device)
    table, j_pad = (None, 0) if up == down else (audio.phase_table(up, down, x.device), audio.table_shape(up, down)[1])
    a = dict(dtype=L.dt_of(x), x=L.ptr(x), lens=L.ptr(ld), mul=mul, nseq=nseq, L=length, up=up, down=down, table=L.ptr(table),
             J=j_pad, fmt=fmt, out=L.ptr(out), out_elems=C.c_int64(max(total, 1)), off=L.ptr(od), gap=gap)
    a.update(over or {})
    rc = L.lib().evt_resample_pack_rows(a["dtype"], a["x"], a["lens"], a["mul"], a["nseq"], a["L"], a["up"], a["down"], a["table"],
                                        a["J"], a["fmt"], a["out"], a["out_elems"], a["off"], a["gap"], L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, offsets, lengths


@pytest.mark.parametrize("rate", O.RATES)
@pytest.mark.parametrize("dtype,half", CASES, ids=IDS)
def test_rows_formats_packing_and_row_alone(gpu, dtype, half, rate):
    """1. fp32 output against the float64 oracle at every sample: |got - want| <= 2^-24 (Jm + 3) A[m], A[m] = sum_i |x[i]|
    |g[m down - i up]|, Jm the live taps of m -- one rounding of each coefficient (the table is fp32), one of each product,
    Jm - 1 additions of partial sums <= A[m]; + 3 covers the second-order terms at Jm <= 513.  Derived, not measured: fused
    multiply-adds and the kernel's four accumulators stay inside it.  At 32000 got == x exactly.
    2. int16 output == the conversion rule applied on the host to the fp32 output, every element; at 32000 also
    (x * 32768).astype(int16).
    3. packing: permuted order, gap 0 and 5, no 77 left, every gap zero.
    4. every row launched alone (nseq = 1) gives the bytes it has in the batch, fp32 and int16."""
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(half)
    xh = _x_host(dtype)
    x = xh.to(gpu)
    up, down = O.ratio(rate)
    oracle = _oracle(rate, dtype)
    rows = {}
    for fmt in (F32, S16):
        for gap in (0, 5):
            rc, out, offsets, lengths = _launch(x, NS, rate, fmt, ORDER, gap)
            assert rc == 0
            oc = out.cpu()
            assert lengths == [(n * up) // down for n in NS]
            assert oc.numel() == sum(lengths) + gap * len(NS)
            place = 0
            for b in ORDER:                                    # the rows lie in the sequence ORDER, back to back
                assert offsets[b] == place
                place += lengths[b] + gap
            live = torch.zeros(oc.numel(), dtype=torch.bool)
            for b in range(len(NS)):
                live[offsets[b]:offsets[b] + lengths[b]] = True
                assert int((oc[offsets[b] + lengths[b]:offsets[b] + lengths[b] + gap] != 0).sum()) == 0, ("gap", b)
            assert int((~live).sum()) == gap * len(NS) and int((oc[~live] != 0).sum()) == 0
            got = [oc[offsets[b]:offsets[b] + lengths[b]] for b in range(len(NS))]
            if fmt == F32:
                assert int((oc == FILL).sum()) == 0, "every element of the buffer is written"
            else:
                # an int16 sample may BE 77: every element written shows as equality with the converted fp32 rows below
                assert all(torch.equal(g, torch.from_numpy(O.to_int16(r.numpy()))) for g, r in zip(got, rows[F32]))
            if gap == 0:
                rows[fmt] = got
            else:
                assert all(torch.equal(a, b) for a, b in zip(got, rows[fmt])), "the gap moves the rows, not their values"
    for s, n in enumerate(NS):
        got = rows[F32][s].double().numpy()
        if rate == O.IN_RATE:
            assert torch.equal(rows[F32][s], xh[s, :n].float()), s
            assert np.array_equal(rows[S16][s].numpy(), (xh[s, :n].float().numpy() * 32768).astype(np.int16)), s
            continue
        want, a, jm = oracle[s]
        assert got.shape == want.shape
        if not len(want):
            continue
        err, bound = np.abs(got - want), 2.0 ** -24 * (jm + 3) * a
        worst = int(np.argmax(err - bound))
        print(f"{dtype} {rate} Hz row {s} (n = {n}): max err {err.max():.3e}, at the tightest place err {err[worst]:.3e} "
              f"bound {bound[worst]:.3e}")
        assert (err <= bound).all(), (rate, s, float(err[worst]), float(bound[worst]))
        assert np.abs(got).max() < 4.0, "a tap on the 1e4 behind the row's end would show"
    for s, n in enumerate(NS):                                  # 4. the row alone
        for fmt in (F32, S16):
            rc, out, _o, lengths = _launch(x[s:s + 1].contiguous(), [n], rate, fmt)
            assert rc == 0 and lengths == [(n * up) // down]
            assert torch.equal(out.cpu()[:lengths[0]], rows[fmt][s]), (s, fmt)


@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16], ids=["bf16build", "f16build"])
def test_int16_saturates_and_nan_is_zero(gpu, half):
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(half)
    vals = [1.0, -1.0, 1.5, float("nan"), -1.5, 0.99999, -0.99999, 1.0 / 32768, -1.0 / 32768, 0.5 / 32768, float("inf")]
    want = [32767, -32768, 32767, 0, -32768, 32767, -32767, 1, -1, 0, 32767]
    for dtype in (torch.float32, half):
        x = torch.tensor([vals], dtype=torch.float32).to(dtype).to(gpu)
        rc, out, _o, _l = _launch(x, [len(vals)], 32000, S16)
        assert rc == 0
        ref = O.to_int16(x.float().cpu().numpy()[0])
        assert np.array_equal(out.cpu().numpy(), ref), dtype
        if dtype == torch.float32:
            assert out.cpu().tolist() == want
        assert out.cpu().tolist()[:4] == [32767, -32768, 32767, 0]


def test_lens_mul_and_clamp(gpu):
    """n_s = min(lens[s] * mul, L), as evt_mask_tail reads its lengths: frames times samples per frame, clamped to the row"""
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(torch.bfloat16)
    x = _x_host(torch.float32)[:, :640 * 3].contiguous().to(gpu)
    for rate in (48000, 32000):
        rc, a, off_a, len_a = _launch(x, [1, 2, 3, 3, 0], rate, F32, mul=640)
        rc2, b, off_b, len_b = _launch(x, [640, 1280, 1920, 5000, 0], rate, F32)
        assert rc == 0 and rc2 == 0 and len_a == len_b and len_a[4] == 0 and torch.equal(a, b)


def test_a_ratio_outside_lds_takes_the_direct_form(gpu):
    """32000 -> 500 Hz (1/64): 8193 taps per output, a tile's input span does not fit in LDS and the kernel reads x from
    global memory -- same definition, same bound, same row-alone identity"""
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(torch.bfloat16)
    xh = _x_host(torch.float32)
    x = xh.to(gpu)
    rc, out, offsets, lengths = _launch(x, NS, 500, F32, ORDER, 3)
    assert rc == 0 and lengths == [n // 64 for n in NS] and lengths[4] == 96
    oc = out.cpu()
    for s, n in enumerate(NS):
        want, a, jm = O.resample(xh[s, :n].double().numpy(), 1, 64)
        got = oc[offsets[s]:offsets[s] + lengths[s]]
        assert (np.abs(got.double().numpy() - want) <= 2.0 ** -24 * (jm + 3) * a).all(), s
        assert int((oc[offsets[s] + lengths[s]:offsets[s] + lengths[s] + 3] != 0).sum()) == 0
        rc, alone, _o, _l = _launch(x[s:s + 1].contiguous(), [n], 500, F32)
        assert rc == 0 and torch.equal(alone.cpu()[:lengths[s]], got), s


def test_argument_errors_launch_nothing(gpu):
    from easevoice_trainer_amd.hip import lib as L

    null = C.c_void_p(0)
    for half in (torch.bfloat16, torch.float16):
        L.set_half(half)
        x = _x_host(half)[:, :700].contiguous().to(gpu)
        lens = [1, 2, 37, 641, 700]
        rc, out, _o, _l = _launch(x, lens, 48000, S16)
        assert rc == 0 and not bool((out == FILL).all())
        other = 2 if half == torch.bfloat16 else 1
        bad = [dict(x=null), dict(lens=null), dict(out=null), dict(off=null), dict(table=null), dict(nseq=0), dict(L=0),
               dict(mul=0), dict(up=0), dict(down=-2), dict(gap=-1), dict(out_elems=C.c_int64(0)), dict(J=128), dict(J=131), dict(J=136),
               dict(fmt=2), dict(dtype=other), dict(dtype=7),
               dict(x=C.c_void_p(x.data_ptr() + 1)), dict(table=C.c_void_p(_table_ptr(gpu) + 4))]
        for over in bad:
            rc, out, _o, _l = _launch(x, lens, 48000, S16, over=over)
            assert rc == EINVAL, over
            assert bool((out == FILL).all()), ("nothing was launched", over)
        rc, out, _o, _l = _launch(x, lens, 48000, F32, over=dict(out=null))
        assert rc == EINVAL
        # up == down == 1 needs no table
        rc, out, _o, _l = _launch(x, lens, 32000, S16, over=dict(table=null, J=0))
        assert rc == 0


def _table_ptr(gpu):
    from easevoice_trainer_amd.hip import audio

    return audio.phase_table(3, 2, gpu).data_ptr()


def test_binding_orders_gaps_and_refuses(gpu):
    """hip.audio.resample_pack: the launch above behind a host prefix sum -- PackedAudio.row(b) in a permuted order with the
    reference's gap int(rate * interval), equal to the raw launch; rates it does not serve are EvtErrors"""
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(torch.bfloat16)
    x = _x_host(torch.bfloat16).to(gpu)
    pa = audio.resample_pack(x.unsqueeze(-1), NS, 1, 32000, 44100, "int16", order=ORDER, interval=0.001)
    torch.cuda.synchronize()
    rc, out, offsets, lengths = _launch(x, NS, 44100, S16, ORDER, 44)
    assert rc == 0 and pa.gap == 44 and pa.rate == 44100 and pa.offsets == offsets and pa.lengths == lengths
    assert pa.data.dtype == torch.int16 and torch.equal(pa.data, out)
    for b in range(len(NS)):
        assert torch.equal(pa.row(b), out[offsets[b]:offsets[b] + lengths[b]])
        assert pa.row(b, gap=True).numel() == lengths[b] + 44
    one = audio.resample_pack(x[3, :641], [641], 1, 32000, 44100, "int16")
    assert torch.equal(one.row(0), pa.row(3))
    assert audio.phase_table(441, 320, gpu) is audio.phase_table(441, 320, gpu)
    for bad in (dict(out_rate=11025), dict(out_format="int8"), dict(order=[0, 0, 1, 2, 3]), dict(interval=-1.0)):
        kw = dict(dict(out_rate=48000, out_format="int16"), **bad)
        with pytest.raises(L.EvtError):
            audio.resample_pack(x, NS, 1, 32000, kw.pop("out_rate"), kw.pop("out_format"), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# behind the vocoder

@pytest.fixture(scope="module")
def decoded(gpu):
    """the three ragged rows of tests/test_decode_batch_speed_gpu.py (its export fixture, fp32): decode_batch without the
    keywords, with out_rate = 48000 / out_format = "int16", every fragment alone with them, and at mixed speeds"""
    from test_decode_batch_speed_gpu import MIXED, _batch, _export, _frames
    from util_fill import decode_inputs

    from easevoice_trainer_amd.inference.sovits import SoVITSVoice

    weight, hps = _export()
    d = decode_inputs()
    voice = SoVITSVoice({"weight": weight, "config": hps, "info": "fixture"}, device=str(gpu), dtype=torch.float32)
    rows_c, rows_t, pc, pt, noise = _batch(d)
    args = (pc, [t.numel() for t in rows_c], pt, [t.numel() for t in rows_t], d["refers"][0])
    kw = dict(noise_scale=0.5, noise=noise)
    out = dict(plain=voice.decode_batch(*args, **kw),
               packed=voice.decode_batch(*args, out_rate=48000, out_format="int16", interval=0.3, **kw),
               default=voice.decode_batch(*args, out_format="float32", **kw),
               mixed=voice.decode_batch(*args, speed=MIXED, out_rate=48000, out_format="int16", **kw),
               alone=[voice.decode_batch(rows_c[b].view(1, 1, -1), [rows_c[b].numel()], rows_t[b].view(1, -1),
                                         [rows_t[b].numel()], d["refers"][0], noise_scale=0.5, noise=noise[b:b + 1],
                                         out_rate=48000, out_format="int16") for b in range(3)])
    torch.cuda.synchronize()
    return out, _frames(MIXED), voice, args, kw


def test_decode_batch_packs_what_it_returns_without_the_keywords(decoded):
    from easevoice_trainer_amd.hip import audio

    out, _frames, voice, _args, _kw = decoded
    pa = out["packed"]
    assert isinstance(pa, audio.PackedAudio) and pa.rate == 48000 and pa.gap == int(48000 * 0.3) and len(pa) == 3
    assert pa.data.dtype == torch.int16 and pa.data.is_cuda and pa.data.numel() == sum(pa.lengths) + 3 * pa.gap
    assert pa.offsets == [0, pa.lengths[0] + pa.gap, pa.lengths[0] + pa.lengths[1] + 2 * pa.gap]       # batch order
    for b, w in enumerate(out["plain"]):
        assert pa.lengths[b] == (w.numel() * 3) // 2
        one = audio.resample_pack(w, [w.numel()], 1, 32000, 48000, "int16")
        assert torch.equal(pa.row(b), one.row(0)), b
        assert int((pa.row(b, gap=True)[pa.lengths[b]:] != 0).sum()) == 0
        assert int(pa.row(b).abs().max()) > 0
        # out_rate None with a format given: the model's rate, the values unchanged
        assert out["default"].rate == voice.sampling_rate == 32000 and torch.equal(out["default"].row(b), w.float()), b


def test_decode_batch_row_equals_the_fragment_alone(decoded):
    out, *_ = decoded
    for b in range(3):
        alone = out["alone"][b]
        diff = (out["packed"].row(b).int() - alone.row(0).int()).abs().max()
        print("row", b, "batch vs alone, int16 max difference:", int(diff))
        assert len(alone) == 1 and torch.equal(out["packed"].row(b), alone.row(0)), b


def test_decode_batch_lengths_at_mixed_speeds(decoded):
    out, frames, *_ = decoded
    assert out["mixed"].lengths == [(n * 640 * 3) // 2 for n in frames]


def test_decode_batch_refuses_before_the_pass(decoded):
    from easevoice_trainer_amd.hip.lib import EvtError

    _out, _frames, voice, args, kw = decoded
    for bad in (dict(out_rate=11025), dict(out_format="int8"), dict(interval=0.3)):
        with pytest.raises(EvtError):
            voice.decode_batch(*args, **bad, **kw)
