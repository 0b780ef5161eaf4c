"""GPU: ragged batches through the vocoder and the s2 decoder.  Requirement under test: every row of a batch is what the
one-row call gives for that row alone.

  * evt_resunit_fwd_multi_lens / evt_resunit_wide_fwd_lens (csrc/resunit.hip, resunit_wide.hip): row s on [0, Ls) is bit for
    bit the existing one-row launch with L = Ls, [Ls, L) is stored as zero, whatever the dead tail of x holds (1e4 here).
    The one-row fused launches refuse L < 64, so the row of 7 positions is compared with the unfused three launches
    under the bound tests/test_resunit_gpu.py puts on fused vs unfused (1e-2 of max-abs).
  * evt_mask_tail against torch.masked_fill, exact, three dtypes.
  * Generator.forward(x, g, lens) row by row against forward on the row alone.
  * SynthesizerTrn.decode_batch against decode per row, and against the reference's own outputs for the fixture row
    (tests/golden/s2_decode.pt, bounds of tests/test_s2_model_gpu.py::test_decode_and_extract_latent)."""
import ctypes as C
import json
import os

import pytest
import torch

from util_fill import decode_inputs, fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIG = 1e4          # the dead tails of x: a missed mask shows


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _pairs(gpu, half, C_, specs):
    """[(conv1, conv2)] for (k, dil) in specs, weights folded into a bank of the 16-bit type `half`"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.module.models import get_padding

    mods = []
    for k, d in specs:
        mods += [HC.EvtConv1d(C_, C_, k, dilation=d, padding=get_padding(k, d), weight_norm=True),
                 HC.EvtConv1d(C_, C_, k, dilation=1, padding=get_padding(k, 1), weight_norm=True)]
    m = torch.nn.ModuleList(mods).to(gpu)
    with torch.no_grad():
        for c in m:
            c.weight_g.mul_(torch.rand_like(c.weight_g) + 0.5)
            c.bias.normal_(0, 0.2)
    bank = HC.WeightBank(m, half, gpu)
    bank.build_tables()
    bank.fold()
    return [(m[2 * i], m[2 * i + 1]) for i in range(len(specs))], bank


def _ragged_x(gpu, half, nseq, Lq, C_, live):
    x = torch.randn(nseq, Lq, C_, device=gpu).to(half)
    for s, n in enumerate(live):
        x[s, n:] = BIG
    return x


def _unfused(pair, x, slope):
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    s1, s2 = pair[0]._slot, pair[1]._slot
    xa = HC._lrelu(x, slope)
    mid = HC._fwd(s1, xa, None, 1.0, L.ACT_LRELU, slope)
    return xa, mid, HC._fwd(s2, mid, x, 1.0, L.ACT_NONE, 1.0)


# ------------------------------------------------------------------------------------------------ narrow kernels
def _narrow_multi(pairs, xs, dil, slope, lens=None, mul=1, with_acts=True):
    """one grouped launch over the three kernel sizes; xs: one input per job.  -> [(xa, mid_a, y)] per job"""
    from easevoice_trainer_amd.hip import lib as L

    lib = L.lib()
    jobs = (L.ResUnitFwdJob * len(pairs))()
    outs = []
    for i, ((c1, c2), x) in enumerate(zip(pairs, xs)):
        nseq, Lq, C_ = x.shape
        xa, mid, y = (torch.full_like(x, 77.0) for _ in range(3))
        jb = jobs[i]
        jb.p = L.ResUnitParams(L.dt_code(x.dtype), nseq, Lq, C_, c1.k, dil, slope)
        jb.x, jb.w1_reg, jb.w2_reg = x.data_ptr(), c1._slot.reg.data_ptr(), c2._slot.reg.data_ptr()
        jb.b1, jb.b2 = c1.bias.data.data_ptr(), c2.bias.data.data_ptr()
        jb.xa, jb.mid_a = (xa.data_ptr(), mid.data_ptr()) if with_acts else (None, None)
        jb.y = y.data_ptr()
        outs.append((xa, mid, y))
    if lens is None:
        L.check(lib.evt_resunit_fwd_multi(jobs, len(pairs), L.stream_ptr()), "evt_resunit_fwd_multi")
    else:
        L.check(lib.evt_resunit_fwd_multi_lens(jobs, len(pairs), L.ptr(lens), int(mul), L.stream_ptr()),
                "evt_resunit_fwd_multi_lens")
    torch.cuda.synchronize()
    return outs


NARROW_L = 200                                    # three 64-position units and a remainder
NARROW_LIVE = [200, 64, 65, 7]                    # full, exactly one unit, one past a unit's edge, below the largest halo (25)


def _check_narrow(gpu, half, C_, dil, lens_list, mul, with_acts):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.module.models import LRELU_SLOPE

    L.set_half(half)
    torch.manual_seed(C_ * 100 + dil)
    pairs, _bank = _pairs(gpu, half, C_, [(3, dil), (7, dil), (11, dil)])
    live = [min(NARROW_L, n * mul) for n in lens_list]
    xs = [_ragged_x(gpu, half, len(live), NARROW_L, C_, live) for _ in pairs]
    lens = torch.tensor(lens_list, dtype=torch.int32, device=gpu)
    got = _narrow_multi(pairs, xs, dil, LRELU_SLOPE, lens, mul, with_acts)
    for s, n in enumerate(live):
        for j, (_xa, _mid, y) in enumerate(got):
            assert int((y[s, n:] != 0).sum()) == 0, ("tail of y must be stored as zero", s, j)
        rows = [x[s:s + 1, :n].contiguous() for x in xs]
        if n >= 64:
            want = _narrow_multi(pairs, rows, dil, LRELU_SLOPE)
            for j, ((xa, mid, y), (xa1, mid1, y1)) in enumerate(zip(got, want)):
                assert torch.equal(y[s, :n], y1[0]), ("y", s, j)
                if with_acts:
                    assert torch.equal(xa[s, :n], xa1[0]) and torch.equal(mid[s, :n], mid1[0]), ("xa / mid_a", s, j)
        else:
            for j, (pair, row) in enumerate(zip(pairs, rows)):
                xa1, mid1, y1 = _unfused(pair, row, LRELU_SLOPE)
                xa, mid, y = got[j]
                assert rel(y[s, :n], y1[0]) < 1e-2, (rel(y[s, :n], y1[0]), s, j)
                if with_acts:
                    assert torch.equal(xa[s, :n], xa1[0]) and rel(mid[s, :n], mid1[0]) < 1e-2, (s, j)
    if not with_acts:
        for xa, mid, _y in got:          # NULL pointers: nothing else was written
            assert bool((xa == 77.0).all()) and bool((mid == 77.0).all())


@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C_", [16, 32])
@pytest.mark.parametrize("dil", [1, 3, 5])
def test_narrow_ragged_rows_equal_one_row_launches(gpu, half, C_, dil):
    """k = 3 / 7 / 11 in one launch, xa / mid_a given"""
    _check_narrow(gpu, half, C_, dil, NARROW_LIVE, 1, True)


@pytest.mark.parametrize("C_", [16, 32])
def test_narrow_ragged_without_saved_activations(gpu, C_):
    """xa = mid_a = NULL (inference)"""
    _check_narrow(gpu, torch.bfloat16, C_, 3, NARROW_LIVE, 1, False)


def test_narrow_ragged_lens_in_frames(gpu):
    """mul = 8: lens in frames; 30 frames = 240 positions are clamped to L = 200"""
    _check_narrow(gpu, torch.bfloat16, 32, 5, [30, 8, 9, 1], 8, True)


# -------------------------------------------------------------------------------------------------- wide kernels
WIDE_P = 160                                       # positions per tile of evt_resunit_wide_fwd
WIDE_L = 3 * WIDE_P + 40
WIDE_LIVE = [WIDE_L, WIDE_P, WIDE_P + 1, 64, 7]


def _wide(pair, x, dil, slope, lens=None, mul=1, with_acts=True):
    from easevoice_trainer_amd.hip import lib as L

    c1, c2 = pair
    nseq, Lq, C_ = x.shape
    xa, mid, y = (torch.full_like(x, 77.0) for _ in range(3))
    p = L.ResUnitParams(L.dt_code(x.dtype), nseq, Lq, C_, c1.k, dil, slope)
    args = (C.byref(p), L.ptr(x), L.ptr(c1._slot.reg), L.ptr(c2._slot.reg), L.ptr(c1.bias.data), L.ptr(c2.bias.data),
            L.ptr(xa if with_acts else None), L.ptr(mid if with_acts else None), L.ptr(y))
    if lens is None:
        L.check(L.lib().evt_resunit_wide_fwd(*args, L.stream_ptr()), "evt_resunit_wide_fwd")
    else:
        L.check(L.lib().evt_resunit_wide_fwd_lens(*args, L.ptr(lens), int(mul), L.stream_ptr()), "evt_resunit_wide_fwd_lens")
    torch.cuda.synchronize()
    return xa, mid, y


def _check_wide(gpu, C_, k, dil, lens_list, mul, with_acts):
    from easevoice_trainer_amd.module.models import LRELU_SLOPE

    half = torch.bfloat16
    torch.manual_seed(C_ * 100 + k * 10 + dil)
    (pair,), _bank = _pairs(gpu, half, C_, [(k, dil)])
    live = [min(WIDE_L, n * mul) for n in lens_list]
    x = _ragged_x(gpu, half, len(live), WIDE_L, C_, live)
    lens = torch.tensor(lens_list, dtype=torch.int32, device=gpu)
    xa, mid, y = _wide(pair, x, dil, LRELU_SLOPE, lens, mul, with_acts)
    for s, n in enumerate(live):
        assert int((y[s, n:] != 0).sum()) == 0, ("tail of y must be stored as zero", s)
        row = x[s:s + 1, :n].contiguous()
        if n >= 64:
            xa1, mid1, y1 = _wide(pair, row, dil, LRELU_SLOPE)
            assert torch.equal(y[s, :n], y1[0]), ("y", s)
            if with_acts:
                assert torch.equal(xa[s, :n], xa1[0]) and torch.equal(mid[s, :n], mid1[0]), ("xa / mid_a", s)
        else:
            xa1, mid1, y1 = _unfused(pair, row, LRELU_SLOPE)
            assert rel(y[s, :n], y1[0]) < 1e-2, (rel(y[s, :n], y1[0]), s)
            if with_acts:
                assert torch.equal(xa[s, :n], xa1[0]) and rel(mid[s, :n], mid1[0]) < 1e-2, s
    if not with_acts:
        assert bool((xa == 77.0).all()) and bool((mid == 77.0).all())


@pytest.mark.parametrize("C_", [64, 128])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("dil", [1, 5])
def test_wide_ragged_rows_equal_one_row_launches(gpu, C_, k, dil):
    _check_wide(gpu, C_, k, dil, WIDE_LIVE, 1, True)


@pytest.mark.parametrize("C_", [64, 128])
def test_wide_ragged_without_saved_activations(gpu, C_):
    _check_wide(gpu, C_, 7, 5, WIDE_LIVE, 1, False)


def test_wide_ragged_lens_in_frames(gpu):
    """mul = 80: 7 frames = 560 positions are clamped to L = 520; 2 frames = one tile, 1 frame = 80 positions"""
    _check_wide(gpu, 128, 11, 5, [7, 2, 1, 3], 80, True)


# ----------------------------------------------------------------------------------------------------- mask_tail
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_mask_tail_exact(gpu, dtype):
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    torch.manual_seed(5)
    nseq, Lq, C_ = 4, 37, 24                       # C a multiple of 8, an odd L
    for lens_list, mul in (([37, 5, 0, 36], 1), ([10, 2, 0, 9], 4)):
        x = torch.randn(nseq, Lq, C_, device=gpu).to(dtype)
        lens = torch.tensor(lens_list, dtype=torch.int32, device=gpu)
        dead = torch.arange(Lq, device=gpu).view(1, -1) >= (lens.view(-1, 1) * mul)
        want = x.masked_fill(dead.unsqueeze(-1), 0)
        got = HC.mask_tail(x.clone(), lens, mul)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (lens_list, mul)
        assert int(dead.sum()) > 0 and int((~dead).sum()) > 0


# ----------------------------------------------------------------------------------------------------- Generator
FRAMES = [12, 5, 1]


def _generator(gpu, dtype):
    from easevoice_trainer_amd.module import models
    from easevoice_trainer_amd.runtime import ModelRuntime

    hm = json.load(open(os.path.join(ROOT, "configs", "s2.json")))["model"]
    gen = models.Generator(hm["inter_channels"], hm["resblock"], hm["resblock_kernel_sizes"], hm["resblock_dilation_sizes"],
                           hm["upsample_rates"], hm["upsample_initial_channel"], hm["upsample_kernel_sizes"],
                           gin_channels=hm["gin_channels"])
    fill_module(gen, 11)
    gen.eval()
    rt = ModelRuntime(gen, dtype=dtype, device=gpu)
    rt.prepare(force=True)
    return gen, rt


def _generator_rows(gpu, dtype):
    """(batched output [3, 12 * 640], [row-alone outputs])"""
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    gen, _rt = _generator(gpu, dtype)
    g_ = torch.Generator().manual_seed(21)
    x = torch.randn(len(FRAMES), max(FRAMES), 192, generator=g_).to(gpu)
    ge = (0.3 * torch.randn(len(FRAMES), 512, generator=g_)).to(gpu)
    for b, n in enumerate(FRAMES):
        x[b, n:] = BIG                                # whatever the memory holds behind a row's end
    lens = torch.tensor(FRAMES, dtype=torch.int32, device=gpu)
    amp = dtype != torch.float32
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype if amp else torch.bfloat16, enabled=amp):
        xin = x.clone()
        o = gen(xin, g=ge, lens=lens)
        assert torch.equal(xin, x), "the caller's tensor is not written"
        alone = [gen(x[b:b + 1, :n].contiguous(), g=ge[b:b + 1]) for b, n in enumerate(FRAMES)]
    torch.cuda.synchronize()
    assert o.shape == (len(FRAMES), max(FRAMES) * 640, 1)
    return o[..., 0], [a[0, :, 0] for a in alone]


def test_generator_ragged_bf16_bit_identical(gpu, monkeypatch):
    """The two fused families and a single convolution of a zero-tailed input are per-row arithmetic, so a batched row is
    bit for bit the row alone -- as long as both runs take the same kernels.  One dispatch decision looks at the size of
    the whole problem: the transposed up-samplers ups.1 .. ups.4 run on the LDS-DMA GEMM kernels with a pre-activated
    input when nseq * L is large enough (evt_conv1d_wants_plain_x) and on the generic kernel with the leaky-relu fused on
    load otherwise, two summation orders (measured: up to 1.1e-2 of max-abs per up-sampler between the batch of 12 + 5 + 1
    frames and the row of 5 frames alone).  So: bit-identical with that decision held fixed (hip.conv.PLAIN_X off, the
    switch of EVT_CONV_PLAIN_X), and under the default dispatch within what tests/test_conv_gpu.py allows a bf16
    convolution, 3e-2 of max-abs."""
    from easevoice_trainer_amd.hip import conv as HC

    o, alone = _generator_rows(gpu, torch.bfloat16)
    for b, n in enumerate(FRAMES):
        assert alone[b].numel() == n * 640
        # conv_post (k = 7, no bias) answers the row's last samples on the three positions behind its end; zeros from there on
        assert int((o[b, n * 640 + 3:] != 0).sum()) == 0, b
        print("default dispatch: row", b, "rel", rel(o[b, :n * 640], alone[b]))
        assert rel(o[b, :n * 640], alone[b]) < 3e-2, (b, rel(o[b, :n * 640], alone[b]))
    monkeypatch.setattr(HC, "PLAIN_X", False)
    o, alone = _generator_rows(gpu, torch.bfloat16)
    for b, n in enumerate(FRAMES):
        assert int((o[b, n * 640 + 3:] != 0).sum()) == 0, b
        print("one up-sampler kernel: row", b, "rel", rel(o[b, :n * 640], alone[b]))
        assert torch.equal(o[b, :n * 640], alone[b]), (b, rel(o[b, :n * 640], alone[b]))


def test_generator_ragged_fp32(gpu):
    o, alone = _generator_rows(gpu, torch.float32)
    for b, n in enumerate(FRAMES):
        # conv_post (k = 7, no bias) answers the row's last samples on the three positions behind its end; zeros from there on
        assert int((o[b, n * 640 + 3:] != 0).sum()) == 0, b
        assert rel(o[b, :n * 640], alone[b]) < 1e-5, (b, rel(o[b, :n * 640], alone[b]))


# -------------------------------------------------------------------------------------------------- decode_batch
def _export():
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    net = models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)                                   # the weights of tests/golden/s2_decode.pt
    weight = {k: v.detach().clone() for k, v in net.state_dict().items() if "enc_q" not in k}
    return weight, hps


def _batch(d):
    """short row (the fixture's first 11 codes, 9 phonemes), the fixture, long row (its codes and phonemes twice over)"""
    codes, text = d["codes"][0, 0], d["text"][0]
    rows_c = [codes[:11], codes, torch.cat([codes, codes])]
    rows_t = [text[:9], text, torch.cat([text, text])]
    pc = torch.nn.utils.rnn.pad_sequence(rows_c, batch_first=True).unsqueeze(0)
    pt = torch.nn.utils.rnn.pad_sequence(rows_t, batch_first=True)
    noise = torch.randn(3, 192, 2 * pc.size(2) + 8, generator=torch.Generator().manual_seed(99))
    noise[1, :, :d["noise"].size(2)] = d["noise"][0]
    return rows_c, rows_t, pc, pt, noise


@pytest.fixture(scope="module")
def decoded(gpu):
    """fp32: per gold case with speed 1 -> (batch outputs, row-alone outputs); computed once"""
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice

    weight, hps = _export()
    dg = torch.load(os.path.join(HERE, "golden", "s2_decode.pt"), weights_only=False)
    d = decode_inputs()
    voice = SoVITSVoice({"weight": weight, "config": hps, "info": "fixture"}, device=str(gpu), dtype=torch.float32)
    rows_c, rows_t, pc, pt, noise = _batch(d)
    out = []
    for c in dg["cases"]:
        if c["speed"] != 1:
            continue
        if c["n_refer"] == 2:
            refer = [d["refers"][1], d["refers"], [d["refers"][0]]]        # one entry per row; the fixture row averages two
        else:
            refer = d["refers"][0]                                           # shared
        per_row = refer if c["n_refer"] == 2 else [refer] * 3
        got = voice.decode_batch(pc, [t.numel() for t in rows_c], pt, [t.numel() for t in rows_t], refer,
                                 noise_scale=0.5, noise=noise)
        alone = [voice.decode(rows_c[b].view(1, 1, -1), rows_t[b].view(1, -1), per_row[b], noise_scale=0.5,
                              noise=noise[b:b + 1])[0, 0] for b in range(3)]
        torch.cuda.synchronize()
        out.append((c, [g.cpu() for g in got], [a.cpu() for a in alone]))
    assert len(out) == 2
    return out, (weight, hps, dg, d)


def test_decode_batch_fixture_row_meets_reference(decoded):
    for c, got, _alone in decoded[0]:
        o = got[1]
        assert o.dim() == 1 and o.numel() == c["shape"][-1]
        assert rel(o[:4096], c["o_head"]) < 1e-3 and rel(o[::37], c["o_dec"]) < 1e-3, c["n_refer"]
        assert abs(float(o.double().pow(2).sum()) - c["sq_sum"]) < 2e-3 * c["sq_sum"]


def test_decode_batch_rows_equal_decode_alone(decoded):
    """whole row and -- where a missing mask in the vocoder shows -- its last 4096 samples on their own"""
    for c, got, alone in decoded[0]:
        for b, (o, a) in enumerate(zip(got, alone)):
            assert o.shape == a.shape and o.numel() == [11, 30, 60][b] * 2 * 640
            assert rel(o, a) < 1e-3, (c["n_refer"], b, rel(o, a))
            assert rel(o[-4096:], a[-4096:]) < 1e-3, (c["n_refer"], b, rel(o[-4096:], a[-4096:]))


def test_decode_batch_bf16(gpu, decoded):
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice

    weight, hps, dg, d = decoded[1]
    voice = SoVITSVoice({"weight": {k: v.half() for k, v in weight.items()}, "config": hps, "info": "fixture"},
                        device=str(gpu), dtype=torch.bfloat16)
    rows_c, rows_t, pc, pt, noise = _batch(d)
    c = dg["cases"][0]
    assert c["speed"] == 1 and c["n_refer"] == 1
    got = voice.decode_batch(pc, [t.numel() for t in rows_c], pt, [t.numel() for t in rows_t], d["refers"][0],
                             noise_scale=0.5, noise=noise)
    assert rel(got[1][::37], c["o_dec"]) < 5e-2, rel(got[1][::37], c["o_dec"])
    # a batch of one: decode's output size
    one = voice.decode_batch(d["codes"], [d["codes"].size(2)], d["text"], [d["text"].size(1)], d["refers"][0],
                             noise_scale=0.5, noise=d["noise"])
    o = voice.decode(d["codes"], d["text"], d["refers"][0], noise_scale=0.5, noise=d["noise"])
    assert len(one) == 1 and one[0].shape == o[0, 0].shape and list(o.shape) == c["shape"]
    assert rel(one[0][::37], c["o_dec"]) < 5e-2
    # without injected noise: random prior draw, finite output of the same sizes
    free = voice.decode_batch(pc, [t.numel() for t in rows_c], pt, [t.numel() for t in rows_t], d["refers"][0])
    assert [f.numel() for f in free] == [g.numel() for g in got] and all(bool(torch.isfinite(f).all()) for f in free)
