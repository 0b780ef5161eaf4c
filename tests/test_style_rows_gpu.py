"""GPU: the style encoder on a ragged batch of references and precomputed voices in the s2 decoder.

  * evt_mish_rows_fwd / evt_glu_res_rows_fwd: bit for bit the existing p = 0 entry followed by evt_mask_tail.
  * evt_mean_rows: exact on small integers; on random inputs within (n_s + 1) 2^-24 mean_t |x| per channel -- the first-order
    bound of an fp32 sum of n_s terms in ANY order ((n_s - 1) u sum |x|, divided by n_s) plus the division's rounding --;
    a row of a batch bit for bit the row alone.
  * MelStyleEncoder.forward_rows, T = [5, 64, 65, 131] in Tmax = 136 with NaN behind every row's frames:
      - row b bit for bit forward_rows of the row alone (B = 1, Tmax = T_b);
      - fp32: within the project's standing fp32 parity bound 1e-3 max(1, max |ref|) of oracle.s2_step.mel_style_encoder in
        float64 on the row alone with an all-ones mask;
      - bf16: against the parent's forward on the same spectrogram, |d| <= 2^-7 |v| + (T + 1) 2^-24 mean_t |y| per element
        (y = the frames the mean is taken of): the bound for a parent that rounds its sum and its quotient to bf16 -- twice
        the two half-ulp roundings -- plus the summation bound above.  Under autocast the parent's sum runs in fp32 as well
        (torch lists sum among its fp32 operations), so only the second term is at work and the first is slack.  At these
        lengths the parent's dispatcher picks the generic implicit GEMM too; forward_rows pins it.
        MEASURED on an MI355X (largest |d| / bound per row, no bound changed after the first run): the end of this docstring.
  * decode_batch(style=cat(_style(r_b))) is torch.equal to decode_batch(refer=[r_b]) (code_lens = [3, 7]); the same for
    decode; the refusals raise.

MEASURED (bf16 forward_rows vs the parent, |d| / bound, max per row):  T=5: 0.000   T=64: 0.000   T=65: 0.000   T=131: 0.000
(the two agree to three decimals of the bound: same kernels in front of the mean, both means in fp32).  fp32 against the
float64 oracle: max |d| 2.4e-7 .. 7.4e-7 against bounds of 2.1e-3 .. 2.3e-3.  evt_mean_rows on random inputs: at most 0.014 of
its bound."""
import ctypes as C
import json
import os

import pytest
import torch

from util_fill import decode_inputs, fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16]
ids = lambda d: str(d).split(".")[-1]


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ------------------------------------------------------------------------------------------------ tail-zeroing forms
@pytest.mark.parametrize("dt,wide", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                     (torch.bfloat16, torch.float32)], ids=["f32", "bf16", "bf16-f32"])
def test_tail_zeroing_forms_equal_entry_then_mask_tail(gpu, dt, wide):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.conv import mask_tail
    from easevoice_trainer_amd.hip.enc import glu_dropout_res, glu_res_rows, mish_dropout, mish_rows

    L.set_half(torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    lens_h = [37, 5, 0]
    lens = torch.tensor(lens_h, dtype=torch.int32).to(gpu)
    x = (3 * torch.randn(3, 37, 128, generator=g)).to(dt).to(gpu)
    h = (3 * torch.randn(3, 37, 256, generator=g)).to(dt).to(gpu)
    res = torch.randn(3, 37, 128, generator=g).to(wide).to(gpu)
    x[0, 3, :4] = torch.tensor([25.0, -25.0, 0.0, 20.0]).to(dt)        # softplus' threshold and the far ends
    with torch.no_grad():
        want_m = mask_tail(mish_dropout(x, 0.0, 3, wide), lens)
        want_g = mask_tail(glu_dropout_res(h, res, 0.0, 4), lens)
        xp, hp, rp = x.clone(), h.clone(), res.clone()
        for b, n in enumerate(lens_h):                                   # whatever the memory holds behind a row's end
            xp[b, n:], hp[b, n:], rp[b, n:] = float("nan"), float("nan"), float("nan")
        got_m, got_g = mish_rows(xp, lens, wide), glu_res_rows(hp, rp, lens)
    assert got_m.dtype == want_m.dtype == wide and got_g.dtype == want_g.dtype == wide
    assert torch.equal(_bits(got_m), _bits(want_m)), int((_bits(got_m) != _bits(want_m)).sum())
    assert torch.equal(_bits(got_g), _bits(want_g)), int((_bits(got_g) != _bits(want_g)).sum())
    for b, n in enumerate(lens_h):
        assert bool((_bits(got_m[b, n:]) == 0).all()) and bool((_bits(got_g[b, n:]) == 0).all())


# ------------------------------------------------------------------------------------------------------ evt_mean_rows
MEAN_LENS, MEAN_L, MEAN_C = [1, 63, 64, 65, 130, 0], 130, 72


def _mean_inputs(kind, dt):
    g = torch.Generator().manual_seed(17)
    if kind == "int":
        x = torch.randint(-8, 9, (len(MEAN_LENS), MEAN_L, MEAN_C), generator=g).float()
    else:
        x = torch.randn(len(MEAN_LENS), MEAN_L, MEAN_C, generator=g)
    x = x.to(dt)
    for b, n in enumerate(MEAN_LENS):
        x[b, n:] = float("nan")
    return x


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["int", "randn"])
def test_mean_rows(gpu, kind, dt):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.enc import mean_rows

    L.set_half(torch.bfloat16)
    x = _mean_inputs(kind, dt)
    lens = torch.tensor(MEAN_LENS, dtype=torch.int32).to(gpu)
    got = mean_rows(x.to(gpu), lens).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(MEAN_LENS), MEAN_C)
    for b, n in enumerate(MEAN_LENS):
        if n == 0:
            assert bool((_bits(got[b]) == 0).all())
            continue
        x64 = x[b, :n].double()
        mean64 = x64.sum(0) / n
        if kind == "int":
            assert torch.equal(got[b], mean64.float()), b       # every partial sum is an exact integer, the division rounds once
        else:
            tol = (n + 1) * U * x64.abs().mean(0)
            frac = float(((got[b].double() - mean64).abs() / tol).max())
            print(f"MEASURED mean_rows {ids(dt)} n = {n}: error / bound = {frac:.3f}")
            assert frac <= 1.0, (b, frac)
        # the row alone, in a tensor that ends with the row and in a longer one
        for l1 in (n, n + 9):
            x1 = torch.full((1, l1, MEAN_C), float("nan"), dtype=dt)
            x1[0, :n] = x[b, :n]
            one = mean_rows(x1.to(gpu), lens[b:b + 1].contiguous()).cpu()
            assert torch.equal(_bits(one[0]), _bits(got[b])), (b, l1)


def test_mean_rows_refusals(gpu):
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(torch.bfloat16)
    x = torch.zeros(2, 4, 8, device=gpu)
    lens = torch.tensor([4, 4], dtype=torch.int32).to(gpu)
    out = torch.full((64,), -7.0, device=gpu)
    f, null = L.lib().evt_mean_rows, C.c_void_p(0)
    px, pl, po = L.ptr(x), L.ptr(lens), L.ptr(out)
    for a in [(0, null, pl, 2, 4, 8, po), (0, px, null, 2, 4, 8, po), (0, px, pl, 2, 4, 8, null), (0, px, pl, 0, 4, 8, po),
              (0, px, pl, 65536, 4, 8, po), (0, px, pl, 2, 0, 8, po), (0, px, pl, 2, 4, 0, po), (7, px, pl, 2, 4, 8, po)]:
        assert f(*a, L.stream_ptr()) == 22, a
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------------------ forward_rows
FR_T, FR_TMAX = [5, 64, 65, 131], 136


@pytest.fixture(scope="module", params=DTYPES, ids=ids)
def encoder(request, gpu):
    """(dtype, MelStyleEncoder behind an attached bank, x [4, 136, 704] with NaN behind the rows, lens, forward_rows(x))"""
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.module import models
    from easevoice_trainer_amd.runtime import ModelRuntime

    dtype = request.param
    L.set_half(torch.bfloat16)
    enc = models.MelStyleEncoder(704, style_vector_dim=512)
    fill_module(enc, 5)
    enc.eval()
    rt = ModelRuntime(enc, dtype=dtype, device=gpu)
    rt.prepare(force=True)
    x = torch.rand(len(FR_T), FR_TMAX, 704, generator=torch.Generator().manual_seed(8)) * 2.0
    for b, n in enumerate(FR_T):
        x[b, n:] = float("nan")
    lens = torch.tensor(FR_T, dtype=torch.int32).to(gpu)
    got = _rows(enc, dtype, x.to(gpu), lens)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(FR_T), 512) and bool(torch.isfinite(got).all())
    return dtype, enc, rt, x, lens, got


def _amp(dtype):
    amp = dtype != torch.float32
    return torch.autocast("cuda", dtype=dtype if amp else torch.bfloat16, enabled=amp)


def _rows(enc, dtype, x, lens):
    with torch.no_grad(), _amp(dtype):
        return enc.forward_rows(x, lens)


def test_forward_rows_row_equals_the_row_alone(gpu, encoder):
    """bit for bit in both dtypes: forward_rows pins a 16-bit bank to the generic implicit GEMM, so the convolution
    dispatcher cannot change kernel with the batch's shape (left to itself it hands the k = 5 convolutions and fc of the
    batch [4, 136] to conv_ring<2, 2, 4> of csrc/conv_deep.hip and those of a row alone to conv_igemm of csrc/conv1d.hip;
    measured then: max |batch - alone| = 8.2e-4 at T = 64 in bf16, 16 times the bound of the comparison with the parent)"""
    dtype, enc, _rt, x, lens, got = encoder
    for b, n in enumerate(FR_T):
        one = _rows(enc, dtype, x[b:b + 1, :n].contiguous().to(gpu), lens[b:b + 1].contiguous())
        assert torch.equal(_bits(one[0]), _bits(got[b])), \
            f"{ids(dtype)} row {b} (T = {n}): max |batch - alone| = {float((one[0] - got[b]).abs().max()):.3e}"


def test_forward_rows_against_the_reference(gpu, encoder):
    dtype, enc, _rt, x, _lens, got = encoder
    got = got.cpu()
    if dtype == torch.float32:
        from oracle.s2_step import SD, mel_style_encoder

        sd = SD({k: v.detach().double().cpu() for k, v in enc.state_dict().items()})
        for b, n in enumerate(FR_T):
            ref = mel_style_encoder(sd, x[b:b + 1, :n].double().transpose(1, 2), torch.ones(1, 1, n, dtype=torch.float64))[0, :, 0]
            err, bound = float((got[b].double() - ref).abs().max()), 1e-3 * max(1.0, float(ref.abs().max()))
            print(f"MEASURED fp32 forward_rows T = {n}: max |d| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (b, err, bound)
        return
    seen = []
    hook = enc.fc.register_forward_hook(lambda _m, _i, o: seen.append(o.detach().float().cpu()))
    try:
        for b, n in enumerate(FR_T):
            xb = x[b:b + 1, :n].contiguous().to(gpu)
            with torch.no_grad(), _amp(dtype):
                v = enc(xb, torch.ones(1, n, 1, device=gpu))            # the parent's pass: what _style runs per reference
            assert v.dtype == torch.float32            # autocast runs the parent's sum in fp32 too
            v, y = v[0].double().cpu(), seen.pop()[0].double()          # y [T, 512]: the frames the mean is taken of
            assert not seen and tuple(y.shape) == (n, 512)
            bound = 2.0 ** -7 * v.abs() + (n + 1) * U * y.abs().mean(0)
            frac = float(((got[b].double() - v).abs() / bound).max())
            print(f"MEASURED bf16 forward_rows vs the parent, T = {n}: |d| / bound = {frac:.3f}")
            assert frac <= 1.0, (b, frac)
    finally:
        hook.remove()


def test_forward_rows_is_the_inference_form(gpu, encoder):
    from easevoice_trainer_amd.hip.lib import EvtError

    dtype, enc, _rt, x, lens, _got = encoder
    enc.train()
    try:
        with pytest.raises(EvtError):
            enc.forward_rows(x.to(gpu), lens)
    finally:
        enc.eval()


# ------------------------------------------------------------------------------------ precomputed voices in the decoder
CODE_LENS, TEXT_LENS = [3, 7], [4, 9]


@pytest.fixture(scope="module", params=DTYPES, ids=ids)
def voice(request, gpu):
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    net = models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)
    weight = {k: v.detach().clone() for k, v in net.state_dict().items() if "enc_q" not in k}
    v = SoVITSVoice({"weight": weight, "config": hps, "info": "fixture"}, device=str(gpu), dtype=request.param)
    d = decode_inputs()
    codes, text = d["codes"][0, 0], d["text"][0]
    pc = torch.nn.utils.rnn.pad_sequence([codes[:n] for n in CODE_LENS], batch_first=True).unsqueeze(0)
    pt = torch.nn.utils.rnn.pad_sequence([text[:n] for n in TEXT_LENS], batch_first=True)
    noise = torch.randn(2, 192, 16, generator=torch.Generator().manual_seed(3))
    refers = [r.to(gpu) for r in d["refers"]]
    with torch.no_grad(), _amp(request.param):
        styles = torch.cat([v.model._style(r) for r in refers], 0)
    return v, pc, pt, noise, refers, styles


def test_decode_batch_with_styles_equals_refer(voice):
    v, pc, pt, noise, refers, styles = voice
    kw = dict(noise_scale=0.5, noise=noise)
    want = v.decode_batch(pc, CODE_LENS, pt, TEXT_LENS, refers, **kw)
    got = v.decode_batch(pc, CODE_LENS, pt, TEXT_LENS, None, style=styles, **kw)
    assert len(got) == 2 and [g.numel() for g in got] == [n * 2 * 640 for n in CODE_LENS]
    for b in range(2):
        assert torch.equal(got[b], want[b]), b
    # one shared voice [1, gin] against one shared reference
    want = v.decode_batch(pc, CODE_LENS, pt, TEXT_LENS, refers[0], **kw)
    got = v.decode_batch(pc, CODE_LENS, pt, TEXT_LENS, None, style=styles[:1], **kw)
    for b in range(2):
        assert torch.equal(got[b], want[b]), b


def test_decode_with_style_equals_refer(voice):
    v, pc, pt, noise, refers, styles = voice
    for b in range(2):
        args = (pc[:, b:b + 1, :CODE_LENS[b]], pt[b:b + 1, :TEXT_LENS[b]])
        want = v.decode(*args, refers[b], noise_scale=0.5, noise=noise[b:b + 1])
        got = v.decode(*args, None, noise_scale=0.5, noise=noise[b:b + 1], style=styles[b:b + 1])
        assert torch.equal(got, want), b


def test_style_refusals(voice):
    from easevoice_trainer_amd.hip.lib import EvtError

    v, pc, pt, noise, refers, styles = voice
    args = (pc, CODE_LENS, pt, TEXT_LENS)
    for refer, style in ((refers, styles),                               # both
                         (None, styles[:, :100]), (None, styles[0]),     # wrong shapes
                         (None, torch.cat([styles, styles[:1]], 0)),     # 3 rows for a batch of 2
                         (None, styles.cpu())):                          # wrong device
        with pytest.raises(EvtError):
            v.decode_batch(*args, refer, noise_scale=0.5, noise=noise, style=style)
    one = (pc[:, :1, :3], pt[:1, :4])
    for refer, style in ((refers[0], styles[:1]), (None, styles), (None, styles[:1].cpu())):
        with pytest.raises(EvtError):
            v.decode(*one, refer, noise_scale=0.5, noise=noise[:1], style=style)


def test_style_rows_of_the_model(voice, gpu):
    """SynthesizerTrn.style_rows on channels-last spectrograms padded together: the dtype _style returns, every row close to
    _style of the reference alone (the per-element bf16 bound is test_forward_rows_against_the_reference's; here its first
    term on the largest component, 2^-7 max |v|, in bf16, and the fp32 parity bound in fp32)"""
    v, _pc, _pt, _noise, refers, styles = voice
    t = [r.size(2) for r in refers]
    spec = torch.zeros(2, max(t), 1025, device=gpu)
    for b, r in enumerate(refers):
        spec[b, :t[b]] = r[0].transpose(0, 1)
    got = v.style_rows(spec, t)
    assert got.dtype == styles.dtype and tuple(got.shape) == tuple(styles.shape)
    tol = (2.0 ** -7 if v.dtype == torch.bfloat16 else 1e-3) * max(1.0, float(styles.float().abs().max()))
    assert float((got.float() - styles.float()).abs().max()) <= tol
    from easevoice_trainer_amd.hip.lib import EvtError

    with pytest.raises(EvtError):
        v.style_rows(spec[..., :700].contiguous(), t)
