"""GPU: CN-HuBERT on ragged batches of clips -- the clip front end (evt_hubert_front_rows, evt_clip_rescale_rows of
csrc/feat_ops.hip), HubertModel.forward_rows / CNHubert.batch, FeatureWriter.ssl_batch and inference.semantic.prompt_semantics.
The reference of a ragged batch is EACH CLIP ALONE: a float64 restatement for the front kernel, numpy's rescale_clip for the
rescaling, transformers' HubertModel on the host (random-initialised base architecture, as test_feature_extractors_gpu.py)
for the model.  Tolerances are that file's stage tolerances: 1e-3 of max-abs in fp32, 6e-2 in 16-bit."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = {torch.float32: 1e-3, torch.bfloat16: 6e-2, torch.float16: 6e-2}
FRONT_N = (10, 14, 400, 3217, 9000)      # 1 frame, 1 frame, 79 / 642 / 1799 frames: 2, 11 and 29 chunks of 64, ragged last
NEAR_CONST = 7                           # the channel whose convolution output is near-constant


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ---------------------------------------------------------------- front kernel
_FRONT = {}


def _front_case():
    """rows, weights and the float64 reference per row, built once"""
    if not _FRONT:
        g = torch.Generator().manual_seed(11)
        w = 0.3 * torch.randn(512, 10, generator=g)
        w -= w.mean(dim=1, keepdim=True)                 # zero-sum taps: the rows' DC does not reach these channels
        w[NEAR_CONST] = 0.1                              # ... and reaches this one in full: c = 0.1 * (10 * 30 + sum of noise)
        gamma = 1 + 0.1 * torch.randn(512, generator=g)
        beta = 0.05 * torch.randn(512, generator=g)
        rows = [30.0 + 0.1 * torch.randn(n, generator=g) for n in FRONT_N]
        refs = []
        for r in rows:
            c = r.double().unfold(0, 10, 5) @ w.double().T                       # [T, 512]
            mean, var = c.mean(0), c.var(0, unbiased=False)
            y = (c - mean) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
            refs.append(0.5 * y * (1 + torch.erf(y / math.sqrt(2.0))))
        c7 = rows[-1].double().unfold(0, 10, 5) @ w[NEAR_CONST].double()
        assert 300 < float(c7.mean() / c7.std()) < 3000                          # mean about 1e3 x its deviation
        _FRONT.update(w=w, gamma=gamma, beta=beta, rows=rows, refs=refs)
    return _FRONT


def _padded(rows, width, fill, device):
    x = torch.full((len(rows), width), fill, dtype=torch.float32)
    for b, r in enumerate(rows):
        x[b, :r.numel()] = r
    return x.to(device)


def _front(case, gpu, dtype, rows=None, width=None, fill=0.0):
    from easevoice_trainer_amd.hip import feat
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    rows = case["rows"] if rows is None else rows
    width = max(r.numel() for r in rows) if width is None else width
    lens = torch.tensor([r.numel() for r in rows], dtype=torch.int32).to(gpu)
    return feat.hubert_front_rows(_padded(rows, width, fill, gpu), lens, case["w"].to(gpu), case["gamma"].to(gpu),
                                  case["beta"].to(gpu), 1e-5, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_front_rows_match_float64_per_row(gpu, dtype):
    case = _front_case()
    out = _front(case, gpu, dtype)
    assert out.shape == (len(FRONT_N), (9000 - 10) // 5 + 1, 512) and out.dtype == dtype
    for b, ref in enumerate(case["refs"]):
        t = ref.size(0)
        err = _rel(out[b, :t], ref)
        err7 = _rel(out[b, :t, NEAR_CONST], ref[:, NEAR_CONST])
        print(f"front {dtype} n={FRONT_N[b]} frames={t}: rel err {err:.3e}, near-constant channel {err7:.3e}")
        assert err < TOL[dtype], (FRONT_N[b], err)
        if t > 1:
            assert err7 < TOL[dtype], (FRONT_N[b], err7)       # E[x^2] - E[x]^2 in fp32 loses this channel's variance
        assert not out[b, t:].any(), "tail not exactly zero"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_front_rows_padding_and_batch_do_not_enter(gpu, dtype):
    """the pad region is never read (1e30 / NaN there change no bit), a row is bit for bit the row alone"""
    case = _front_case()
    base = _front(case, gpu, dtype, width=9100)
    assert torch.isfinite(base.float()).all()
    for fill in (1e30, float("nan")):
        assert torch.equal(_bits(_front(case, gpu, dtype, width=9100, fill=fill)), _bits(base)), fill
    for b, r in enumerate(case["rows"]):
        alone = _front(case, gpu, dtype, rows=[r])
        t = alone.size(1)
        assert t == max((r.numel() - 10) // 5 + 1, 0)
        assert torch.equal(_bits(alone[0]), _bits(base[b, :t])), FRONT_N[b]


def _front_raw(gpu, dtype_code, wav, lens, w, gamma, beta, out, ws, ws_floats=None, nseq=None, n=None, eps=1e-5):
    from easevoice_trainer_amd.hip import lib as L

    p = lambda t: C.c_void_p(t if isinstance(t, int) else (t.data_ptr() if t is not None else 0))  # noqa: E731
    fn = L.lib().evt_hubert_front_rows
    return fn(C.c_int32(dtype_code), p(wav), p(lens), C.c_int32(wav.size(0) if nseq is None else nseq),
              C.c_int32(wav.size(1) if n is None else n), p(w), p(gamma), p(beta), C.c_float(eps), p(out), p(ws),
              C.c_int64(ws.numel() if ws_floats is None else ws_floats), L.stream_ptr())


def test_front_rows_write_every_element_and_refuse_bad_arguments(gpu):
    from easevoice_trainer_amd.hip import feat
    from easevoice_trainer_amd.hip import lib as L

    case = _front_case()
    rows = case["rows"]
    wav = _padded(rows, 9003, 0.0, gpu)
    lens = torch.tensor([r.numel() for r in rows], dtype=torch.int32).to(gpu)
    w, gamma, beta = case["w"].to(gpu), case["gamma"].to(gpu), case["beta"].to(gpu)
    lib = L.lib()
    t1 = (9003 - 10) // 5 + 1
    need = lib.evt_hubert_front_ws_floats(len(rows), 9003)
    assert need == len(rows) * 512 * (-(-t1 // 64) + 2)
    assert lib.evt_hubert_front_ws_floats(0, 9003) == 0 and lib.evt_hubert_front_ws_floats(1, 9) == 0
    ws = torch.empty(need + 4, dtype=torch.float32, device=gpu)
    for dtype, code in ((torch.float32, L.DT_F32), (torch.bfloat16, L.DT_BF16)):
        out = torch.full((len(rows), t1, 512), 777.0, dtype=dtype, device=gpu)
        assert _front_raw(gpu, code, wav, lens, w, gamma, beta, out, ws) == 0
        assert not (out == 777.0).any(), "an element of out was not written"
        assert torch.equal(_bits(out[:, :(9000 - 10) // 5 + 1]), _bits(_front(case, gpu, dtype, width=9003)[:, :(9000 - 10) // 5 + 1]))
    out = torch.empty(len(rows), t1, 512, dtype=torch.float32, device=gpu)
    ok = dict(wav=wav, lens=lens, w=w, gamma=gamma, beta=beta, out=out, ws=ws)
    for name in ("wav", "lens", "w", "gamma", "beta", "out", "ws"):
        assert _front_raw(gpu, L.DT_F32, **{**ok, name: None}, nseq=len(rows), n=9003,
                          ws_floats=need) == 22, name                                        # NULL pointer
    assert _front_raw(gpu, L.DT_F32, **ok, nseq=0) == 22 and _front_raw(gpu, L.DT_F32, **ok, n=9) == 22
    assert _front_raw(gpu, L.DT_F32, **ok, ws_floats=need - 1) == 22
    assert _front_raw(gpu, L.DT_F32, **ok, eps=-1.0) == 22
    assert _front_raw(gpu, L.DT_F32, **{**ok, "out": out.data_ptr() + 4}) == 22              # misaligned out
    assert _front_raw(gpu, L.DT_F32, **{**ok, "ws": ws.data_ptr() + 4}, ws_floats=need) == 22  # misaligned workspace
    assert _front_raw(gpu, L.DT_F16, **ok) == 95 and _front_raw(gpu, 7, **ok) == 95          # the bf16 build is selected
    torch.cuda.synchronize()
    with pytest.raises(L.EvtError):
        feat.hubert_front_rows(wav, lens.long(), w, gamma, beta, 1e-5, torch.float32)
    with pytest.raises(L.EvtError):
        feat.hubert_front_rows(wav, lens.cpu(), w, gamma, beta, 1e-5, torch.float32)
    with pytest.raises(L.EvtError):
        feat.hubert_front_rows(wav, lens[:2], w, gamma, beta, 1e-5, torch.float32)
    with pytest.raises(L.EvtError):
        feat.hubert_front_rows(wav[:, :9].contiguous(), lens, w, gamma, beta, 1e-5, torch.float32)
    with pytest.raises(L.EvtError):
        feat.hubert_front_rows(wav, lens, w[:, :9].contiguous(), gamma, beta, 1e-5, torch.float32)


# ---------------------------------------------------------------- clip_rescale_rows
def test_clip_rescale_rows_equal_numpy_bit_for_bit(gpu):
    from easevoice_trainer_amd.feature_extractor.normalize import rescale_clip
    from easevoice_trainer_amd.hip import feat
    from easevoice_trainer_amd.hip import lib as L

    rs = np.random.RandomState(21)
    rows = [(rs.rand(n).astype(np.float32) * 2 - 1) * np.float32(a) for n, a in ((1, 0.37), (2, 0.9), (641, 1.0), (70001, 0.61))]
    rows[2][17] = -1.0                                                        # a peak of exactly 1
    assert all(np.abs(r).max() <= 1 for r in rows)
    width = 70001 + 13
    x = np.full((len(rows), width), np.nan, dtype=np.float32)                  # the pad region is never read
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32).to(gpu)
    f, q, peak = feat.clip_rescale_rows(torch.from_numpy(x).to(gpu), lens)
    assert f.dtype == torch.float32 and q.dtype == torch.int16 and peak.dtype == torch.float32
    f, q, peak = f.cpu().numpy(), q.cpu().numpy(), peak.cpu().numpy()
    for b, r in enumerate(rows):
        want_q, want_f = rescale_clip(r)
        n = len(r)
        assert peak[b] == np.abs(r).max()
        assert np.array_equal(q[b, :n], want_q), (n, int(np.abs(q[b, :n].astype(np.int32) - want_q).max()))
        assert np.array_equal(f[b, :n].view(np.int32), want_f.view(np.int32)), n
        assert not f[b, n:].any() and not q[b, n:].any()
        assert np.abs(q[b, :n].astype(np.int32)).max() <= 31949
    # a clip the reference skips, a clip with a NaN, a silent clip
    loud = rows[2] * np.float32(2.5)
    bad = rows[2].copy()
    bad[300] = np.nan
    x = np.zeros((3, 641), dtype=np.float32)
    x[0], x[1] = loud, bad
    f, q, peak = feat.clip_rescale_rows(torch.from_numpy(x).to(gpu), torch.tensor([641, 641, 641], dtype=torch.int32).to(gpu))
    peak = peak.cpu().numpy()
    assert peak[0] == np.abs(loud).max() == 2.5 and peak[0] > 2.2
    assert np.isnan(peak[1]) and peak[2] == 0
    assert int(q[0].max()) == 32767 and int(q[0].min()) == -32768              # saturated where numpy's cast is undefined
    with pytest.raises(L.EvtError):
        feat.clip_rescale_rows(torch.from_numpy(x).to(gpu), torch.tensor([641, 641, 641]).to(gpu))
    with pytest.raises(L.EvtError):
        feat.clip_rescale_rows(torch.from_numpy(x).to(gpu).double(), torch.tensor([641, 641, 641], dtype=torch.int32).to(gpu))


# ---------------------------------------------------------------- whole model
def _hf_hubert(seed=0):
    """the random-initialised base model of test_feature_extractors_gpu.py::_hf_hubert, restated"""
    from transformers import HubertConfig
    from transformers import HubertModel as HF

    torch.manual_seed(seed)
    hf = HF(HubertConfig()).eval()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if n.endswith("layer_norm.weight") or n.endswith("LayerNorm.weight"):
                p.add_(0.1 * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.add_(0.05 * torch.randn_like(p))
    return hf


_MODEL = {}
CLIP_N = (400, 9000, 2 * 16000 + 37)


def _model_case():
    """the HF model, three clips and HF's last_hidden_state of each clip ALONE, computed once"""
    if not _MODEL:
        hf = _hf_hubert()
        g = torch.Generator().manual_seed(3)
        clips = [torch.randn(n, generator=g) * 0.1 * 1145.14 / 32768 * 30 for n in CLIP_N]
        with torch.no_grad():
            refs = [hf(c.unsqueeze(0))["last_hidden_state"][0] for c in clips]
        _MODEL.update(sd=hf.state_dict(), clips=clips, refs=refs, hub={})
    return _MODEL


def _hub(gpu, dtype):
    from easevoice_trainer_amd.feature_extractor import CNHubert

    case = _model_case()
    if dtype not in case["hub"]:
        case["hub"][dtype] = CNHubert(case["sd"], gpu, dtype)
    return case["hub"][dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ragged_batch_matches_transformers_clip_by_clip(gpu, dtype):
    case = _model_case()
    hub = _hub(gpu, dtype)
    hs, frame_lens = hub.last_hidden_state_batch(case["clips"])
    assert frame_lens == [r.size(0) for r in case["refs"]] == [hub.model.frames(n) for n in CLIP_N]
    assert hs.shape == (3, max(frame_lens), 768)
    for b, ref in enumerate(case["refs"]):
        err = _rel(hs[b, :frame_lens[b]], ref)
        print(f"forward_rows {dtype} n={CLIP_N[b]}: rel err to transformers {err:.3e}")
        assert err < TOL[dtype], (CLIP_N[b], err)
        assert not hs[b, frame_lens[b]:].any()
    # the (padded, lens) form with garbage in the padding, and batch() against the single-clip path
    width = max(CLIP_N) + 50
    padded = torch.full((3, width), float("nan"))
    for b, c in enumerate(case["clips"]):
        padded[b, :c.numel()] = c
    hs2, fl2 = hub.last_hidden_state_batch((padded, list(CLIP_N)))
    assert fl2 == frame_lens and hs2.shape == hs.shape and torch.isfinite(hs2.float()).all()
    assert _rel(hs2, hs) < TOL[dtype]
    rows = hub.batch(case["clips"])
    for b, c in enumerate(case["clips"]):
        alone = hub(c)
        assert rows[b].shape == alone.shape == (1, 768, frame_lens[b]) and rows[b].dtype == torch.float32
        err = _rel(rows[b], alone)
        print(f"batch {dtype} n={CLIP_N[b]}: rel diff to __call__ {err:.3e}")
        assert err < TOL[dtype], (CLIP_N[b], err)
    with pytest.raises(ValueError):
        hub.last_hidden_state_batch([case["clips"][1], torch.zeros(399)])


# ---------------------------------------------------------------- ssl_batch
def test_ssl_batch_writes_what_ssl_writes(gpu, tmp_path):
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter

    hub = _hub(gpu, torch.float32)
    rs = np.random.RandomState(6)
    clips = {"a.wav": (rs.rand(32000 + 11) - 0.5).astype(np.float32),
             "b.wav": (rs.rand(2 * 32000 + 5) - 0.5).astype(np.float32) * 1.7,
             "c.wav": (rs.rand(3 * 32000 + 211) - 0.5).astype(np.float32) * 0.3,
             "loud.wav": (rs.rand(32000 + 640) - 0.5).astype(np.float32),
             "have.wav": (rs.rand(40000) - 0.5).astype(np.float32)}
    clips["loud.wav"] *= np.float32(2.5) / np.abs(clips["loud.wav"]).max()
    assert np.abs(clips["loud.wav"]).max() > 2.2
    w = FeatureWriter(str(tmp_path / "batch"), hub, None)
    torch.save(torch.zeros(1), tmp_path / "batch" / "4-cnhubert" / "have.wav.pt")
    names = ["a.wav", "loud.wav", "b.wav", "have.wav", "c.wav"]
    assert w.ssl_batch(names, [clips[n] for n in names]) == [True] * 5
    one = FeatureWriter(str(tmp_path / "one"), hub, None)
    for name in ("a.wav", "b.wav", "c.wav"):
        assert one.ssl(name, clips[name])
        got = torch.load(tmp_path / "batch" / "4-cnhubert" / (name + ".pt"))
        want = torch.load(tmp_path / "one" / "4-cnhubert" / (name + ".pt"))
        assert got.shape == want.shape == (1, 768, hub.model.frames(len(clips[name]) // 2)) and got.dtype == torch.float32
        err = _rel(got, want)
        print(f"ssl_batch {name}: rel diff to ssl {err:.3e}")
        assert err < 1e-3, (name, err)
        assert open(tmp_path / "batch" / "5-wav32k" / name, "rb").read() == open(tmp_path / "one" / "5-wav32k" / name, "rb").read()
    assert sorted(os.listdir(tmp_path / "batch" / "5-wav32k")) == ["a.wav", "b.wav", "c.wav"]
    assert sorted(os.listdir(tmp_path / "batch" / "4-cnhubert")) == ["a.wav.pt", "b.wav.pt", "c.wav.pt", "have.wav.pt"]
    assert torch.load(tmp_path / "batch" / "4-cnhubert" / "have.wav.pt").shape == (1,)
    # a non-finite peak returns False and writes nothing; the clip next to it is written
    bad = clips["a.wav"].copy()
    bad[100] = np.nan
    assert w.ssl_batch(["nan.wav", "d.wav", "a.wav"], [bad, clips["a.wav"], clips["a.wav"]]) == [False, True, True]
    assert not os.path.exists(tmp_path / "batch" / "4-cnhubert" / "nan.wav.pt")
    assert torch.equal(torch.load(tmp_path / "batch" / "4-cnhubert" / "d.wav.pt"),
                       torch.load(tmp_path / "batch" / "4-cnhubert" / "a.wav.pt"))


# ---------------------------------------------------------------- prompt_semantics
def test_prompt_semantics_match_clip_by_clip(gpu):
    import json

    from easevoice_trainer_amd.inference.semantic import PROMPT_TAIL, prompt_semantics
    from easevoice_trainer_amd.module import models
    from easevoice_trainer_amd.runtime import ModelRuntime
    from util_fill import fill_module

    hub = _hub(gpu, torch.float32)
    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    d = hps["data"]
    net = models.SynthesizerTrn(d["filter_length"] // 2 + 1, hps["train"]["segment_size"] // d["hop_length"],
                                n_speakers=d["n_speakers"], **hps["model"])
    fill_module(net, 1)
    net.eval()
    rt = ModelRuntime(net, torch.float32, gpu)
    rt.prepare(force=True)
    extract = lambda s: net.extract_latent(s.to(gpu))  # noqa: E731
    g = torch.Generator().manual_seed(8)
    clips = [torch.randn(n, generator=g) * 0.1 for n in (3 * 16000, int(4.1 * 16000))]
    assert PROMPT_TAIL == 9600
    got = prompt_semantics(hub, extract, clips)
    assert len(got) == 2
    for b, c in enumerate(clips):
        alone = extract(hub(torch.cat([c, torch.zeros(PROMPT_TAIL)])))[0, 0]
        t = hub.model.frames(c.numel() + PROMPT_TAIL)
        assert got[b].dim() == 1 and got[b].numel() == alone.numel() == t // 2
        agree = float((got[b].cpu() == alone.cpu()).float().mean())
        print(f"prompt_semantics clip {b}: {agree:.4f} of {t // 2} codes agree")
        assert agree >= 0.99, agree          # a tie within fp32 rounding may pick the neighbouring row
    with pytest.raises(OSError):
        prompt_semantics(hub, extract, [clips[0], torch.zeros(2 * 16000)])
