"""GPU: evt_semantic_codes_rows (csrc/semantic.hip) -- ssl_proj + nearest code on ragged batches in one launch -- against the
float64 oracle of tests/semantic_refs.py, in fp32 and in both 16-bit input types (the inputs are rounded first, the oracle
is computed from the rounded values), at the model's D = 768, K = 1024 and at D = 128, K = 72 (a codebook tail).  B = 6 rows
of 1 / 2 / 63 / 64 / 67 / 131 frames: 0 / 1 / 31 / 32 / 33 / 65 codes -- an empty row, one code, either side of a tile edge, an
odd last frame, more than two tiles -- with Tmax above the longest row and NaN behind every row's frames.
  * integer-exact, planted and close-pair inputs: the codes equal the oracle's (tests/test_semantic_refs_cpu.py shows that
    these inputs leave one answer; the same condition is re-checked here on the rounded 16-bit inputs);
  * unplanted inputs: for EVERY frame the float64 distance of the chosen code is above the minimum by at most E;
  * a row alone, in the batch, and in the reversed batch with a larger Tmax gives the same codes;
  * an all-NaN live frame gives code 0; every invalid call returns EVT_EINVAL;
  * SynthesizerTrn.extract_latent_rows equals extract_latent row by row on the planted inputs and refuses an uninitialised
    codebook and malformed input;
  * end to end with a random-init CN-HuBERT on three clips of 0.5 .. 1 s: ssl_batch(tokens=True) + write_semantic writes the
    lines that write_semantic_tsv_batch writes from the files just saved, with the codebook planted on the clips' own
    projected features."""
import json
import os

import numpy as np
import pytest
import torch

import semantic_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
_cache = {}


def rounded_case(name, D, K, dtype):
    """(inputs with x rounded to dtype and widened again, the oracle of those), computed once per case"""
    key = (name, D, K, dtype)
    if key not in _cache:
        inp = dict(R.GENERATORS[name](D, K))
        inp["x"] = inp["x"].to(dtype).float()
        _cache[key] = (inp, R.oracle(inp["x"], inp["frames"], inp["w"], inp["bias"], inp["embed"]))
    return _cache[key]


def run(gpu, x, frames, w, bias, embed, dtype):
    from easevoice_trainer_amd.hip import feat as HF
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    codes, off = HF.semantic_codes_rows(x.to(gpu).to(dtype).contiguous(), frames, HF.make_proj_image(w.to(gpu)), bias.to(gpu),
                                        embed.to(gpu))
    assert codes.dtype == torch.int64 and off.dtype == torch.int64
    assert off.cpu().tolist() == np.concatenate([[0], np.cumsum([t // 2 for t in frames])]).tolist()
    assert codes.numel() == sum(t // 2 for t in frames)
    return list(torch.split(codes.cpu(), [t // 2 for t in frames]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,K", R.SHAPES)
@pytest.mark.parametrize("name", ["exact", "planted", "close"])
def test_codes_equal_the_oracle(gpu, name, D, K, dtype):
    inp, ora = rounded_case(name, D, K, dtype)
    if name != "exact":
        for o in ora:                        # the rounded inputs still leave one answer
            assert (o["margin"] >= 2 * o["E"]).all(), (float(o["margin"].min()), float(o["E"].max()))
    got = run(gpu, inp["x"], inp["frames"], inp["w"], inp["bias"], inp["embed"], dtype)
    for b, (g, o) in enumerate(zip(got, ora)):
        assert torch.equal(g, o["codes"]), (b, torch.nonzero(g != o["codes"]).flatten().tolist()[:8])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,K", R.SHAPES)
def test_unplanted_codes_are_within_the_bound_on_every_frame(gpu, D, K, dtype):
    inp, ora = rounded_case("unplanted", D, K, dtype)
    got = run(gpu, inp["x"], inp["frames"], inp["w"], inp["bias"], inp["embed"], dtype)
    worst = 0.0
    for b, (g, o) in enumerate(zip(got, ora)):
        assert g.numel() == o["codes"].numel() and bool(((g >= 0) & (g < K)).all())
        if not g.numel():
            continue
        excess = o["dist"].gather(1, g[:, None])[:, 0] - o["dist"].min(1).values
        worst = max(worst, float((excess / o["E"]).max()))
        assert (excess <= o["E"]).all(), (b, float((excess / o["E"]).max()))
    print(f"unplanted D={D} K={K} {dtype}: worst excess / E = {worst:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,K", R.SHAPES)
def test_a_row_does_not_depend_on_its_batch(gpu, D, K, dtype):
    inp, _ora = rounded_case("unplanted", D, K, dtype)
    x, frames = inp["x"], inp["frames"]
    args = (inp["w"], inp["bias"], inp["embed"], dtype)
    batch = run(gpu, x, frames, *args)
    B, tmax = len(frames), x.size(1)
    rev = torch.full((B, tmax + 37, D), float("nan"))
    for b in range(B):
        rev[B - 1 - b, :frames[b]] = x[b, :frames[b]]
    got_rev = run(gpu, rev, frames[::-1], *args)
    for b in range(B):
        alone = run(gpu, x[b:b + 1, :frames[b]].clone(), [frames[b]], *args)[0]
        assert torch.equal(alone, batch[b]), b
        assert torch.equal(got_rev[B - 1 - b], batch[b]), b


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,K", R.SHAPES)
def test_all_nan_live_frame_gives_code_0(gpu, D, K, dtype):
    """NaN reaches the kernel through the load path of the dtype: a whole pair, and one frame of a pair in another tile"""
    inp, ora = rounded_case("planted", D, K, dtype)
    x = inp["x"].clone()
    planted = ora[5]["codes"]
    t1 = next(t for t in range(1, 32) if int(planted[t]) != 0)                  # the planted codes there are not 0 anyway
    t2 = next(t for t in range(33, 65) if int(planted[t]) != 0)
    x[5, 2 * t1: 2 * t1 + 2] = float("nan")                                     # code frame t1 of the long row: both frames
    x[5, 2 * t2 + 1] = float("nan")                                             # code frame t2: its second frame only
    got = run(gpu, x, inp["frames"], inp["w"], inp["bias"], inp["embed"], dtype)
    want = [o["codes"].clone() for o in ora]
    want[5][t1] = 0
    want[5][t2] = 0
    for g, wnt in zip(got, want):
        assert torch.equal(g, wnt)


def test_invalid_calls_return_einval(gpu):
    from easevoice_trainer_amd.hip import feat as HF
    from easevoice_trainer_amd.hip import lib as L

    EINVAL = 22
    fn = L.lib().evt_semantic_codes_rows
    B, T, D, K = 2, 8, 128, 72
    hs = torch.zeros(B, T, D, device=gpu)
    frames = torch.tensor([8, 4], dtype=torch.int32, device=gpu)
    fh = torch.tensor([8, 4], dtype=torch.int32)
    off = torch.tensor([0, 4, 6], dtype=torch.int64, device=gpu)
    image, bias = torch.zeros(2 * D, D, device=gpu), torch.zeros(D, device=gpu)
    embed, ee = torch.zeros(K + 1, D, device=gpu), torch.zeros(K, device=gpu)
    codes = torch.full((6,), -1, dtype=torch.int64, device=gpu)

    def call(**kw):
        a = dict(dtype=0, hs=hs.data_ptr(), frames=frames.data_ptr(), fh=fh.data_ptr(), off=off.data_ptr(), B=B, T=T, D=D,
                 K=K, image=image.data_ptr(), bias=bias.data_ptr(), embed=embed.data_ptr(), ee=ee.data_ptr(),
                 codes=codes.data_ptr(), total=6)
        a.update(kw)
        return fn(a["dtype"], a["hs"], a["frames"], a["fh"], a["off"], a["B"], a["T"], a["D"], a["K"], a["image"], a["bias"],
                  a["embed"], a["ee"], a["codes"], a["total"], L.stream_ptr())

    assert call() == 0 and call(fh=None) == 0
    torch.cuda.synchronize()
    assert bool((codes == 0).all())                      # zero distances everywhere: the first code
    for name in ("hs", "frames", "off", "image", "bias", "embed", "ee", "codes"):
        assert call(**{name: None}) == EINVAL, name
    bad = torch.tensor([8, 9], dtype=torch.int32)
    neg = torch.tensor([-1, 4], dtype=torch.int32)
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(K=0), dict(total=-1), dict(D=0), dict(D=96), dict(D=100),
               dict(D=1216), dict(dtype=7), dict(dtype=2), dict(fh=bad.data_ptr()), dict(fh=neg.data_ptr()),
               dict(embed=embed.data_ptr() + 4), dict(hs=hs.data_ptr() + 8), dict(bias=bias.data_ptr() + 4),
               dict(image=image.data_ptr() + 4)):
        assert call(**kw) == EINVAL, kw
    with pytest.raises(L.EvtError):
        HF.semantic_codes_rows(hs, [8, 9], image, bias, embed[:K].contiguous())
    with pytest.raises(L.EvtError):
        HF.semantic_codes_rows(hs, [8], image, bias, embed[:K].contiguous())
    with pytest.raises(L.EvtError):
        HF.semantic_codes_rows(hs.cpu(), [8, 4], image, bias, embed[:K].contiguous())


@pytest.fixture(scope="module")
def net(gpu):
    from easevoice_trainer_amd.module import models
    from easevoice_trainer_amd.runtime import ModelRuntime
    from util_fill import fill_module

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    d = hps["data"]
    m = models.SynthesizerTrn(d["filter_length"] // 2 + 1, hps["train"]["segment_size"] // d["hop_length"],
                              n_speakers=d["n_speakers"], **hps["model"])
    fill_module(m, 1)
    m.eval()
    rt = ModelRuntime(m, torch.float32, gpu)
    rt.prepare(force=True)
    m._keep_rt = rt
    return m


def _plant(net, w, bias, embed):
    with torch.no_grad():
        net.ssl_proj.weight.copy_(w)
        net.ssl_proj.bias.copy_(bias)
        cb = net.quantizer.vq.layers[0]._codebook
        cb.embed.copy_(embed)
        cb.inited.fill_(1.0)


@pytest.mark.parametrize("name", ["planted", "close"])
def test_extract_latent_rows_equals_extract_latent(gpu, net, name):
    inp, ora = rounded_case(name, 768, 1024, torch.float32)
    _plant(net, inp["w"], inp["bias"], inp["embed"])
    x, frames = inp["x"].to(gpu), inp["frames"]
    rows = net.extract_latent_rows(x, frames)
    assert len(rows) == len(frames) and all(r.dtype == torch.int64 and r.dim() == 1 for r in rows)
    assert all(r._base is rows[0]._base for r in rows)                        # views of one packed buffer
    for b, t in enumerate(frames):
        assert rows[b].numel() == t // 2
        assert torch.equal(rows[b].cpu(), ora[b]["codes"]), b
        if t >= 2:
            one = net.extract_latent(x[b:b + 1, :t].transpose(1, 2).contiguous())           # [1, 1, t // 2]
            assert torch.equal(one[0, 0], rows[b]), b
    # the 16-bit hidden states of a bf16 HuBERT go in as they are
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(torch.bfloat16)
    inp16, ora16 = rounded_case(name, 768, 1024, torch.bfloat16)
    rows16 = net.extract_latent_rows(inp16["x"].to(gpu).bfloat16(), frames)
    for b in range(len(frames)):
        assert torch.equal(rows16[b].cpu(), ora16[b]["codes"]), b


def test_extract_latent_rows_follows_the_live_parameters_and_refuses(gpu, net):
    from easevoice_trainer_amd.hip.lib import EvtError

    inp, ora = rounded_case("planted", 768, 1024, torch.float32)
    _plant(net, inp["w"], inp["bias"], inp["embed"])
    x, frames = inp["x"].to(gpu), inp["frames"]
    first = net.extract_latent_rows(x, frames)
    perm = torch.arange(1023, -1, -1)
    with torch.no_grad():                                                     # written in place: the cached norms are stale
        net.quantizer.vq.layers[0]._codebook.embed.copy_(inp["embed"][perm])
    second = net.extract_latent_rows(x, frames)
    for a, b in zip(first, second):
        assert torch.equal(1023 - a, b)
    for bad, fr in ((x[0], frames), (x[:, :, :704].contiguous(), frames), (x.cpu(), frames), (x, frames[:-1])):
        with pytest.raises(EvtError):
            net.extract_latent_rows(bad, fr)
    with torch.no_grad():
        net.quantizer.vq.layers[0]._codebook.inited.zero_()
    with pytest.raises(EvtError, match="not initialised"):
        net.extract_latent_rows(x, frames)
    _plant(net, inp["w"], inp["bias"], inp["embed"])
    for b, r in enumerate(net.extract_latent_rows(x, frames)):
        assert torch.equal(r.cpu(), ora[b]["codes"])


def test_ssl_batch_tokens_end_to_end(gpu, net, tmp_path):
    from transformers import HubertConfig
    from transformers import HubertModel as HF

    from easevoice_trainer_amd.feature_extractor import CNHubert
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter
    from easevoice_trainer_amd.inference.semantic import write_semantic_tsv_batch

    torch.manual_seed(5)
    hub = CNHubert(HF(HubertConfig()).eval().state_dict(), gpu, torch.float32)
    rs = np.random.RandomState(8)
    names = ["a.wav", "b.wav", "c.wav"]
    clips = [(rs.rand(n) - 0.5).astype(np.float32) for n in (16000, 24001, 32000)]          # 0.5 / 0.75 / 1 s at 32 kHz
    plain = FeatureWriter(str(tmp_path / "plain"), hub, None)
    assert plain.ssl_batch(names, clips) == [True] * 3
    feats = [torch.load(tmp_path / "plain" / "4-cnhubert" / (n + ".pt")) for n in names]
    # the codebook: every code frame's own projection (float64) first, random vectors of their scale behind them
    g = torch.Generator().manual_seed(9)
    w = torch.randn(768, 768, 2, generator=g) / 1536 ** 0.5
    bias = 0.1 * torch.randn(768, generator=g)
    hproj = torch.cat([torch.nn.functional.conv1d(f.double(), w.double(), bias.double(), stride=2)[0].t() for f in feats])
    embed = torch.randn(1024, 768, generator=g) * float(hproj.std())
    embed[: hproj.size(0)] = hproj.float()
    _plant(net, w, bias, embed)
    want, at = [], 0
    for f in feats:
        o = R.oracle_row(f[0].t(), w, bias, embed)
        assert (o["margin"] >= 2 * o["E"]).all(), (float(o["margin"].min()), float(o["E"].max()))
        assert torch.equal(o["codes"], torch.arange(at, at + f.size(2) // 2))
        at += f.size(2) // 2
        want.append(o["codes"].tolist())

    with pytest.raises(ValueError):
        FeatureWriter(str(tmp_path / "novoice"), hub, None).ssl_batch(names, clips, tokens=True)
    fw = FeatureWriter(str(tmp_path / "tok"), hub, None, voice=net)
    assert fw.ssl_batch(names, clips, tokens=True) == [True] * 3
    for n, f in zip(names, feats):                                           # the files are those of the plain pass
        assert torch.equal(torch.load(tmp_path / "tok" / "4-cnhubert" / (n + ".pt")), f)
    assert fw.write_semantic(names + ["missing.wav"]) == 3
    got = open(tmp_path / "tok" / "6-name2semantic.tsv", "rb").read()
    assert write_semantic_tsv_batch(net.extract_latent_rows, names + ["missing.wav"], str(tmp_path / "tok" / "4-cnhubert"),
                                    str(tmp_path / "files.tsv"), group=2, device=gpu) == 3
    assert got == open(tmp_path / "files.tsv", "rb").read()
    lines = got.decode("utf8").split("\n")
    assert lines[0] == "item_name\tsemantic_audio" and lines[4] == "" and len(lines) == 5
    for line, n, c in zip(lines[1:4], names, want):
        assert line == n + "\t" + " ".join(str(i) for i in c)
