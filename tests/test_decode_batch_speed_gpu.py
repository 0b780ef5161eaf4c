"""GPU: SynthesizerTrn.decode_batch(speed=...) -- a ragged batch decoded at one speed, or at one speed per row, in one s2
pass.  Requirement under test: row b is what decode(speed=speed[b]) gives for fragment b alone, with
int(T_b / speed[b]) + 1 frames (T_b where the row's speed is 1); and speed 1, scalar or per row, is the call without the
keyword.  The batch is the one of tests/test_vocoder_ragged_gpu.py (11, 30 and 60 codes; row 1 is the fixture of
tests/golden/s2_decode.pt, whose speed = 1.25 case the reference computed), the bounds are the ones the project puts on
batch vs alone (1e-3 of max-abs in fp32, whole row and last 4096 samples) and on decode vs the reference
(tests/test_s2_model_gpu.py::test_decode_and_extract_latent)."""
import json
import os

import pytest
import torch

from util_fill import decode_inputs, fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CODES = [11, 30, 60]
MIXED = [0.8, 1.25, 1.0]


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _export():
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    net = models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)                                   # the weights of tests/golden/s2_decode.pt
    weight = {k: v.detach().clone() for k, v in net.state_dict().items() if "enc_q" not in k}
    return weight, hps


def _batch(d):
    """short row (the fixture's first 11 codes, 9 phonemes), the fixture, long row (its codes and phonemes twice over);
    the prior noise is wide enough for the long row at speed 0.8 (151 frames)"""
    codes, text = d["codes"][0, 0], d["text"][0]
    rows_c = [codes[:11], codes, torch.cat([codes, codes])]
    rows_t = [text[:9], text, torch.cat([text, text])]
    pc = torch.nn.utils.rnn.pad_sequence(rows_c, batch_first=True).unsqueeze(0)
    pt = torch.nn.utils.rnn.pad_sequence(rows_t, batch_first=True)
    noise = torch.randn(3, 192, 160, generator=torch.Generator().manual_seed(99))
    noise[1, :, :d["noise"].size(2)] = d["noise"][0]
    return rows_c, rows_t, pc, pt, noise


def _frames(speeds):
    return [2 * n if v == 1 else int(2 * n / v) + 1 for n, v in zip(CODES, speeds)]


@pytest.fixture(scope="module")
def decoded(gpu):
    """fp32, one reference: the batch at 1.25, at [0.8, 1.25, 1.0], without the keyword, at 1 and at [1, 1, 1], and every
    row alone through decode at 0.8, 1.0 and 1.25; computed once"""
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice

    weight, hps = _export()
    dg = torch.load(os.path.join(HERE, "golden", "s2_decode.pt"), weights_only=False)
    d = decode_inputs()
    voice = SoVITSVoice({"weight": weight, "config": hps, "info": "fixture"}, device=str(gpu), dtype=torch.float32)
    rows_c, rows_t, pc, pt, noise = _batch(d)
    args = (pc, [t.numel() for t in rows_c], pt, [t.numel() for t in rows_t], d["refers"][0])
    kw = dict(noise_scale=0.5, noise=noise)
    out = {"plain": voice.decode_batch(*args, **kw)}
    for name, speed in (("1.25", 1.25), ("mixed", MIXED), ("one", 1), ("ones", [1, 1, 1])):
        out[name] = voice.decode_batch(*args, speed=speed, **kw)
    alone = {}
    for b in range(3):
        for v in sorted(set(MIXED)):
            alone[b, v] = voice.decode(rows_c[b].view(1, 1, -1), rows_t[b].view(1, -1), d["refers"][0], noise_scale=0.5,
                                       speed=v, noise=noise[b:b + 1])[0, 0].cpu()
    torch.cuda.synchronize()
    out = {k: [o.cpu() for o in v] for k, v in out.items()}
    return out, alone, (weight, hps, dg, d, voice, args, kw)


def _gold_125(dg):
    (c,) = [c for c in dg["cases"] if c["speed"] == 1.25]
    assert c["n_refer"] == 1
    return c


def test_uniform_speed_rows_equal_decode_alone(decoded):
    out, alone, _ = decoded
    for b, (o, n) in enumerate(zip(out["1.25"], _frames([1.25] * 3))):
        a = alone[b, 1.25]
        assert o.dim() == 1 and o.numel() == n * 640 == (int(2 * CODES[b] / 1.25) + 1) * 640 and o.shape == a.shape, b
        print("speed 1.25 row", b, "rel", rel(o, a), "last 4096", rel(o[-4096:], a[-4096:]))
        assert rel(o, a) < 1e-3, (b, rel(o, a))
        assert rel(o[-4096:], a[-4096:]) < 1e-3, (b, rel(o[-4096:], a[-4096:]))


def test_uniform_speed_fixture_row_meets_reference(decoded):
    out, _alone, (_w, _h, dg, *_rest) = decoded
    c = _gold_125(dg)
    o = out["1.25"][1]
    assert o.numel() == c["shape"][-1]
    assert rel(o[:4096], c["o_head"]) < 1e-3 and rel(o[::37], c["o_dec"]) < 1e-3
    assert abs(float(o.double().pow(2).sum()) - c["sq_sum"]) < 2e-3 * c["sq_sum"]


def test_mixed_speeds_rows_equal_decode_alone(decoded):
    out, alone, _ = decoded
    assert _frames(MIXED)[2] == 2 * CODES[2]                 # the speed-1 row is not interpolated: T_b frames, not T_b + 1
    for b, (o, n, v) in enumerate(zip(out["mixed"], _frames(MIXED), MIXED)):
        a = alone[b, v]
        assert o.dim() == 1 and o.numel() == n * 640 and o.shape == a.shape, (b, o.shape, a.shape)
        print("speed", v, "row", b, "rel", rel(o, a), "last 4096", rel(o[-4096:], a[-4096:]))
        assert rel(o, a) < 1e-3, (b, rel(o, a))
        assert rel(o[-4096:], a[-4096:]) < 1e-3, (b, rel(o[-4096:], a[-4096:]))


def test_speed_one_is_the_call_without_the_keyword(decoded):
    out, _alone, _ = decoded
    for name in ("one", "ones"):
        assert len(out[name]) == 3
        for o, p in zip(out[name], out["plain"]):
            assert torch.equal(o, p), name


def test_speed_errors(decoded):
    from easevoice_trainer_amd.hip.lib import EvtError

    _out, _alone, (_w, _h, _dg, _d, voice, args, kw) = decoded
    for bad in (0, float("nan"), float("inf"), -1.0, [1.25, 1.25], [1.0, 0.0, 1.0]):
        with pytest.raises(EvtError, match="speed"):
            voice.decode_batch(*args, speed=bad, **kw)
    with pytest.raises(EvtError, match="row 1"):
        voice.decode_batch(*args, speed=[1.0, float("nan"), 1.0], **kw)
    # the long row at 0.8 needs int(120 / 0.8) + 1 = 151 columns of prior noise, more than its 120 frames: a table of 150
    # is refused, not sliced
    slow_last = [1.0, 1.25, 0.8]
    assert _frames(slow_last) == [22, 49, 151]
    with pytest.raises(EvtError, match="noise"):
        voice.decode_batch(*args, noise_scale=0.5, noise=kw["noise"][:, :, :150], speed=slow_last)
    got = voice.decode_batch(*args, noise_scale=0.5, noise=kw["noise"][:, :, :151], speed=slow_last)
    assert [g.numel() for g in got] == [n * 640 for n in _frames(slow_last)]


def test_speed_bf16(gpu, decoded):
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice

    _out, _alone, (weight, hps, dg, d, _voice, args, kw) = decoded
    voice = SoVITSVoice({"weight": {k: v.half() for k, v in weight.items()}, "config": hps, "info": "fixture"},
                        device=str(gpu), dtype=torch.bfloat16)
    c = _gold_125(dg)
    got = voice.decode_batch(*args, speed=1.25, **kw)
    assert [g.numel() for g in got] == [n * 640 for n in _frames([1.25] * 3)]
    assert all(bool(torch.isfinite(g).all()) for g in got)
    print("bf16 speed 1.25 fixture row vs the reference:", rel(got[1][::37], c["o_dec"]))
    assert rel(got[1][::37], c["o_dec"]) < 5e-2, rel(got[1][::37], c["o_dec"])
