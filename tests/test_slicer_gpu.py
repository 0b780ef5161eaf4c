"""The slicer's launches (csrc/slicer.hip through hip/slicer.py) and audiokit.slicer.slice_batch on the GPU against the
reference's recorded behaviour (tests/golden/slicer.json): RMS frames as bit patterns, chunk labels, peak bits and the
sha256 of every chunk's int16 bytes.  Every comparison is exact."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import slicer_inputs as I
from easevoice_trainer_amd.audiokit import slicer as SL
from easevoice_trainer_amd.hip import lib as L
from easevoice_trainer_amd.hip import slicer as S
from easevoice_trainer_amd.train.dataset import read_wav_pcm16

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "slicer.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs():
    """the recordings, built once and never written to"""
    out = {"A": I.case_a(), "B": I.case_b(), "C": I.case_c()}
    out.update({f"edge{k}": x for k, x in enumerate(I.edges())})
    for x in out.values():
        x.setflags(write=False)
    return out


def pack(arrays, dev, sentinel=None):
    """the arrays back to back on the device, `sentinel` (three of them) in front of, between and behind them"""
    parts, offs, pos = [], [], 0
    fence = np.full(3 if sentinel is not None else 0, sentinel if sentinel is not None else 0, dtype=np.float32)
    for a in arrays:
        parts.append(fence)
        pos += fence.shape[0]
        offs.append(pos)
        parts.append(a)
        pos += a.shape[0]
    parts.append(fence)
    return torch.from_numpy(np.concatenate(parts)).to(dev), offs, [a.shape[0] for a in arrays]


def rms_bits(x, offs, lens, win, hop):
    rms, frame_off = S.rms_frames_rows(x, offs, lens, win, hop)
    bits = rms.cpu().numpy().view(np.uint32)
    return [bits[frame_off[k]:frame_off[k + 1]] for k in range(len(offs))]


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_rms_frames_equal_the_reference_bits(gpu, golden, inputs, case):
    p = SL.SlicerParams(**golden[case]["params"])
    x, offs, lens = pack([inputs[case]], gpu)
    (got,) = rms_bits(x, offs, lens, p.win, p.hop)
    assert got.tolist() == golden[case]["rms"]


def test_rms_frames_of_short_recordings(gpu, golden, inputs):
    """1, 319, 320 and 400 samples (fewer than a window, a hop, one frame more) and 3 s, in one packed call"""
    p = SL.SlicerParams()
    x, offs, lens = pack([inputs[f"edge{k}"] for k in range(len(I.EDGE_LENGTHS))], gpu)
    for got, g in zip(rms_bits(x, offs, lens, p.win, p.hop), golden["edges"]):
        assert got.tolist() == g["rms"], g["n"]


def test_rms_frames_do_not_depend_on_the_batch(gpu, inputs):
    """three lengths in one packed call = the three single calls; with NaN between the recordings nothing changes and
    everything is finite: no sample outside a recording is read"""
    p = SL.SlicerParams()
    arrays = [inputs["A"], inputs["B"], inputs["C"]]
    single = [rms_bits(*pack([a], gpu), p.win, p.hop)[0] for a in arrays]
    together = rms_bits(*pack(arrays, gpu), p.win, p.hop)
    fenced = rms_bits(*pack(arrays, gpu, sentinel=NAN), p.win, p.hop)
    for a, s, t, f in zip(arrays, single, together, fenced):
        assert s.shape[0] == S.frame_count(a.shape[0], p.win, p.hop)
        assert np.array_equal(s, t) and np.array_equal(s, f)
        assert np.isfinite(f.view(np.float32)).all()


# the (hop, win) pairs the recipe was checked at against the reference, the sequential branch (win < 8), leftovers behind the
# eight accumulators, one leaf of 128, the largest window and the odd window below it (the deepest tree)
@pytest.mark.parametrize("hop,win", [(320, 960), (224, 800), (220, 816), (80, 176), (441, 1323), (8, 8), (3, 1), (5, 7),
                                     (16, 13), (64, 128), (64, 129), (1000, 8192), (997, 8191)])
def test_rms_frames_equal_the_recipe_at_other_windows(gpu, inputs, hop, win):
    """against the float32 emulation of the summation recipe (tests/test_slicer_cpu.py holds it to the reference's bits)"""
    arrays = [inputs["edge4"][:5001], inputs["B"][19990:20500], inputs["edge1"]]
    got = rms_bits(*pack(arrays, gpu, sentinel=NAN), win, hop)
    for a, g in zip(arrays, got):
        assert np.array_equal(g, I.emulate_rms(a, win, hop).view(np.uint32))


def test_span_peaks_and_pack_edge_spans(gpu, inputs):
    """an empty span (peak 0), a span holding a NaN (peak NaN), an all-zero span (packed as zeros), a span of one sample"""
    a = inputs["B"]
    zero_at = int(np.flatnonzero(a == 0)[0])
    buf = np.concatenate([a, [NAN], a[:100]]).astype(np.float32)
    x = torch.from_numpy(buf).to(gpu)
    src, n = [0, 5, a.shape[0] - 3, zero_at, 20000, 7], [a.shape[0], 0, 10, 50, 1, 4099]
    spans = S.Spans(x, src, n)
    peak = S.span_peaks(x, spans)
    got = peak.cpu().numpy()
    want = np.array([np.abs(buf[o:o + k]).max() if k else 0 for o, k in zip(src, n)], dtype=np.float32)
    assert np.isnan(got[2]) and np.isnan(want[2]) and got[3] == 0
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    out = S.slice_pack(x, spans, peak, 0.225, 0.75).cpu().numpy()
    assert out.shape[0] == sum(n)
    for k, (o, cnt, d) in enumerate(zip(src, n, spans.dst)):
        if k in (2, 3):
            assert not out[d:d + cnt].any()          # NaN -> 0, and zeros for the all-zero chunk
            continue
        v = buf[o:o + cnt].copy()
        if want[k] > 1:
            v /= want[k]
        w = (v / want[k] * np.float32(0.225)) + np.float32(0.75) * v
        assert np.array_equal(out[d:d + cnt], (w * np.float32(32767)).astype(np.int16)), k


def test_binding_refuses_what_it_cannot_serve(gpu):
    x = torch.zeros(1000, device=gpu)
    for bad in (x.double(), x.reshape(10, 100), x.cpu(), x[::2]):
        with pytest.raises(L.EvtError):
            S.rms_frames_rows(bad, [0], [10], 8, 8)
    for offs, lens in (([0], [0]), ([990], [11]), ([-1], [5]), ([0, 1], [5]), ([], [])):
        with pytest.raises(L.EvtError):
            S.rms_frames_rows(x, offs, lens, 8, 8)
    with pytest.raises(L.EvtError):
        S.rms_frames_rows(x, [0], [10], 8193, 8)
    with pytest.raises(L.EvtError):
        S.rms_frames_rows(x, [0], [10], 8, 0)
    with pytest.raises(L.EvtError):
        S.Spans(x, [995], [6])
    with pytest.raises(L.EvtError):
        S.span_peaks(torch.zeros(999, device=gpu), S.Spans(x, [0], [6]))
    with pytest.raises(L.EvtError):
        S.slice_pack(x, S.Spans(x, [0], [6]), torch.zeros(2, device=gpu), 0.2, 0.7)
    with pytest.raises(L.EvtError, match="inference only"):
        S.rms_frames_rows(x.clone().requires_grad_(), [0], [10], 8, 8)


def sha(pcm):
    return hashlib.sha256(pcm.cpu().numpy().astype("<i2").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def batch(golden, inputs, tmp_path_factory):
    """A, B, the edge recordings and a recording holding one NaN in ONE call, written to a directory"""
    keys = ["A", "edge0", "B", "edge1", "edge2", "nan", "edge3", "edge4"]
    bad = inputs["edge4"].copy()
    bad[777] = NAN
    recs = [bad if k == "nan" else inputs[k] for k in keys]
    params = [SL.SlicerParams(**(I.PARAMS_B if k == "B" else I.PARAMS_A)) for k in keys]
    out_dir = str(tmp_path_factory.mktemp("slicer"))
    names = [f"dir/{k}.reformatted.wav" for k in keys]
    return keys, SL.slice_batch(names, recs, params, golden["normalize_max"], golden["alpha_mix"], out_dir=out_dir), out_dir


def golden_of(golden, key):
    return golden["edges"][int(key[4:])] if key.startswith("edge") else golden[key]


def test_slice_batch_equals_the_reference(gpu, golden, batch):
    keys, results, _ = batch
    assert len(results) == len(keys)
    for key, (ok, slices) in zip(keys, results):
        if key == "nan":
            continue
        g = golden_of(golden, key)
        assert ok == g["sliced"] and len(slices) == len(g["chunks"]), key
        for s, c in zip(slices, g["chunks"]):
            assert (s.start, s.end, s.pcm.numel()) == (c["start"], c["end"], c["n"]), key
            assert s.name == "%s_%010d_%010d.wav" % (key, c["start"], c["end"])
            assert s.pcm.dtype == torch.int16 and s.pcm.is_cuda
            assert int(s.peak.cpu().numpy().view(np.uint32)) == c["peak"], key
            assert sha(s.pcm) == c["sha256"], (key, c["start"])
    assert sum(len(s) for _, s in results) == 5 + 3 + 1
    assert any(c["peak"] > np.float32(1).view(np.uint32) for c in golden["B"]["chunks"])     # the peak-above-1 division ran


def test_slice_batch_drops_a_recording_with_a_nan(gpu, batch):
    keys, results, _ = batch
    assert results[keys.index("nan")] == (False, [])


def test_slice_batch_files_hold_the_slices(gpu, golden, batch):
    keys, results, out_dir = batch
    want = {"%s_%010d_%010d.wav" % (k, c["start"], c["end"]) for k in keys if k != "nan"
            for c in golden_of(golden, k)["chunks"]}
    assert set(os.listdir(os.path.join(out_dir, "slices"))) == want
    for _, slices in results:
        for s in slices:
            pcm = read_wav_pcm16(os.path.join(out_dir, "slices", s.name), 32000, raw=True)
            assert np.array_equal(pcm, s.pcm.cpu().numpy())


def test_slice_batch_reads_wav_files(gpu, golden, inputs, tmp_path):
    """a PCM16 file at the slicer's rate is a recording too: the same slices as its samples give"""
    from scipy.io import wavfile

    x = (inputs["edge4"] * np.float32(30000)).astype(np.int16)
    path = str(tmp_path / "take.wav")
    wavfile.write(path, 32000, x)
    (ok_f, from_file), (ok_a, from_array) = SL.slice_batch(["take.wav", "take.wav"],
                                                           [path, x.astype(np.float32) * np.float32(1.0 / 32768.0)])
    assert ok_f and ok_a and len(from_file) == len(from_array) == 1
    assert from_file[0].name == from_array[0].name and torch.equal(from_file[0].pcm, from_array[0].pcm)
