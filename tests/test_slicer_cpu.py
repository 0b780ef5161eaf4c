"""The slicer's host side (audiokit/slicer.py) against the reference's recorded behaviour (tests/golden/slicer.json, made by
tests/golden/make_golden_slicer.py): derived parameters, the tag walk on silent runs fed the golden RMS frames, file names,
argument errors -- and the summation recipe that csrc/slicer.hip implements, emulated in float32, against the golden bits.
Every comparison is exact."""
import json
import os

import numpy as np
import pytest

import slicer_inputs as I
from easevoice_trainer_amd.audiokit import slicer as SL

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "slicer.json")) as f:
        return json.load(f)


def cases(golden):
    return [("A", golden["A"]), ("B", golden["B"]), ("C", golden["C"])] + [(f"edge{k}", g) for k, g in
                                                                          enumerate(golden["edges"])]


def rms_of(g):
    return np.array(g["rms"], dtype=np.uint32).view(np.float32)


def test_params_match_the_reference(golden):
    for name, g in cases(golden):
        p, d = SL.SlicerParams(**g["params"]), g["derived"]
        assert (p.hop, p.win, p.min_length_frames, p.min_interval_frames, p.max_sil_kept_frames, p.threshold_lin) == (
            d["hop"], d["win"], d["min_length"], d["min_interval"], d["max_sil_kept"], d["threshold"]), name
    assert SL.SlicerParams(**I.PARAMS_B).win == 640 and SL.SlicerParams(**I.PARAMS_C).win == 1323


def test_params_value_errors():
    with pytest.raises(ValueError, match="min_length >= min_interval >= hop_size"):
        SL.SlicerParams(min_length=200, min_interval=300)
    with pytest.raises(ValueError, match="min_length >= min_interval >= hop_size"):
        SL.SlicerParams(min_interval=5, hop_size=10)
    with pytest.raises(ValueError, match="max_sil_kept >= hop_size"):
        SL.SlicerParams(max_sil_kept=5)


def test_tag_walk_reproduces_every_label(golden):
    seen = 0
    for name, g in cases(golden):
        if "chunks" not in g:
            continue
        p, rms = SL.SlicerParams(**g["params"]), rms_of(g)
        assert p.too_short(g["n"]) == (not g["sliced"]), name
        if not g["sliced"]:
            continue
        assert rms.shape[0] == (g["n"] + 2 * (p.win // 2) - p.win) // p.hop + 1
        spans = SL.chunk_spans(SL.silence_tags(rms, p), g["n"], rms.shape[0], p.hop)
        assert [(s, e, n) for s, e, _, n in spans] == [(c["start"], c["end"], c["n"]) for c in g["chunks"]], name
        assert all(b == s for s, _, b, _ in spans)
        seen += len(spans)
    assert seen == 5 + 3 + 1          # A, B and the 3 s recording without silence


def test_the_inputs_reach_every_branch(golden):
    """case A drives the walk through the leading tag, the three silence-length branches and the trailing tag"""
    g = golden["A"]
    p, rms = SL.SlicerParams(**g["params"]), rms_of(g)
    tags = SL.silence_tags(rms, p)
    assert tags[0][0] == 0 and tags[-1][1] == rms.shape[0] + 1
    silent = np.concatenate(([False], rms < np.float32(p.threshold_lin), [False]))
    edge = np.flatnonzero(silent[1:] != silent[:-1])
    runs = [(int(b), int(e - b)) for b, e in zip(edge[::2], edge[1::2])]        # (first frame, length) of every silent run
    keep = p.max_sil_kept_frames
    cut = [n for b, n in runs if any(b <= t[0] <= b + n for t in tags[1:-1])]
    assert any(n <= keep for n in cut) and any(keep < n <= 2 * keep for n in cut) and any(n > 2 * keep for n in cut), runs
    assert len(runs) > len(tags)      # the silence behind the clip that is too short is not cut
    zeros = np.flatnonzero(rms == 0)
    assert zeros.size > 1 and any(t == (int(zeros[0]), int(zeros[0])) for t in tags)   # argmin ties: the first zero wins
    assert SL.chunk_spans([], 1000, 4, 320) == [(0, 1280, 0, 1000)]
    # the end label may exceed the sample count, the chunk is clipped
    assert SL.chunk_spans([(2, 2), (5, 9)], 1500, 8, 320) == [(0, 640, 0, 640), (640, 1600, 640, 860)]


def test_file_names():
    assert SL.slice_name("take.reformatted.wav", 12800, 192000) == "take_0000012800_0000192000.wav"
    assert SL.slice_name("/some/dir/voice.wav", 0, 5) == "voice_0000000000_0000000005.wav"
    assert SL.slice_name("plain", 1, 2) == "plain_0000000001_0000000002.wav"


def test_slice_batch_argument_errors():
    x = np.zeros(8, dtype=np.float32)
    assert SL.slice_batch([], []) == []
    with pytest.raises(ValueError, match="2 names for 1 recordings"):
        SL.slice_batch(["a", "b"], [x])
    with pytest.raises(ValueError, match="1-D float32"):
        SL.slice_batch(["a"], [x.astype(np.float64)])
    with pytest.raises(ValueError, match="1-D float32"):
        SL.slice_batch(["a"], [x.reshape(2, 4)])
    with pytest.raises(ValueError, match="1-D float32"):
        SL.slice_batch(["a"], [list(x)])
    with pytest.raises(ValueError, match="one per recording"):
        SL.slice_batch(["a"], [x], params=[SL.SlicerParams(), SL.SlicerParams()])
    with pytest.raises(ValueError, match="32000"):
        SL.slice_batch(["a"], [x], params=SL.SlicerParams(**I.PARAMS_C))
    # nothing to slice: no device is touched
    assert SL.slice_batch(["a"], [np.zeros(0, dtype=np.float32)], device="cuda:99") == [(False, [])]


def test_summation_recipe_equals_the_reference_bits(golden):
    """the order of additions the kernel is written to (a float32 emulation of it) gives the reference's frames bit for bit"""
    inputs = {"B": I.case_b(), "C": I.case_c()}
    inputs.update({f"edge{k}": x for k, x in enumerate(I.edges())})
    for name, g in cases(golden):
        if name not in inputs or g["n"] > 101000:
            continue
        p = SL.SlicerParams(**g["params"])
        got = I.emulate_rms(inputs[name], p.win, p.hop)
        assert got.dtype == np.float32 and got.view(np.uint32).tolist() == g["rms"], name
