"""No GPU: the conditions the GPU tests of evt_semantic_codes_rows (tests/test_semantic_rows_gpu.py) rest on, checked on
every frame of every case of tests/semantic_refs.py.  Conditions, not measurements:
  * integer-exact inputs: every intermediate of the formula is an integer whose partial sums stay below 2^24 in any order,
    and at least a tenth of the frames are exact ties (some between copies of one vector, some between two different ones);
  * planted and close-pair inputs: every frame's margin is at least 2 E (semantic_refs' forward bound, which already
    counts the error of both distances compared): any fp32 evaluation has one possible answer;
  * an fp32 torch composition of the reference's formula gives the oracle's codes on all of those;
  * the oracle's codes are the codes the reference's own quantizer gives (tests/golden/semantic_rows.pt).

Measured here at D = 768, K = 1024 (162 codes per case): planted E 11 .. 15, margin 1089 .. 1500; close pairs (delta = 0.05) E
about 6, margin 68 .. 77; unplanted E about 12, median margin 17, 70 % of the frames below 2 E."""
import os

import pytest
import torch
import torch.nn.functional as F

import semantic_refs as R

CASES = [(name, D, K) for name in ("exact", "planted", "close") for D, K in R.SHAPES]
_cache = {}


def case(name, D, K):
    key = (name, D, K)
    if key not in _cache:
        inp = R.GENERATORS[name](D, K)
        _cache[key] = (inp, R.oracle(inp["x"], inp["frames"], inp["w"], inp["bias"], inp["embed"]))
    return _cache[key]


@pytest.mark.parametrize("D,K", R.SHAPES)
def test_exact_inputs_are_integers_below_2_24_with_ties(D, K):
    inp, ora = case("exact", D, K)
    w, bias, embed = inp["w"].double(), inp["bias"].double(), inp["embed"].double()
    for t in (w, bias, embed):
        assert torch.equal(t, t.round())
    ties = frames = zero_ties = dup_ties = 0
    for b, n in enumerate(inp["frames"]):
        x = inp["x"][b, :n].double()
        assert torch.isfinite(x).all() and torch.equal(x, x.round())
        assert torch.isnan(inp["x"][b, n:]).all()                      # the padding is NaN: reading it would show
        if n < 2:
            continue
        xin = x[: n // 2 * 2].t().unsqueeze(0)
        h = F.conv1d(xin, w, bias, stride=2)[0].t()
        habs = F.conv1d(xin.abs(), w.abs(), bias.abs(), stride=2)[0].t()       # bounds every partial sum of the projection
        xx, ee, dabs = (h * h).sum(1), (embed * embed).sum(1), h.abs() @ embed.abs().t()
        assert torch.equal(h, h.round())
        assert habs.max() < 2 ** 24 and xx.max() < 2 ** 24 and ee.max() < 2 ** 24 and dabs.max() < 2 ** 24
        assert (xx[:, None] + 2 * dabs + ee[None]).max() < 2 ** 24
        o = ora[b]
        tie = o["margin"] == 0
        frames += n // 2
        ties += int(tie.sum())
        for t in torch.nonzero(tie).flatten().tolist():
            at = torch.nonzero(o["dist"][t] == o["dist"][t].min()).flatten()
            assert int(o["codes"][t]) == int(at[0])                    # the lower index
            same = torch.equal(embed[at[0]], embed[at[1]])
            dup_ties += int(same)
            zero_ties += int(not same)
    assert ties * 10 >= frames
    assert dup_ties > 0 and zero_ties > 0


@pytest.mark.parametrize("name,D,K", [c for c in CASES if c[0] != "exact"])
def test_planted_margins_are_decisive(name, D, K):
    _inp, ora = case(name, D, K)
    for o in ora:
        assert (o["margin"] >= 2 * o["E"]).all(), (float(o["margin"].min()), float(o["E"].max()))


@pytest.mark.parametrize("name,D,K", CASES)
def test_fp32_composition_gives_the_oracle_codes(name, D, K):
    inp, ora = case(name, D, K)
    got = R.fp32_codes(inp["x"], inp["frames"], inp["w"], inp["bias"], inp["embed"])
    for g, o, t in zip(got, ora, inp["frames"]):
        assert g.numel() == t // 2 and torch.equal(g, o["codes"])


def test_unplanted_margins_are_not_decisive():
    """why exact agreement is asked on planted inputs only: on random inputs a good part of the frames has a margin below E"""
    inp = R.unplanted_inputs(768, 1024)
    ora = R.oracle(inp["x"], inp["frames"], inp["w"], inp["bias"], inp["embed"])
    margin, E = torch.cat([o["margin"] for o in ora]), torch.cat([o["E"] for o in ora])
    assert (margin < E).float().mean() > 0.1


def test_oracle_matches_the_reference_quantizer():
    gold = torch.load(os.path.join(os.path.dirname(__file__), "golden", "semantic_rows.pt"))
    assert len(gold) == 2 * len(R.SHAPES)
    for key, rec in gold.items():
        name, D, K = key.rsplit("_", 2)
        inp, ora = case(name, int(D), int(K))
        assert R.checksum(inp) == rec["sha256"], f"{key}: the seeded inputs changed, regenerate the fixture"
        assert torch.equal(torch.cat([o["codes"] for o in ora]), rec["codes"].to(torch.int64))
