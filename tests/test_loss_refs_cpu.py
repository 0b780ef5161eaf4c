"""CPU: the conditions the references and inputs of tests/loss_refs.py rest on (no GPU, no kernel).

* mel_ref in float64 is the reference project's formula (mel_processing.py:93-142): F.pad(reflect) -> torch.stft(hann,
  center=False) -> sqrt(re^2 + im^2 + 1e-6) -> mel_basis @ -> log(clamp(., 1e-5)), written out here with torch ops.
* no pre-log mel entry lies within a factor 2 of the clamp threshold -- except in the two runs of loss_refs.NEAR_CLAMP_RUNS
  (512 mel bins, quiet and zero waveform), where every entry still keeps 32 pre-log tolerances from it -- so that which
  side an entry is on never depends on rounding; the clamp case has entries on both sides; the all-zero rows of the
  512-bin filterbank are found and are clamped.
* every segment size list sums to fewer than 2^24 units, so that fp32 accumulation is exact in any order.
* the fp32 yardsticks Y_X and Y_b are printed per case (pytest -s); tests/test_mel_gpu.py's docstring records them.
"""
import pytest
import torch
import torch.nn.functional as F

import loss_refs as R

MEL_RUNS = [(c, w, "real") for c in R.MEL_CASES for w in R.WAVES] + [(R.CLAMP_CASE, "quiet", "clamp"),
                                                                       (R.ONEHOT_CASE, "randn", "onehot")]
MEL_IDS = [f"{R.case_id(c)}-{w}-{b}" for c, w, b in MEL_RUNS]


def _reference_formula(wav, basis, hop):
    """the reference project's mel_spectrogram_torch, float64"""
    pad = (R.NFFT - hop) // 2
    y = F.pad(wav.double().unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, R.NFFT, hop_length=hop, win_length=R.NFFT, window=R.hann().double(), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-6)
    p = torch.matmul(basis.double(), mag)
    return spec, mag, p, torch.log(torch.clamp(p, min=1e-5))


@pytest.mark.parametrize("case,wave,kind", MEL_RUNS, ids=MEL_IDS)
def test_mel_ref_is_the_reference_formula(case, wave, kind):
    ref = R.mel_case_reference(case, wave, kind)
    spec, mag, p, mel = _reference_formula(ref["wav"], ref["basis"], case[2])
    _, frames = R.geometry(case[1], case[2])
    assert tuple(ref["mel"].shape) == (case[0], frames, case[3])
    scale = float(ref["norm"].max())
    # two float64 evaluations of one formula: different FFT plans / summation orders, 1e-12 relative at the most
    assert float((ref["X"].transpose(1, 2) - spec).abs().max()) <= 1e-12 * max(scale, 1.0)
    assert torch.allclose(ref["mag"].transpose(1, 2), mag, rtol=1e-11, atol=0)
    assert torch.allclose(ref["p"].transpose(1, 2), p, rtol=1e-11, atol=1e-300)
    assert torch.allclose(ref["mel"].transpose(1, 2), mel, rtol=0, atol=1e-10)


@pytest.mark.parametrize("case,wave,kind", MEL_RUNS, ids=MEL_IDS)
def test_no_entry_near_the_clamp_and_yardsticks(case, wave, kind):
    ref = R.mel_case_reference(case, wave, kind)
    live, clamped, undecided = R.clamp_sets(ref)
    assert not bool(undecided.any()), f"{int(undecided.sum())} entries within {R.CLAMP_MARGIN} tolerances of 1e-5"
    near = R.near_clamp(ref)
    if (case, wave, kind) in R.NEAR_CLAMP_RUNS:
        gap = ((ref["p"] - R.CLAMP).abs() / R.tol_p(ref).clamp(min=1e-300))[near].min()
        print(f"\nNEAR CLAMP {R.case_id(case)} {wave}: {int(near.sum())} of {near.numel()} entries within a factor 2, the "
              f"closest {float(gap):.0f} pre-log tolerances from 1e-5")
        assert bool(near.any())
    else:
        assert not bool(near.any()), f"{int(near.sum())} entries within a factor 2 of 1e-5"
    print(f"\nYARDSTICK {R.case_id(case)} {wave} {kind}: Y_X = {ref['Y_X']:.3e}  Y_b = {ref['Y_b']:.3e}  "
          f"clamped = {int(clamped.sum())} of {clamped.numel()}")
    # a float32 evaluation has to be an fp32-sized distance from the float64 one, or the yardstick measures something else
    assert ref["Y_X"] < 64 * R.U
    if kind != "onehot":        # (the one-hot basis serves the forward's exact assertions alone: 1 / p of single bins is
        assert ref["Y_b"] < 1e-5    # ill-conditioned, fp32 autograd itself is 4e-5 off there)
    if wave == "zero":
        assert ref["Y_X"] == 0.0 and ref["Y_b"] == 0.0 and float(ref["dwav"].abs().max()) == 0.0
    else:
        assert ref["Y_X"] > 0.0 and ref["Y_b"] > 0.0
    if kind == "real" and case[3] <= 129:
        assert not bool(clamped.any())      # the real filterbank never reaches the clamp at the model's size


def test_clamp_case_has_both_sides():
    ref = R.mel_case_reference(R.CLAMP_CASE, "quiet", "clamp")
    live, clamped, _ = R.clamp_sets(ref)
    rows = torch.zeros(R.CLAMP_CASE[3], dtype=torch.bool)
    rows[1::4] = True
    assert bool(clamped[..., rows].all()) and bool(live[..., ~rows].all())
    assert int(clamped.sum()) > 0 and int(live.sum()) > 0
    for seed in (0, 1):
        p = R.mel_case_reference(R.CLAMP_CASE, "quiet", "clamp", seed)["p"]
        print(f"\nCLAMP CASE seed {seed}: scaled rows p <= {float(p[..., rows].max()) / R.CLAMP:.3g} x 1e-5, "
              f"others p >= {float(p[..., ~rows].min()) / R.CLAMP:.3g} x 1e-5")
        assert float(p[..., rows].max()) < 0.5 * R.CLAMP and float(p[..., ~rows].min()) > 2 * R.CLAMP


def test_zero_rows_of_the_512_bin_filterbank_are_clamped():
    b = R.real_basis(512)
    zero_rows = (b == 0).all(1)
    assert int(zero_rows.sum()) > 0
    print(f"\n512-bin filterbank: {int(zero_rows.sum())} all-zero rows: {torch.nonzero(zero_rows).flatten().tolist()}")
    for wave in R.WAVES:
        ref = R.mel_case_reference((2, 2500, 320, 512), wave)
        _, clamped, _ = R.clamp_sets(ref)
        assert bool(clamped[..., zero_rows].all()) and float(ref["p"][..., zero_rows].abs().max()) == 0.0


def test_onehot_basis_covers_the_ends_and_both_parities():
    bins = R.onehot_bins(512)
    for k in R.ONEHOT_FIXED:
        assert int((bins == k).sum()) >= 1
    assert int((bins % 2 == 0).sum()) > 100 and int((bins % 2 == 1).sum()) > 100
    b = R.onehot_basis(512)
    assert torch.equal(b.sum(1), torch.ones(512)) and int((b != 0).sum()) == 512
    assert 0 <= int(bins.min()) and int(bins.max()) == R.NBIN - 1


@pytest.mark.parametrize("name", list(R.SEG_LISTS))
def test_segment_sums_stay_below_2_24_units(name):
    spec = R.SEG_LISTS[name]
    a_list, b_list = R.seg_operands(name)
    for t in a_list + b_list:
        k = t / 0.125
        assert torch.equal(k, k.round()) and float(t.abs().max()) <= 2.0      # multiples of 1/8 in +-2: exact in bfloat16
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    for sc in spec["scales"] + (R.SEG_DLOSS,):
        m, _ = torch.frexp(torch.tensor(sc))
        assert float(m) == 0.5                                                  # a power of two
    for mode, target in [(0, 0.0)] + [(1, t) for t in R.SEG_TARGETS]:
        count, unit = R.seg_units(name, mode, target)
        print(f"\nSEG {name} mode {mode} target {target}: {count} units of {unit} (2^24 = {R.F32_EXACT})")
        assert 0 < count < R.F32_EXACT
    # a == b planted on purpose in head, body and tail elements of the kernel's split, for both vector widths
    planted = R.seg_planted(spec["sizes"])
    for a, b, pos in zip(a_list, b_list, planted):
        assert bool((a == b)[pos].all())
    for V in R.SEG_VS:
        kinds = R.seg_partition(spec["sizes"], V)
        found = [sum(int((k[pos] == which).sum()) for k, pos in zip(kinds, planted)) for which in (0, 1, 2)]
        print(f"\nSEG {name} V = {V}: planted a == b in {found[0]} head, {found[1]} body, {found[2]} tail elements "
              f"(of {sum(int((k == 0).sum()) for k in kinds)} head elements in all)")
        assert min(found) >= 1, found


def test_segment_lists_reach_what_they_are_for():
    cuts = R.SEG_LISTS["cuts"]["sizes"]
    assert sum(cuts) == 22613
    starts = [sum(cuts[:i]) for i in range(len(cuts))]
    # a 2048-chunk boundary falls inside a segment at an offset that is no multiple of 4 (fp32) or 8 (16-bit) elements
    offs = [c - s for c in range(2048, 22613, 2048) for s, n in zip(starts, cuts) if s < c < s + n]
    assert len(offs) == 11 and any(o % 8 for o in offs) and any(o % 4 for o in offs)
    assert len(R.SEG_LISTS["many"]["sizes"]) == 64
    assert sum(R.SEG_LISTS["big"]["sizes"]) > 512 * 2048
