"""CPU: the float64 reference of the ragged reference-clip spectrogram (tests/ref_voice_refs.py) against torch.stft on each
row alone, its peak rule at the thresholds, and its frame count at the edges of the reflect padding."""
import pytest
import torch

import loss_refs as R
import ref_voice_refs as V


def _stft_mag(v, hop):
    """the reference's spectrogram_torch (module/mel_processing.py:40-74 of the reference) in float64 on one clip"""
    pad = (R.NFFT - hop) // 2
    y = torch.nn.functional.pad(v.double().view(1, 1, -1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, R.NFFT, hop_length=hop, win_length=R.NFFT, window=R.hann().double(), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    return torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-6).transpose(1, 2)          # [1, F, 1025]


def test_reference_equals_torch_stft_row_by_row():
    _x, clips, refs = V.batch()
    for s, (c, ref) in enumerate(zip(clips, refs)):
        if ref is None:
            assert V.frames(c.numel()) == 0 and V.LENS[s] in (600, 0)
            continue
        want = _stft_mag(V.normalise32(c), V.HOP)
        assert tuple(ref["mag"].shape) == tuple(want.shape) == (1, V.frames(c.numel()), R.NBIN), s
        err = float((ref["mag"] - want).abs().max())
        print(f"row {s}: n = {c.numel()}, frames {want.size(1)}, max |mag - stft| = {err:.3e}, Y_X = {ref['Y_X']:.2e}")
        assert err <= 1e-11 * max(1.0, float(want.max())), (s, err)
        assert 0 < ref["Y_X"] < 2e-6, ref["Y_X"]          # the fp32 yardstick is of fp32 size


@pytest.mark.parametrize("peak,div", [(0.5, None), (1.0, None), (1.5, 1.5), (2.0, 2.0), (3.0, 2.0)])
def test_peak_rule(peak, div):
    """untouched up to and including 1.0, divided by the peak up to 2, by 2 from there on; one fp32 division"""
    x = V.clip(1500, peak, 3)
    assert float(V.peak_of(x)) == peak
    got = V.normalise32(x)
    if div is None:
        assert torch.equal(got, x)
    else:
        want = (x.double() / div).float()                 # float64 quotient rounded once == the correctly rounded fp32 division
        assert torch.equal(got, want)
        assert float(got.abs().max()) == (1.0 if peak <= 2 else peak / 2)


@pytest.mark.parametrize("n,want", [(704, 0), (705, 1), (1279, 1), (1280, 2), (2047, 3), (2048, 3), (2049, 3)])
def test_frame_count(n, want):
    from easevoice_trainer_amd.hip.audio import ref_frames

    assert V.frames(n) == want == ref_frames(n, V.HOP)
    if n > 704:
        assert want == n // 640 == _stft_mag(torch.zeros(n), V.HOP).size(1)
    else:
        with pytest.raises(RuntimeError):                 # torch's reflect padding refuses pad >= n
            _stft_mag(torch.zeros(n), V.HOP)


def test_batch_covers_the_cases():
    x, clips, _refs = V.batch()
    assert [c.numel() for c in clips] == V.LENS and tuple(x.shape) == (6, V.N)
    for s, n in enumerate(V.LENS):
        assert bool(torch.isnan(x[s, n:]).all()) and bool(torch.isfinite(x[s, :n]).all())
        assert float(V.peak_of(clips[s])) == V.PEAKS[s]
    assert [V.frames(n) for n in V.LENS] == [1, 2, 4, 3, 0, 0] and V.frames(V.N) == 4
