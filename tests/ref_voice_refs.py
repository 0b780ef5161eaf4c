"""Reference of the ragged reference-clip spectrogram (include/evt.h: the batched `_get_ref_spec`), restated from its
definition; nothing here touches a GPU or the library's kernels.  tests/test_ref_voice_refs_cpu.py checks it against
torch.stft, tests/test_ref_spec_rows_gpu.py holds the kernel to it.

A clip of n live samples, hop h, pad = (2048 - h) // 2:
  frames      F = (n + 2 pad - 2048) // h + 1 when n > pad and n + 2 pad >= 2048, else 0
  peak        max |x| over the live samples, fp32
  normalise   x untouched for peak <= 1; x / peak for 1 < peak <= 2; x / 2 above -- ONE fp32 division per sample (the
              reference divides a float32 array by a float32 scalar), restated here in float32 because that rounding is part
              of the definition
  spectrum    float64 from there on, on the float32 samples converted exactly: reflect padding at the clip's own ends, Hann
              window, 2048-point DFT, sqrt(re^2 + im^2 + 1e-6) -- loss_refs.mel_ref's stages, whose float32 run gives the
              yardstick Y_X that loss_refs.tol_mag is tied to."""
import functools

import torch

import loss_refs as R

LENS = [705, 1280, 3000, 2049, 600, 0]          # the batch of tests/test_ref_spec_rows_gpu.py, in N = 3072
N = 3072
HOP = 640
PEAKS = [0.5, 1.5, 3.0, 2.0, 1.25, 0.0]         # untouched / divided by the peak / by 2 / exactly 2 / (too short) / (empty)


def frames(n, hop=HOP):
    pad = (R.NFFT - hop) // 2
    return (n + 2 * pad - R.NFFT) // hop + 1 if n > pad and n + 2 * pad >= R.NFFT else 0


def peak_of(x):
    """fp32 scalar tensor; 0 for an empty clip"""
    return x.abs().max() if x.numel() else torch.zeros((), dtype=torch.float32)


def normalise32(x):
    """x fp32 1-D -> fp32: the reference's `if maxx > 1: audio /= min(2, maxx)`, one float32 division per sample"""
    assert x.dtype == torch.float32
    pk = peak_of(x)
    if float(pk) > 1.0:
        return x / torch.minimum(pk, torch.tensor(2.0, dtype=torch.float32))
    return x.clone()


def spec_reference(x, hop=HOP, window=None):
    """x fp32 1-D (the live samples of one clip, at least pad + 1 of them) -> dict: mag float64 [1, F, 1025] and what
    loss_refs.tol_mag reads (norm, Y_X), v (the normalised fp32 clip), peak.  window: the fp32 Hann window the operator is
    handed (default: loss_refs.hann(); a caller whose window was computed elsewhere passes that one, the reference is of
    the operands as they are)"""
    v = normalise32(x)
    win = R.hann() if window is None else window.float().cpu()
    basis = torch.zeros(1, R.NBIN, dtype=torch.float32)          # the mel stages are not used
    r64 = R.mel_ref(v.double().unsqueeze(0), win, basis, hop, torch.float64)
    r32 = R.mel_ref(v.unsqueeze(0), win, basis, hop, torch.float32)
    ref = dict(mag=r64["mag"], X=r64["X"], norm=r64["xw"].norm(dim=-1), v=v, peak=peak_of(x))
    err = (r32["X"].to(torch.complex128) - r64["X"]).abs().amax(-1)
    live = ref["norm"] > 0
    ref["Y_X"] = float((err[live] / ref["norm"][live]).max()) if bool(live.any()) else 0.0
    return ref


def clip(n, peak, key):
    """n samples in [-peak, peak] with the peak attained exactly once, negative for every other clip"""
    if n == 0:
        return torch.zeros(0, dtype=torch.float32)
    x = (torch.rand(n, generator=R.gen("refclip", key, n), dtype=torch.float64) * 2 - 1) * 0.9 * peak
    x[(n * 7) // 11] = -peak if key % 2 else peak
    return x.float()


@functools.lru_cache(maxsize=None)
def batch():
    """(x [6, N] fp32 with NaN behind every row's length, the clips, per-row references (None for the rows without a
    frame)); computed once and shared: do not modify"""
    clips = [clip(n, p, k) for k, (n, p) in enumerate(zip(LENS, PEAKS))]
    x = torch.full((len(LENS), N), float("nan"), dtype=torch.float32)
    for s, c in enumerate(clips):
        x[s, :c.numel()] = c
    refs = [spec_reference(c) if frames(c.numel()) > 0 else None for c in clips]
    return x, clips, refs
