"""GPU: evt_ref_spec_rows (csrc/stft_mel.hip) -- linear spectrograms of a ragged batch of reference clips, the C ABI called
directly, 256 sentinel floats on either side of both outputs.

The batch is tests/ref_voice_refs.py's: lens = [705, 1280, 3000, 2049, 600, 0] in N = 3072 with NaN behind every row's
length (a NaN in the output would mean the padding was read), peaks 0.5 / 1.5 / 3.0 / exactly 2.0.  Asserted, for 704 and
for 1025 bins:
  * row s is bit for bit the entry at nseq = 1 with another N;
  * row s is within loss_refs.tol_mag (the project's derived bound, unchanged) of the float64 reference;
  * row s against spectrogram_torch of that row alone after the same fp32 normalisation done in torch.  The two kernels share
    the source of fft2048, of the window product and of the magnitude, but they are NOT bit-identical and the shared code
    cannot be made so without changing evt_mel_fwd's own bits: fft2048 is inlined into both, evt_mel_fwd keeps re and im of
    every bin alive for its workspace while this kernel consumes them in the magnitude alone, and the compiler contracts the
    products and sums of the last butterfly stages differently for the two (device assembly: 256 against 278 v_pk_fma_f32,
    113 against 122 v_pk_mul_f32).  How many values differ and by how many ulp is printed.  Asserted instead, as the next
    bound: both are within tol_mag of the float64 reference, hence within 2 tol_mag of each other;
    MEASURED on an MI355X (no bound changed after the first run): 43-47 % of a row's values differ, by at most 95 ulp
    (in bins of small magnitude), 0.06-0.09 of 2 tol_mag; against the float64 reference the rows are at 0.15-0.26 of tol_mag;
  * the rows of 600 and 0 samples and every frame >= F_s are exact zeros; peak is exact;
  * every refusal returns EVT_EINVAL and leaves both outputs untouched."""
import ctypes as C

import pytest
import torch

import loss_refs as R
import ref_voice_refs as V

pytestmark = pytest.mark.gpu

G = 256
SENT = -7777.25
EINVAL = 22
FMAX = V.frames(V.N)


def _guarded(n, dev):
    buf = torch.full((n + 2 * G,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G:G + n]


def _intact(buf, name):
    assert bool((buf[:G] == SENT).all()) and bool((buf[-G:] == SENT).all()), f"{name}: a sentinel was overwritten"


def _win(dev):
    """the Hann window the project hands its STFT kernels (module/mel_processing.py keeps one per device, computed there):
    the bit-for-bit comparison with spectrogram_torch needs the same operand, and the float64 reference is taken of it"""
    from easevoice_trainer_amd.module.mel_processing import _window

    return _window(R.NFFT, torch.device(dev))


def _call(L, x, lens, bins, hop=V.HOP):
    """x [nseq, N] on the device -> (out [nseq, Fmax, bins], peak [nseq]) on the CPU; the sentinels are checked"""
    nseq, n = x.shape
    fmax = V.frames(n, hop)
    out_b, out = _guarded(nseq * fmax * bins, x.device)
    pk_b, pk = _guarded(nseq, x.device)
    lens_d = torch.tensor(lens, dtype=torch.int32).to(x.device)
    L.check(L.lib().evt_ref_spec_rows(L.ptr(x), L.ptr(lens_d), nseq, n, L.ptr(_win(x.device)), R.NFFT, hop, bins,
                                      L.ptr(out), L.ptr(pk), L.stream_ptr()), "evt_ref_spec_rows")
    torch.cuda.synchronize()
    _intact(out_b, "out")
    _intact(pk_b, "peak")
    return out.view(nseq, fmax, bins).cpu(), pk.cpu()


@pytest.fixture(scope="module")
def runs(gpu):
    from easevoice_trainer_amd.hip import lib as L

    x, _clips, _refs = V.batch()
    xd = x.to(gpu)
    return {bins: _call(L, xd, V.LENS, bins) for bins in (704, 1025)}


@pytest.mark.parametrize("bins", [704, 1025])
def test_rows_against_spectrogram_torch(gpu, runs, bins):
    from easevoice_trainer_amd.module.mel_processing import spectrogram_torch

    out, _pk = runs[bins]
    assert not bool(torch.isnan(out).any()), "a NaN from behind a row's length reached the output"
    _x, clips, _refs = V.batch()
    for s, c in enumerate(clips):
        f = V.frames(c.numel())
        if f == 0:
            continue
        want = spectrogram_torch(V.normalise32(c).unsqueeze(0).to(gpu), R.NFFT, R.SR, V.HOP, R.NFFT)     # [1, 1025, F]
        want = want[0].transpose(0, 1)[:, :bins].contiguous().cpu()
        assert tuple(want.shape) == (f, bins)
        got = out[s, :f].contiguous()
        ref = V.spec_reference(c, window=_win(gpu))
        tol = R.tol_mag(ref)[0, :, :bins]
        frac = float(((got.double() - want.double()).abs() / (2 * tol)).max())
        print(f"MEASURED row {s} bins {bins}: {int((got != want).sum())} of {got.numel()} values differ from spectrogram_torch, "
              f"at most {int(R.ulps_f32(got, want).max())} ulp; |d| / (2 tol_mag) = {frac:.3f}")
        assert float(((want.double() - ref["mag"][0, :, :bins]).abs() / tol).max()) <= 1.0, s
        assert frac <= 1.0, (s, frac)


@pytest.mark.parametrize("bins", [704, 1025])
def test_rows_equal_the_entry_alone_with_another_length(gpu, runs, bins):
    from easevoice_trainer_amd.hip import lib as L

    out, pk = runs[bins]
    _x, clips, _refs = V.batch()
    for s, c in enumerate(clips):
        f = V.frames(c.numel())
        if f == 0:
            continue
        n1 = c.numel() + (0 if s % 2 else 700)             # exactly the clip, or a longer buffer with poison behind it
        x1 = torch.full((1, n1), float("nan"), dtype=torch.float32)
        x1[0, :c.numel()] = c
        o1, p1 = _call(L, x1.to(gpu), [c.numel()], bins)
        assert torch.equal(o1[0, :f].view(torch.int32), out[s, :f].contiguous().view(torch.int32)), s
        assert bool((o1[0, f:] == 0).all()) and torch.equal(p1[0], pk[s])


@pytest.mark.parametrize("bins", [704, 1025])
def test_rows_meet_the_float64_reference(gpu, runs, bins):
    out, _pk = runs[bins]
    _x, clips, refs = V.batch()
    win = _win(gpu).cpu()
    print(f"window: {int((win != R.hann()).sum())} of {R.NFFT} values differ from the host's torch.hann_window")
    for s, ref in enumerate(refs):
        if ref is None:
            continue
        ref = V.spec_reference(clips[s], window=win)
        f = ref["mag"].size(1)
        err = (out[s, :f].double() - ref["mag"][0, :, :bins]).abs()
        tol = R.tol_mag(ref)[0, :, :bins]
        frac = float((err / tol).max())
        print(f"MEASURED row {s} bins {bins}: error / tol_mag = {frac:.3f}")
        assert frac <= 1.0, (s, frac)


@pytest.mark.parametrize("bins", [704, 1025])
def test_dead_rows_and_frames_are_exact_zeros_and_peak_is_exact(runs, bins):
    out, pk = runs[bins]
    _x, clips, _refs = V.batch()
    for s, c in enumerate(clips):
        f = V.frames(c.numel())
        assert bool((out[s, f:].contiguous().view(torch.int32) == 0).all()), f"row {s}: frames >= {f} are not exact zeros"
        assert float(pk[s]) == float(V.peak_of(c)) == V.PEAKS[s], s
    assert V.frames(600) == 0 and V.frames(0) == 0


def test_python_wrapper(gpu, runs):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.audio import ref_spec_rows

    x, _clips, _refs = V.batch()
    live = [0, 1, 2, 3]
    spec, frames, peak = ref_spec_rows(x[live].contiguous().to(gpu), [V.LENS[s] for s in live])
    assert tuple(spec.shape) == (4, FMAX, 704) and frames == [1, 2, 4, 3]
    assert torch.equal(spec.cpu(), runs[704][0][live]) and torch.equal(peak.cpu(), runs[704][1][live])
    with pytest.raises(L.EvtError):                         # a row of at most pad samples: torch's reflect padding refuses it
        ref_spec_rows(x.to(gpu), V.LENS)
    with pytest.raises(L.EvtError):
        ref_spec_rows(x[:1].contiguous().to(gpu), [704])


def test_refusals_leave_the_outputs_untouched(gpu):
    from easevoice_trainer_amd.hip import lib as L

    lib, nseq, n = L.lib(), 2, 3072
    x = torch.zeros(nseq, n, device=gpu)
    lens = torch.tensor([n, n], dtype=torch.int32).to(gpu)
    win = R.hann().to(gpu)
    out = torch.full((1 << 16,), SENT, device=gpu)          # more than an accepted call of these shapes would write
    pk = torch.full((64,), SENT, device=gpu)
    null = C.c_void_p(0)
    ok = dict(x=L.ptr(x), lens=L.ptr(lens), nseq=nseq, N=n, window=L.ptr(win), n_fft=2048, hop=640, bins=704, out=L.ptr(out),
              peak=L.ptr(pk))
    bad = [dict(x=null), dict(lens=null), dict(window=null), dict(out=null), dict(peak=null), dict(nseq=0), dict(nseq=-1),
           dict(nseq=65536), dict(N=0), dict(N=-5), dict(n_fft=1024), dict(n_fft=4096), dict(hop=0), dict(hop=-640),
           dict(hop=2049), dict(bins=0), dict(bins=1026), dict(out=C.c_void_p(out.data_ptr() + 4))]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.evt_ref_spec_rows(a["x"], a["lens"], a["nseq"], a["N"], a["window"], a["n_fft"], a["hop"], a["bins"],
                                   a["out"], a["peak"], L.stream_ptr())
        assert rc == EINVAL, (change, rc)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((pk == SENT).all()), "an output was written by a refused call"
