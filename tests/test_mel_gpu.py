"""GPU: evt_mel_fwd / evt_mel_bwd (csrc/stft_mel.hip) stage by stage against the float64 reference of tests/loss_refs.py.

The C ABI is called directly, so that the workspace (re, im and the pre-log mel of every frame) is visible; every buffer
the kernels write has 256 sentinel floats on either side.  u = 2^-24; ||xw|| is a frame's windowed 2-norm (float64).

Tolerances -- each derived, or tied to an fp32 evaluation of the REFERENCE on the CPU (loss_refs.mel_reference), never to
what the kernel gives:
  Y_X       max |rfft32(xw32) - X64| / ||xw||: what torch.fft.rfft in float32 loses on the float32 products
  spectrum  |dX_k| <= tolX = max(4 Y_X, 22 u) ||xw||.  4: fp32 sincospif twiddles and a radix-2 schedule against pocketfft's
            split radix (a float32 radix-2 run in numpy matched pocketfft within 10 %); 22 u: two roundings per stage over
            11 stages, the floor for inputs where Y_X is nearly 0
  magnitude |dmag| <= tolX + 4 u mag64   (the square root is 1-Lipschitz in |X|)
  pre-log   |dp_m| <= tolX sum_k b_mk + 517 u p64   (513 sequential non-negative terms, one shuffle add, mag's rounding)
  log-mel   live entries: tol_p / p64 + 4 u max(1, |log p64|); clamped entries: bit-identical to each other and within
            2 fp32 ulp of log(1e-5)
  backward  ||dwav - dwav64||_inf <= max(8 Y_b, 64 u) ||dwav64||_inf, Y_b the same ratio for float32 CPU autograd through
            mel_ref.  8: a second fp32 FFT, fp32 1/p and 1/mag recomputed from the stored re / im, up to about 8 unordered
            atomic adds per sample
What can be exact is asserted exactly: the zero waveform (re = im = 0, one magnitude constant, dwav = 0), the one-hot
basis (the stored pre-log value IS the magnitude of its bin, bit for bit), clamped entries (they contribute nothing).

The fp32 yardsticks printed by tests/test_loss_refs_cpu.py (CPU, left) next to what the kernels measured on an MI355X
(right: the largest error of each stage as a fraction of ITS bound above; no bound was changed after the first GPU run):
  run                               Y_X      Y_b |    re    im   mag     p   mel  dwav
  1x705x640x128 randn           3.8e-07  3.1e-07 |  0.24  0.24  0.25  0.01  0.01  0.08
  1x705x640x128 quiet           4.0e-07  2.0e-07 |  0.23  0.26  0.19  0.01  0.04  0.06
  1x705x640x128 zero            0.0e+00  0.0e+00 |  0.00  0.00  0.20  0.01  0.04  0.00
  2x1985x641x129 randn          4.0e-07  4.7e-07 |  0.21  0.22  0.20  0.01  0.02  0.07
  2x1985x641x129 quiet          3.9e-07  1.8e-07 |  0.23  0.20  0.20  0.01  0.04  0.05
  2x1985x641x129 zero           0.0e+00  0.0e+00 |  0.00  0.00  0.20  0.01  0.04  0.00
  3x3000x640x128 randn          4.3e-07  3.3e-07 |  0.19  0.21  0.19  0.01  0.01  0.05
  3x3000x640x128 quiet          4.4e-07  1.9e-07 |  0.23  0.22  0.21  0.01  0.04  0.04
  3x3000x640x128 zero           0.0e+00  0.0e+00 |  0.00  0.00  0.20  0.01  0.04  0.00
  1x4096x2048x1 randn           3.8e-07  2.7e-07 |  0.23  0.25  0.19  0.01  0.01  0.08
  1x4096x2048x1 quiet           4.3e-07  1.4e-07 |  0.21  0.26  0.23  0.02  0.01  0.18
  1x4096x2048x1 zero            0.0e+00  0.0e+00 |  0.00  0.00  0.20  0.00  0.01  0.00
  2x2500x320x512 randn          5.0e-07  9.6e-07 |  0.23  0.20  0.18  0.05  0.05  0.13
  2x2500x320x512 quiet          4.3e-07  2.1e-07 |  0.24  0.18  0.20  0.01  0.05  0.06
  2x2500x320x512 zero           0.0e+00  0.0e+00 |  0.00  0.00  0.20  0.01  0.04  0.00
  2x20480x640x128 randn         5.5e-07  3.6e-07 |  0.24  0.22  0.27  0.01  0.02  0.12
  2x20480x640x128 quiet         5.1e-07  2.2e-07 |  0.23  0.23  0.20  0.01  0.05  0.06
  2x20480x640x128 zero          0.0e+00  0.0e+00 |  0.00  0.00  0.20  0.01  0.04  0.00
  the same, clamp basis         3.9e-07  2.0e-07 |  0.23  0.20  0.20  0.01  0.04  0.05
The spectrum sits at a quarter of its bound (the kernel's FFT is about as accurate as pocketfft's: the factor 4 is not
used up), the pre-log mel and the log-mel at 1 to 5 %, the backward at 4 to 18 %.  Zero waveform: re, im and dwav are
exact zeros; its magnitude is sqrtf(1e-6f) against the float64 sqrt(1e-6) (0.2 of 4 u).
"""
import ctypes as C

import pytest
import torch

import loss_refs as R

pytestmark = pytest.mark.gpu

G = 256                 # sentinel floats on either side of every written buffer
SENT = -7777.25
EINVAL, ENOTSUP = 22, 95


def _guarded(n, dev):
    buf = torch.full((n + 2 * G,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G:G + n]


def _guards_intact(buf, name):
    assert bool((buf[:G] == SENT).all()) and bool((buf[-G:] == SENT).all()), f"{name}: a sentinel was overwritten"


def _run(L, dev, case, wav, basis, dmel=None, want_spec=True):
    """evt_mel_fwd (+ evt_mel_bwd) on guarded buffers -> dict of CPU tensors in the reference's [nseq, frames, ...] layout"""
    nseq, wav_len, hop, n_mels = case
    _, frames = R.geometry(wav_len, hop)
    lib = L.lib()
    nws = lib.evt_mel_workspace_floats(nseq, wav_len, R.NFFT, hop, n_mels)
    assert nws == nseq * frames * (2 * R.NBIN + n_mels)
    dims = (C.c_int64 * 5)(nseq, wav_len, R.NFFT, hop, n_mels)
    assert lib.evt_workspace_bytes(1, dims, 5) == 4 * nws                     # EVT_WS_MEL
    wav_d, win_d, basis_d = wav.to(dev).contiguous(), R.hann().to(dev), basis.to(dev).contiguous()
    ws_b, ws = _guarded(nws, dev)
    mel_b, mel = _guarded(nseq * n_mels * frames, dev)
    spec_b, spec = _guarded(nseq * R.NBIN * frames, dev)
    L.check(lib.evt_mel_fwd(L.ptr(wav_d), L.ptr(win_d), L.ptr(basis_d), L.ptr(spec) if want_spec else C.c_void_p(0),
                            L.ptr(mel), L.ptr(ws), nseq, wav_len, R.NFFT, hop, n_mels, L.stream_ptr()), "evt_mel_fwd")
    torch.cuda.synchronize()
    for b, nm in ((ws_b, "ws"), (mel_b, "mel"), (spec_b, "spec")):
        _guards_intact(b, nm)
    if not want_spec:
        assert bool((spec == SENT).all())
    wsf = ws.view(nseq, frames, 2 * R.NBIN + n_mels).cpu()
    out = dict(re=wsf[..., :R.NBIN], im=wsf[..., R.NBIN:2 * R.NBIN], p=wsf[..., 2 * R.NBIN:],
               mag=spec.view(nseq, R.NBIN, frames).transpose(1, 2).cpu(),
               mel=mel.view(nseq, n_mels, frames).transpose(1, 2).cpu())
    if dmel is not None:
        dmel_d = dmel.transpose(1, 2).contiguous().to(dev)                      # the kernel's [seq][mel][frame]
        dw_b, dw = _guarded(nseq * wav_len, dev)
        L.check(lib.evt_mel_bwd(L.ptr(dmel_d), L.ptr(win_d), L.ptr(basis_d), L.ptr(ws), L.ptr(dw), nseq, wav_len, R.NFFT,
                                hop, n_mels, L.stream_ptr()), "evt_mel_bwd")
        torch.cuda.synchronize()
        _guards_intact(dw_b, "dwav")
        _guards_intact(ws_b, "ws after the backward")
        out["dwav"] = dw.view(nseq, wav_len).cpu()
    return out


def _ratio(err, tol):
    """max of err / tol where tol > 0; where tol == 0 the error has to be 0 too"""
    err, tol = err.double(), torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    zero = tol == 0
    assert float(err[zero].max() if bool(zero.any()) else 0.0) == 0.0
    return float((err[~zero] / tol[~zero]).max()) if bool((~zero).any()) else 0.0


def _check_stages(got, ref, tag):
    """every stage against its own bound; returns the measured error / bound per stage"""
    m = {}
    tx = R.tol_X(ref)
    m["re"] = _ratio((got["re"].double() - ref["X"].real).abs(), tx)
    m["im"] = _ratio((got["im"].double() - ref["X"].imag).abs(), tx)
    m["mag"] = _ratio((got["mag"].double() - ref["mag"]).abs(), R.tol_mag(ref))
    m["p"] = _ratio((got["p"].double() - ref["p"]).abs(), R.tol_p(ref))
    live, clamped, undecided = R.clamp_sets(ref)
    assert not bool(undecided.any())
    err_mel = (got["mel"].double() - ref["mel"]).abs()
    m["mel"] = _ratio(err_mel[live], R.tol_mel_live(ref)[live]) if bool(live.any()) else 0.0
    if bool(clamped.any()):
        cl = got["mel"][clamped]
        assert bool((cl.view(torch.int32) == cl.view(torch.int32)[0]).all()), f"{tag}: clamped entries differ in bits"
        want = torch.full_like(cl[:1], float(R.log_clamp_f32()))
        assert int(R.ulps_f32(cl[:1], want)) <= 2, f"{tag}: clamped log-mel {float(cl[0])!r}"
    if "dwav" in got:
        m["dwav"] = _ratio((got["dwav"].double() - ref["dwav"]).abs().max().reshape(1), R.tol_dwav(ref))
    print(f"\nMEASURED {tag}: " + "  ".join(f"{k} {v:.3f}" for k, v in m.items()) + "  (error / bound, max)")
    for k, v in m.items():
        assert v <= 1.0, f"{tag}: stage {k} is at {v:.3f} of its bound {m}"
    return m


@pytest.mark.parametrize("wave", R.WAVES)
@pytest.mark.parametrize("case", R.MEL_CASES, ids=R.case_id)
def test_mel_stages_against_float64(gpu, case, wave):
    from easevoice_trainer_amd.hip import lib as L

    ref = R.mel_case_reference(case, wave)
    got = _run(L, gpu, case, ref["wav"], ref["basis"], ref["dmel"])
    _check_stages(got, ref, f"{R.case_id(case)} {wave}")
    if wave == "zero":
        bits = got["mag"].contiguous().view(torch.int32)
        assert bool((bits == bits.flatten()[0]).all()), "the magnitude of silence is not one constant"
        want = torch.sqrt(torch.tensor([1e-6], dtype=torch.float64)).float()
        assert int(R.ulps_f32(got["mag"].flatten()[:1], want)) <= 1
        assert bool((got["re"] == 0).all()) and bool((got["im"] == 0).all())
        assert bool((got["dwav"] == 0).all())
        if case[3] == 512:
            zero_rows = (ref["basis"] == 0).all(1)
            cl = got["mel"][..., zero_rows]
            assert int(zero_rows.sum()) == 12 and int(R.ulps_f32(cl, torch.full_like(cl, float(R.log_clamp_f32()))).max()) <= 2
            assert bool((got["p"][..., zero_rows] == 0).all())


def test_clamp_case_and_clamped_entries_contribute_nothing(gpu):
    from easevoice_trainer_amd.hip import lib as L

    case = R.CLAMP_CASE
    ref = R.mel_case_reference(case, "quiet", "clamp")
    live, clamped, _ = R.clamp_sets(ref)
    assert int(clamped.sum()) > 0 and int(live.sum()) > 0
    got = _run(L, gpu, case, ref["wav"], ref["basis"], ref["dmel"])
    _check_stages(got, ref, f"{R.case_id(case)} quiet clamp-basis")
    # the same backward with dmel changed at clamped entries only: atomics leave the order free, hence twice the bound
    dmel2 = ref["dmel"].clone()
    dmel2[clamped] = dmel2[clamped] * -3.0 + 11.0
    got2 = _run(L, gpu, case, ref["wav"], ref["basis"], dmel2)
    assert float((got2["dwav"].double() - got["dwav"].double()).abs().max()) <= 2 * R.tol_dwav(ref)
    assert float((got2["dwav"].double() - ref["dwav"]).abs().max()) <= R.tol_dwav(ref)


def test_onehot_basis_stores_the_magnitude_itself(gpu):
    from easevoice_trainer_amd.hip import lib as L

    case = R.ONEHOT_CASE
    basis, bins = R.onehot_basis(case[3]), R.onehot_bins(case[3])
    for wave in ("randn", "quiet"):
        got = _run(L, gpu, case, R.waveform(case, wave), basis)
        want = got["mag"][..., bins]                                            # [nseq, frames, n_mels]
        assert torch.equal(got["p"].contiguous().view(torch.int32), want.contiguous().view(torch.int32)), \
            f"{wave}: {int((got['p'] != want).sum())} stored pre-log values differ from the magnitude of their bin"
        # the other 1024 products of a row are exact zeros, so the log is taken of the magnitude itself
        logp = torch.log(torch.clamp(got["p"].double(), min=1e-5))
        assert bool(((got["mel"].double() - logp).abs() <= 4 * R.U * logp.abs().clamp(min=1.0)).all())


def test_mel_without_spec_out(gpu):
    from easevoice_trainer_amd.hip import lib as L

    case = R.MEL_CASES[2]
    ref = R.mel_case_reference(case, "randn")
    a = _run(L, gpu, case, ref["wav"], ref["basis"], want_spec=True)
    b = _run(L, gpu, case, ref["wav"], ref["basis"], want_spec=False)
    for k in ("re", "im", "p", "mel"):
        assert torch.equal(a[k], b[k]), k


def test_python_wrappers(gpu):
    """mel_spectrogram_torch with its autograd, and spectrogram_torch, at the config's geometry"""
    from easevoice_trainer_amd.module.mel_processing import mel_spectrogram_torch, spectrogram_torch

    case = R.MEL_CASES[2]
    ref = R.mel_case_reference(case, "randn")
    y = ref["wav"].to(gpu).requires_grad_(True)
    mel = mel_spectrogram_torch(y, R.NFFT, case[3], R.SR, case[2], R.NFFT, 0.0, None)
    mel.backward(ref["dmel"].transpose(1, 2).contiguous().to(gpu))
    spec = spectrogram_torch(ref["wav"].to(gpu), R.NFFT, R.SR, case[2], R.NFFT)
    got = dict(mel=mel.detach().transpose(1, 2).cpu(), mag=spec.transpose(1, 2).cpu(), dwav=y.grad.cpu())
    assert _ratio((got["mag"].double() - ref["mag"]).abs(), R.tol_mag(ref)) <= 1.0
    assert _ratio((got["mel"].double() - ref["mel"]).abs(), R.tol_mel_live(ref)) <= 1.0
    assert float((got["dwav"].double() - ref["dwav"]).abs().max()) <= R.tol_dwav(ref)


REFUSALS = [    # (n_fft, n_mels, hop, wav_len, code)
    (1024, 128, 640, 3000, ENOTSUP),
    (2048, 513, 640, 3000, ENOTSUP),
    (2048, 128, 0, 3000, ENOTSUP),
    (2048, 128, 2049, 5000, ENOTSUP),
    (2048, 128, 640, 704, EINVAL),
]


@pytest.mark.parametrize("n_fft,n_mels,hop,wav_len,code", REFUSALS)
def test_refusals_leave_the_outputs_untouched(gpu, n_fft, n_mels, hop, wav_len, code):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.module.mel_processing import mel_spectrogram_torch

    lib, nseq, n = L.lib(), 2, 1 << 16                 # n floats: more than any of these shapes would write if accepted
    wav = torch.zeros(nseq, wav_len, device=gpu)
    win = torch.hann_window(2048, device=gpu)
    basis = torch.zeros(513, R.NBIN, device=gpu)
    bufs = {k: torch.full((n,), SENT, device=gpu) for k in ("ws", "mel", "spec", "dwav", "dmel")}
    rc = lib.evt_mel_fwd(L.ptr(wav), L.ptr(win), L.ptr(basis), L.ptr(bufs["spec"]), L.ptr(bufs["mel"]), L.ptr(bufs["ws"]),
                         nseq, wav_len, n_fft, hop, n_mels, L.stream_ptr())
    assert rc == code
    rc = lib.evt_mel_bwd(L.ptr(bufs["dmel"]), L.ptr(win), L.ptr(basis), L.ptr(bufs["ws"]), L.ptr(bufs["dwav"]), nseq,
                         wav_len, n_fft, hop, n_mels, L.stream_ptr())
    assert rc == code
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == SENT).all()), f"{k} was written by a refused call"
    with pytest.raises(L.EvtError):
        mel_spectrogram_torch(wav, n_fft, n_mels, R.SR, hop, n_fft, 0.0, None)
    # the workspace queries answer for a refused geometry too (hop = 0: no division by it)
    nws = lib.evt_mel_workspace_floats(nseq, wav_len, n_fft, hop, n_mels)
    dims = (C.c_int64 * 5)(nseq, wav_len, n_fft, hop, n_mels)
    assert lib.evt_workspace_bytes(1, dims, 5) == 4 * nws and (nws == 0 if hop == 0 else nws >= 0)


def test_shortest_accepted_waveform(gpu):
    """wav_len = pad + 1 = 705 at hop 640 is accepted (704 is refused above)"""
    from easevoice_trainer_amd.hip import lib as L

    case = (1, 705, 640, 128)
    ref = R.mel_case_reference(case, "randn")
    got = _run(L, gpu, case, ref["wav"], ref["basis"])
    assert tuple(got["mel"].shape) == (1, 1, 128) and bool(torch.isfinite(got["mel"]).all())
