"""References and inputs of tests/test_mel_gpu.py and tests/test_seg_loss_gpu.py (and of their CPU-side conditions,
tests/test_loss_refs_cpu.py).  Nothing here touches a GPU or the library's kernels.

Mel front end.  `mel_ref` is the stage-by-stage formula of csrc/stft_mel.hip in plain torch ops: reflect index, frames
through `unfold`, product with the window, torch.fft.rfft, sqrt(re^2 + im^2 + 1e-6), mag @ basis^T, log(clamp(p, 1e-5)).
It returns every stage and is differentiable.  Run in float64 on the float32 operands (converted exactly: what the kernel
reads) it is the reference; run in float32 it is the yardstick: how far a careful fp32 evaluation of the same formula
lands from the float64 one, which is what the kernel's tolerances are tied to (never to the kernel's own numbers).

Segment losses.  Operands are dyadic: values are multiples of 1/8 in a bounded range, scales and dloss powers of two,
targets 0 and 1.  Every term |a - b| or (target - a)^2 times its scale is then an integer multiple of one unit (the
smallest scale times the term unit), and as long as the whole sum stays below 2^24 units every partial sum in ANY order
-- thread, block tree, atomics -- is exact in fp32: the kernel has to reproduce the float64 sum bit for bit.
"""
import functools
import math

import numpy as np
import torch

NFFT = 2048
NBIN = NFFT // 2 + 1
SR = 32000
U = 2.0 ** -24                      # fp32 unit round-off
CLAMP = 1e-5
F32_EXACT = 1 << 24

# (nseq, wav_len, hop, n_mels)
MEL_CASES = [
    (1, 705, 640, 128),             # one frame, reflected on both sides; wav_len = pad + 1
    (2, 1985, 641, 129),            # odd n_fft - hop; 3 frames; a second m0 pass with a single bin
    (3, 3000, 640, 128),            # the config's geometry; 4 frames; 3 sequences
    (1, 4096, 2048, 1),             # pad = 0, no overlap, one mel bin
    (2, 2500, 320, 512),            # 7 frames; the maximum n_mels; all-zero filterbank rows: p = 0
    (2, 20480, 640, 128),           # one training segment: 32 frames
]
WAVES = ("randn", "quiet", "zero")
CLAMP_CASE = (2, 1985, 641, 129)    # with `quiet` and clamp_basis: entries on both sides of the clamp
ONEHOT_CASE = (2, 2500, 320, 512)


def case_id(case):
    return "x".join(str(v) for v in case)


def gen(*key):
    """a torch.Generator seeded from the key (hash() of a tuple is not stable across processes)"""
    s = 0
    for part in key:
        for ch in repr(part):
            s = (s * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(s)


def geometry(wav_len, hop):
    pad = (NFFT - hop) // 2
    return pad, (wav_len + 2 * pad - NFFT) // hop + 1


def reflect_index(wav_len, hop):
    """index into the waveform of every sample of the reflect-padded one (no edge sample repeated)"""
    pad, _ = geometry(wav_len, hop)
    j = (torch.arange(wav_len + 2 * pad) - pad).abs()
    return torch.where(j >= wav_len, 2 * (wav_len - 1) - j, j)


def mel_ref(wav, window, basis, hop, dtype):
    """wav [nseq, wav_len], window [NFFT], basis [n_mels, NBIN] -> dict of stages, all [nseq, frames, ...]:
    xw (windowed frames), X (complex spectrum), mag, p (pre-log mel), mel"""
    wav, window, basis = wav.to(dtype), window.to(dtype), basis.to(dtype)
    fr = wav[:, reflect_index(wav.size(1), hop)].unfold(1, NFFT, hop)
    xw = fr * window
    X = torch.fft.rfft(xw, dim=-1)
    mag = torch.sqrt(X.real ** 2 + X.imag ** 2 + 1e-6)
    p = mag @ basis.T
    mel = torch.log(torch.clamp(p, min=CLAMP))
    return dict(xw=xw, X=X, mag=mag, p=p, mel=mel)


def hann():
    return torch.hann_window(NFFT, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def real_basis(n_mels):
    """the project's Slaney filterbank at the config's sampling rate, float32 [n_mels, NBIN]"""
    from easevoice_trainer_amd.module.mel_processing import mel_filterbank

    return torch.from_numpy(mel_filterbank(SR, NFFT, n_mels, 0.0, None))


def clamp_basis(n_mels):
    """the real basis with rows 1::4 scaled by 1e-3: with the quiet waveform those rows fall far below the clamp"""
    b = real_basis(n_mels).clone()
    b[1::4] *= 1e-3
    return b


ONEHOT_FIXED = (0, 1, 2, 1023, 1024)


def onehot_bins(n_mels=512):
    """bin of row m: the spectrum's ends first, then a walk over both parities"""
    bins = list(ONEHOT_FIXED) + [(3 + 2 * m + (m // 3) % 2) % NBIN for m in range(len(ONEHOT_FIXED), n_mels)]
    return torch.tensor(bins[:n_mels])


def onehot_basis(n_mels=512):
    b = torch.zeros(n_mels, NBIN, dtype=torch.float32)
    b[torch.arange(n_mels), onehot_bins(n_mels)] = 1.0
    return b


def waveform(case, wave, seed=0):
    nseq, wav_len = case[:2]
    if wave == "zero":
        return torch.zeros(nseq, wav_len, dtype=torch.float32)
    amp = {"randn": 0.1, "quiet": 1e-4}[wave]
    return (amp * torch.randn(nseq, wav_len, generator=gen("wav", case, wave, seed), dtype=torch.float64)).float()


def dmel_of(case, seed=0):
    nseq, wav_len, hop, n_mels = case
    _, frames = geometry(wav_len, hop)
    return torch.randn(nseq, frames, n_mels, generator=gen("dmel", case, seed), dtype=torch.float32)


def mel_reference(wav, basis, hop, dmel):
    """float64 stages + dwav, and the fp32 yardsticks Y_X (spectrum) and Y_b (backward) of the same formula on the CPU"""
    w64 = wav.double().requires_grad_(True)
    r64 = mel_ref(w64, hann(), basis, hop, torch.float64)
    (dw64,) = torch.autograd.grad(r64["mel"], w64, dmel.double())
    w32 = wav.clone().requires_grad_(True)
    r32 = mel_ref(w32, hann(), basis, hop, torch.float32)
    (dw32,) = torch.autograd.grad(r32["mel"], w32, dmel)
    ref = {k: v.detach() for k, v in r64.items()}
    ref["dwav"] = dw64
    ref["norm"] = ref["xw"].norm(dim=-1)                                     # ||xw||_2 per frame, [nseq, frames]
    err = (r32["X"].detach().to(torch.complex128) - ref["X"]).abs().amax(-1)
    live = ref["norm"] > 0
    ref["Y_X"] = float((err[live] / ref["norm"][live]).max()) if bool(live.any()) else 0.0
    assert float(err[~live].max() if bool((~live).any()) else 0.0) == 0.0
    top = float(dw64.abs().max())
    ref["Y_b"] = float((dw32.double() - dw64).abs().max()) / top if top > 0 else 0.0
    if top == 0:
        assert float(dw32.abs().max()) == 0.0
    return ref


@functools.lru_cache(maxsize=None)
def mel_case_reference(case, wave, basis_kind="real", seed=0):
    """computed once per process and shared: do not modify the tensors"""
    n_mels = case[3]
    basis = {"real": real_basis, "clamp": clamp_basis, "onehot": onehot_basis}[basis_kind](n_mels)
    wav = waveform(case, wave, seed)
    dmel = dmel_of(case, seed)
    ref = mel_reference(wav, basis, case[2], dmel)
    ref.update(wav=wav, basis=basis, dmel=dmel)
    return ref


CLAMP_MARGIN = 32       # in units of the pre-log mel's own tolerance


def clamp_sets(ref):
    """(live, clamped, undecided).  A kernel that meets the pre-log bound tol_p lands on the float64 side of the threshold
    wherever |p64 - 1e-5| > tol_p; the inputs keep every entry CLAMP_MARGIN times that away, so which side an entry is on
    never depends on rounding.  (Nearly all runs keep a factor 2: near_clamp below.)"""
    margin = CLAMP_MARGIN * tol_p(ref)
    live, clamped = ref["p"] > CLAMP + margin, ref["p"] < CLAMP - margin
    return live, clamped, ~(live | clamped)


def near_clamp(ref):
    """entries within a factor 2 of the threshold"""
    return (ref["p"] >= 0.5 * CLAMP) & (ref["p"] <= 2 * CLAMP)


# the runs that DO have entries within a factor 2 of the threshold: at 512 mel bins the lowest triangles are narrower than
# one FFT bin (15.6 Hz), catch a single bin near a corner and sum to as little as 4.5e-4, so that p = sum * mag crosses 1e-5
# for the quiet and the zero waveform (mag about 3e-3 and 1e-3).  Measured on the CPU: 102 and 224 entries of 7168, the
# closest 0.4 % and 3.5 % from the threshold -- 121 and 1112 pre-log tolerances (what tests/test_loss_refs_cpu.py prints).
NEAR_CLAMP_RUNS = {((2, 2500, 320, 512), "quiet", "real"), ((2, 2500, 320, 512), "zero", "real")}


# ---- stage tolerances (tests/test_mel_gpu.py; the derivations are in that module's docstring) -------------------------
def tol_X(ref):
    """[nseq, frames, 1]"""
    return (max(4 * ref["Y_X"], 22 * U) * ref["norm"]).unsqueeze(-1)


def tol_mag(ref):
    return tol_X(ref) + 4 * U * ref["mag"]


def tol_p(ref):
    return tol_X(ref) * ref["basis"].double().sum(1) + 517 * U * ref["p"]


def tol_mel_live(ref):
    p = ref["p"].clamp(min=CLAMP)           # only read where the entry is live
    return tol_p(ref) / p + 4 * U * torch.log(p).abs().clamp(min=1.0)


def tol_dwav(ref):
    return max(8 * ref["Y_b"], 64 * U) * float(ref["dwav"].abs().max())


def ulps_f32(a, b):
    """distance in fp32 representations between two fp32 tensors of one sign"""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


# ---- segment losses ------------------------------------------------------------------------------------------------------
# name -> sizes, the value grid (q = multiples of 1/8; the values are k * q with |k| <= kmax) and the power-of-two scales
# (cycled over the segments)
SEG_LISTS = {
    # total 22613: twelve chunks of 2048 cut the segments at offsets that are no multiple of the vector width
    "cuts": dict(sizes=[1, 7, 8, 9, 2047, 2048, 2049, 4099, 12345], q=0.125, kmax=16, scales=(1.0, 0.5, 2.0, 0.5)),
    # the segment limit: 64 segments of mixed small sizes
    "many": dict(sizes=[1 + (i * 53) % 257 for i in range(64)], q=0.125, kmax=16, scales=(1.0, 0.5, 2.0, 0.25)),
    # total 1100009 > 512 * 2048: the chunk becomes 4096
    "big": dict(sizes=[600001, 500003, 5], q=0.5, kmax=2, scales=(2.0, 1.0, 4.0)),
}
SEG_DLOSS = 0.5
SEG_PRESET = 3.0                    # `out` before the forward: the kernel accumulates
SEG_TARGETS = (0.0, 1.0)


def seg_scales(name):
    spec = SEG_LISTS[name]
    return [spec["scales"][i % len(spec["scales"])] for i in range(len(spec["sizes"]))]


SEG_GRID = 512          # blocks of the kernel's launch
SEG_VS = (4, 8)         # elements per 16-byte vector: fp32, 16-bit


def seg_partition(sizes, V):
    """the kernel's split replayed on the CPU (csrc/elementwise.hip::seg_flat_kernel, aligned bases): the flat index space in
    chunks of ceil(total / 512) rounded up to 2048; inside a segment a block's range [i0, i1) falls into a head up to the
    next multiple of V, a vector body and a tail.  -> per segment an int8 tensor: 0 head, 1 body, 2 tail"""
    total = sum(sizes)
    chunk = -(-(-(-total // SEG_GRID)) // 2048) * 2048
    kinds, s0 = [], 0
    for n in sizes:
        kind = torch.full((n,), -1, dtype=torch.int8)
        for blk in range(s0 // chunk, (s0 + n - 1) // chunk + 1):
            lo, hi = blk * chunk, min(total, (blk + 1) * chunk)
            i0, i1 = max(lo, s0) - s0, min(hi, s0 + n) - s0
            v0 = min(i1, -(-i0 // V) * V)
            v1 = v0 + (i1 - v0) // V * V
            kind[i0:v0], kind[v0:v1], kind[v1:i1] = 0, 1, 2
        assert int(kind.min()) >= 0
        kinds.append(kind)
        s0 += n
    return kinds


def seg_planted(sizes):
    """per segment, where a == b is put on purpose: the first and last two elements, two in the middle, and around every
    chunk boundary that cuts the segment the element before it (a tail), the boundary element and those up to the second
    next multiple of 8 (the head of the next block's range for either vector width, then its body)"""
    total = sum(sizes)
    chunk = -(-(-(-total // SEG_GRID)) // 2048) * 2048
    out, s0 = [], 0
    for n in sizes:
        pos = {0, 1, n // 2, n // 2 + 1, n - 2, n - 1}
        for c in range((s0 // chunk + 1) * chunk, s0 + n, chunk):
            o = c - s0
            pos.update(range(o - 1, -(-o // 8) * 8 + 9))
        out.append(sorted(p for p in pos if 0 <= p < n))
        s0 += n
    return out


@functools.lru_cache(maxsize=None)
def seg_operands(name, seed=0):
    """float64 lists (a, b): a_i, b_i of sizes[i], with a == b at seg_planted's positions: head, vector body and tail
    elements of the kernel's split for both vector widths (tests/test_loss_refs_cpu.py checks that against seg_partition)"""
    spec = SEG_LISTS[name]
    g = gen("seg", name, seed)
    a_list, b_list = [], []
    for n, planted in zip(spec["sizes"], seg_planted(spec["sizes"])):
        a = torch.randint(-spec["kmax"], spec["kmax"] + 1, (n,), generator=g).double() * spec["q"]
        b = torch.randint(-spec["kmax"], spec["kmax"] + 1, (n,), generator=g).double() * spec["q"]
        b[planted] = a[planted]
        a_list.append(a)
        b_list.append(b)
    return a_list, b_list


def seg_loss64(name, mode, target=0.0, seed=0):
    """the float64 loss: sum_i scale_i * sum |a_i - b_i|  (mode 0)  or  sum_i scale_i * sum (target - a_i)^2  (mode 1)"""
    a_list, b_list = seg_operands(name, seed)
    tot = 0.0
    for a, b, sc in zip(a_list, b_list, seg_scales(name)):
        term = (a - b).abs() if mode == 0 else (target - a) ** 2
        tot += sc * float(term.sum())
    return tot


def seg_units(name, mode, target=0.0, seed=0):
    """(the loss plus the preset counted in units, the unit): unit = smallest scale x term unit (q for L1, q^2 for LSGAN).
    Below 2^24 units every partial sum is exact in fp32."""
    spec = SEG_LISTS[name]
    unit = min(spec["scales"]) * (spec["q"] if mode == 0 else spec["q"] ** 2)
    count = (seg_loss64(name, mode, target, seed) + SEG_PRESET) / unit
    assert count == round(count) and SEG_PRESET / unit == round(SEG_PRESET / unit)
    return int(count), unit


def seg_random(sizes, dtype, seed=0):
    """random operands rounded to the stored type (as float64), for the tolerance tests"""
    g = gen("segrand", tuple(sizes), str(dtype), seed)
    a = [torch.randn(n, generator=g, dtype=torch.float64).to(dtype).double() for n in sizes]
    b = [torch.randn(n, generator=g, dtype=torch.float64).to(dtype).double() for n in sizes]
    return a, b


def lsgan_grad_f32(a, target, dl):
    """the kernel's expression -2 * (target - a) * dl evaluated op by op in float32 (a, the result: fp32 tensors)"""
    return (torch.tensor(-2.0, dtype=torch.float32) * (torch.tensor(target, dtype=torch.float32) - a.float())) * \
        torch.tensor(dl, dtype=torch.float32)


def f32_product(x, y):
    return float(np.float32(x) * np.float32(y))


def ulps_of(got, want):
    """distance in representable values of got's dtype (16- or 32-bit floats of one sign, or exact zeros)"""
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]

    def key(t):
        v = t.contiguous().view(it).long()
        return torch.where(v < 0, -(v & (2 ** (8 * t.element_size() - 1) - 1)), v)
    return (key(got) - key(want)).abs()


def log_clamp_f32():
    return np.float32(math.log(CLAMP))
