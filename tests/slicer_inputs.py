"""Closed-form inputs of the slicer tests: float32 recordings built from a 32-bit LCG and a handful of exactly rounded IEEE
operations, so that tests/golden/make_golden_slicer.py and the tests hold the same bits on any numpy."""
import numpy as np

LOUD, QUIET, ZERO = "loud", "quiet", "zero"
# case A, milliseconds: a leading silence, all three silence-length branches of the tag logic (0.4 s, 0.8 s, 1.5 s against
# max_sil_kept = 0.5 s), a clip that is too short to be cut off (2 s), a run of exact zeros with its argmin ties, and a
# trailing silence
PLAN_A = [(QUIET, 800), (LOUD, 5000), (QUIET, 400), (LOUD, 5000), (QUIET, 800), (LOUD, 5000), (QUIET, 1500), (LOUD, 2000),
          (QUIET, 400), (LOUD, 3000), (ZERO, 450), (LOUD, 4500), (QUIET, 600)]
PARAMS_A = dict(sr=32000)
PARAMS_B = dict(sr=32000, min_length=400, min_interval=40, hop_size=5, max_sil_kept=60)     # win 640, hop 160
PARAMS_C = dict(sr=44100, hop_size=10, min_interval=30)                                     # the odd window 1323
LOUD_AMP, QUIET_AMP = np.float32(0.3), np.float32(2e-3)


def lcg_bits(n, seed):
    """the first n states of x <- 1664525 x + 1013904223 (mod 2^32) behind `seed`, by doubling: x[m + k] = A_m x[k] + C_m"""
    out = np.empty(max(n, 1), dtype=np.uint64)
    a, c, mask = 1664525, 1013904223, 0xFFFFFFFF
    out[0] = (a * (seed & mask) + c) & mask
    m, am, cm = 1, a, c
    while m < n:
        k = min(m, n - m)
        out[m:m + k] = (out[:k] * np.uint64(am) + np.uint64(cm)) & np.uint64(mask)
        am, cm = (am * am) & mask, (cm * am + cm) & mask
        m *= 2
    return out[:n]


def noise(n, seed):
    """uniform in [-1, 1) on a 2^-23 grid: the upper 24 bits of the LCG, exact in float32"""
    u = (lcg_bits(n, seed) >> np.uint64(8)).astype(np.int64) - (1 << 23)
    return u.astype(np.float32) * np.float32(2.0 ** -23)


def from_plan(plan, sr, seed, scale=1):
    """the segments of `plan` (kind, milliseconds) back to back at sr, durations divided by `scale`; a quiet segment's level
    is a V: QUIET_AMP at its ends, a quarter of it in the middle"""
    counts = [sr * ms // (1000 * scale) for _, ms in plan]
    x = noise(sum(counts), seed)
    pos = 0
    for (kind, _), n in zip(plan, counts):
        seg = x[pos:pos + n]
        if kind == LOUD:
            seg *= LOUD_AMP
        elif kind == ZERO:
            seg[:] = 0
        else:
            i = np.arange(n, dtype=np.int64)
            level = (np.abs(2 * i - n) * 3 + n).astype(np.float64) / np.float64(4 * n)
            seg *= QUIET_AMP * level.astype(np.float32)
        pos += n
    return x


def case_a():
    return from_plan(PLAN_A, 32000, 1)


def case_b():
    x = from_plan(PLAN_A, 32000, 2, scale=10)
    x[20000] = np.float32(1.7)          # inside the second loud part: that chunk's peak exceeds 1
    return x


def case_c():
    plan = [(LOUD, 300), (QUIET, 200)] * 4
    x = from_plan(plan, 44100, 3)
    return np.concatenate([x, noise(100001 - x.shape[0], 4) * LOUD_AMP])


EDGE_LENGTHS = (1, 319, 320, 400, 96000)   # at most min_length (400 frames, compared with samples) and 3 s without silence


def edges():
    return [noise(n, 10 + k) * LOUD_AMP for k, n in enumerate(EDGE_LENGTHS)]


def pairwise(a):
    """NumPy's pairwise float32 summation of the last axis of `a`, as include/evt.h states it for evt_rms_frames_rows"""
    n = a.shape[-1]
    if n < 8:
        res = np.zeros(a.shape[:-1], dtype=np.float32)
        for i in range(n):
            res = res + a[..., i]
        return res
    if n <= 128:
        m = n - n % 8
        r = [a[..., j].copy() for j in range(8)]
        for i in range(8, m, 8):
            for j in range(8):
                r[j] = r[j] + a[..., i + j]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(m, n):
            res = res + a[..., i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[..., :n2]) + pairwise(a[..., n2:])


def emulate_rms(x, win, hop):
    y = np.pad(x, (win // 2, win // 2))
    frames = (x.shape[0] + 2 * (win // 2) - win) // hop + 1
    idx = np.arange(frames)[:, None] * hop + np.arange(win)[None, :]
    v = y[idx]
    return np.sqrt(pairwise(v * v) / np.float32(win))
