"""Float64 oracle of the resampler behind evt_resample_pack_rows, written from the operator's definition (include/evt.h) and
from nothing in hip/audio.py: the prototype filter g from the constants of feature_extractor/normalize.py, and the direct
sum y[m] = sum_i x[i] g[m down - i up] over the row's own samples.  Shared by tests/test_resample_poly_cpu.py and
tests/test_resample_pack_gpu.py."""
import math

import numpy as np

RATES = [8000, 16000, 22050, 24000, 32000, 44100, 48000]
IN_RATE = 32000


def ratio(out_rate, in_rate=IN_RATE):
    g = math.gcd(out_rate, in_rate)
    return out_rate // g, in_rate // g


def taps(up, down):
    """{k: g[k]} as an array over k = -(H - 1) .. H - 1, and H"""
    from easevoice_trainer_amd.feature_extractor.normalize import _BETA, _ROLLOFF, _ZEROS

    s = min(1.0, up / down)
    h = _ZEROS * max(up, down)
    k = np.arange(-(h - 1), h).astype(np.float64)
    sinc = np.sinc(_ROLLOFF * s * k / up)
    win = np.i0(_BETA * np.sqrt(np.maximum(0.0, 1.0 - (s * k / (up * _ZEROS)) ** 2))) / np.i0(_BETA)
    return s * _ROLLOFF * sinc * win, h


def resample(x, up, down):
    """x: 1-D array (read as float64) -> (y [To] float64, A [To] = sum |x[i]| |g[..]|, Jm [To] = live taps per output)"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    to = (n * up) // down
    g, h = taps(up, down)
    if to == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64)
    c = np.arange(to, dtype=np.int64) * down
    i_lo = -((h - 1 - c) // up)                       # ceil((c - H + 1) / up)
    width = 2 * (-(-h // up)) + 1
    i = i_lo[:, None] + np.arange(width, dtype=np.int64)[None, :]
    k = c[:, None] - i * up
    live = (np.abs(k) < h) & (i >= 0) & (i < n)
    gg = np.where(live, g[np.clip(k + h - 1, 0, len(g) - 1)], 0.0)
    xx = np.where(live, x[np.clip(i, 0, n - 1)], 0.0)
    return (gg * xx).sum(1), (np.abs(gg) * np.abs(xx)).sum(1), live.sum(1)


def to_int16(v):
    """the conversion rule on fp32 values: trunc(min(max(v * 32768, -32768), 32767)), NaN -> 0"""
    v = np.asarray(v, dtype=np.float32)
    s = np.minimum(np.maximum(v * np.float32(32768.0), np.float32(-32768.0)), np.float32(32767.0))
    return np.where(np.isnan(v), 0, np.trunc(np.nan_to_num(s))).astype(np.int16)
