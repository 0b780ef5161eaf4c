"""Shared by the WAV ingest tests: files of every served encoding written with struct from integer or float arrays (nothing
of audiokit/wav.py is used), and the operator of evt_pcm_ingest_rows in numpy from its definition (include/evt.h): decode,
then the channels added one after the other in float32, then one float32 division.  The float64 answer of the resampling
step is tests/resample_oracle.py::resample."""
import math
import struct

import numpy as np

import resample_oracle as O

U8, S16, S24, S32, F32, F64 = range(6)
NAMES = ("u8", "s16", "s24", "s32", "f32", "f64")
WIDTH = (1, 2, 3, 4, 4, 8)
BITS = (8, 16, 24, 32, 32, 64)
TAG = (1, 1, 1, 1, 3, 3)
PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")      # KSDATAFORMAT_SUBTYPE_*: the tag + these 14 bytes


def sample_bytes(samples, fmt):
    """samples [frames, C] (or [frames]): integers in the format's range, or floats for F32 / F64 -> interleaved
    little-endian bytes"""
    a = np.asarray(samples)
    if fmt == U8:
        return a.astype(np.uint8).tobytes()
    if fmt == S16:
        return a.astype("<i2").tobytes()
    if fmt == S24:
        return a.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    if fmt == S32:
        return a.astype("<i4").tobytes()
    return a.astype("<f4" if fmt == F32 else "<f8").tobytes()


def fmt_chunk(fmt, channels, rate, form="plain", tag=None, block=None, bits=None):
    """form: "plain" (16 bytes), "fmt18" (cbSize = 0 behind them) or "ext" (WAVE_FORMAT_EXTENSIBLE, 40 bytes)"""
    tag = TAG[fmt] if tag is None else tag
    bits = BITS[fmt] if bits is None else bits
    block = channels * WIDTH[fmt] if block is None else block
    body = struct.pack("<HHIIHH", 0xFFFE if form == "ext" else tag, channels, rate & 0xFFFFFFFF, (rate * block) & 0xFFFFFFFF,
                       block, bits)
    if form == "fmt18":
        body += struct.pack("<H", 0)
    elif form == "ext":
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + PCM_GUID_TAIL
    return b"fmt " + struct.pack("<I", len(body)) + body


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def wav_file(path, data, fmt, channels, rate, form="plain", before=b"", data_size=None, after=b"", magic=b"RIFF", **fmt_kw):
    """data: the sample bytes; before: whole chunks between `fmt ` and `data`; data_size: the size the data chunk claims
    (default: its own); after: bytes behind the data.  -> the position of the first sample byte"""
    head = fmt_chunk(fmt, channels, rate, form, **fmt_kw) + before
    size = len(data) if data_size is None else data_size
    body = b"WAVE" + head + b"data" + struct.pack("<I", size) + data + after
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<I", len(body) & 0xFFFFFFFF) + body)
    return 12 + len(head) + 8


def decode(samples, fmt):
    """the decode step: [frames, C] samples -> float32, exact or one round-to-nearest-even"""
    a = np.asarray(samples)
    if fmt == U8:
        return (a.astype(np.int32) - 128).astype(np.float32) * np.float32(2.0 ** -7)
    if fmt == S16:
        return a.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -15)
    if fmt == S24:
        return a.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -23)
    if fmt == S32:
        return a.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -31)       # int32 -> float32 rounds to nearest even
    if fmt == F32:
        return a.astype(np.float32)
    with np.errstate(over="ignore"):
        return a.astype(np.float64).astype(np.float32)


def downmix(v):
    """[frames, C] float32 -> [frames]: ((v_0 + v_1) + ...) + v_{C-1} in float32, one float32 division by C (C > 1)"""
    v = np.asarray(v, dtype=np.float32).reshape(len(v), -1)
    acc = v[:, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(1, v.shape[1]):
            acc = (acc + v[:, c]).astype(np.float32)
        if v.shape[1] > 1:
            acc = (acc / np.float32(v.shape[1])).astype(np.float32)
    return acc


def mono(samples, fmt):
    return downmix(decode(np.asarray(samples).reshape(len(samples), -1), fmt))


def ratio(in_rate, out_rate):
    g = math.gcd(in_rate, out_rate)
    return out_rate // g, in_rate // g


def frames_for(to, up, down):
    """the smallest n with n * up // down == to"""
    return -(-to * down // up)


def ints(fmt, frames, channels, seed):
    """uniform integers over the format's whole range, with both extremes, 0 and -1 in front"""
    lo, hi = {U8: (0, 255), S16: (-2 ** 15, 2 ** 15 - 1), S24: (-2 ** 23, 2 ** 23 - 1), S32: (-2 ** 31, 2 ** 31 - 1)}[fmt]
    a = np.random.default_rng(seed).integers(lo, hi + 1, size=(frames, channels), dtype=np.int64)
    edge = [lo, hi, 128 if fmt == U8 else 0, 127 if fmt == U8 else -1]
    flat = a.reshape(-1)
    flat[:min(len(edge), flat.size)] = edge[:flat.size]
    return a


def floats(fmt, frames, channels, seed):
    a = np.random.default_rng(seed).uniform(-0.95, 0.95, size=(frames, channels))
    return a.astype(np.float32) if fmt == F32 else a


def samples_of(fmt, frames, channels, seed):
    return floats(fmt, frames, channels, seed) if fmt >= F32 else ints(fmt, frames, channels, seed)


def oracle(m, up, down, step=8192):
    """(want, bound) per output of the mono float32 row m: the float64 resample and 2^-24 (Jm + 3) A[m].  A long row is taken
    in pieces of `step` outputs to bound the oracle's memory: a piece starts at an output that is a multiple of `up` (phase
    0, an input index of its own) and is computed from the inputs its taps reach, so every sum has the terms it has in the
    whole row."""
    x = np.asarray(m, dtype=np.float64)
    n = len(x)
    to = (n * up) // down
    if to <= 2 * step:
        want, a, jm = O.resample(x, up, down)
        return want, 2.0 ** -24 * (jm + 3) * a
    reach = -(-64 * max(up, down) // up) + 1                   # inputs on either side of an output's centre
    margin = -(-(reach * up // down + 2) // up) * up            # outputs in front of a piece, a multiple of up
    step = -(-step // up) * up
    wants, bounds = [], []
    for a0 in range(0, to, step):
        b0 = min(a0 + step, to)
        first = max(a0 - margin, 0)
        lo, hi = first * down // up, n if b0 == to else min(n, -(-b0 * down // up) + reach + down)
        want, a, jm = O.resample(x[lo:hi], up, down)
        wants.append(want[a0 - first:b0 - first])
        bounds.append((2.0 ** -24 * (jm + 3) * a)[a0 - first:b0 - first])
        assert len(wants[-1]) == b0 - a0
    return np.concatenate(wants), np.concatenate(bounds)
