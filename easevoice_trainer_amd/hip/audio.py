"""The finishing step of a ragged s2 decode: the vocoder's rows resampled to the requested rate, converted to the requested
sample format and packed into one device buffer by ONE launch (csrc/resample_poly.hip::evt_resample_pack_rows; include/evt.h
has the operator's definition).  The int16 conversion and the silence interval are the reference's audio_postprocess
(inference/tts.py:878-908); the resampler is resampy's kaiser_best filter as feature_extractor/normalize.py restates it for
the ratio 1/2, written for any ratio: at 1/2 its taps are normalize._half_band_taps() and the operator is resample_half.
The filter's constants are taken from there.

The input end uses the same operator: `ingest_pcm` / `load_audio_batch` take the sample bytes of WAV files (audiokit/wav.py)
to packed mono fp32 rows at the pipeline's rate in one launch per input rate (csrc/pcm_ingest.hip::evt_pcm_ingest_rows)."""
import math
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from . import trace as T
from . import lib as L
from ..feature_extractor.normalize import _BETA, _ROLLOFF, _ZEROS

PCM_F32, PCM_S16 = 0, 1
FORMATS = {"float32": (PCM_F32, torch.float32), "int16": (PCM_S16, torch.int16)}
TILE = 2048            # EVT_RESAMPLE_TILE: outputs of one row per block, counted from the row's output 0
MAX_FACTOR = 1024      # largest reduced up / down served
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)     # the rates in everyday use from the model's 32 kHz


def rate_ratio(in_rate, out_rate):
    """(up, down) = out_rate / in_rate reduced; EvtError for a rate <= 0 or a factor above MAX_FACTOR"""
    if int(in_rate) != in_rate or int(out_rate) != out_rate or in_rate <= 0 or out_rate <= 0:
        raise L.EvtError(f"sample rates must be positive integers, got {in_rate} -> {out_rate}")
    g = math.gcd(int(in_rate), int(out_rate))
    up, down = int(out_rate) // g, int(in_rate) // g
    if up > MAX_FACTOR or down > MAX_FACTOR:
        raise L.EvtError(f"{in_rate} -> {out_rate} Hz reduces to {up}/{down}: factors above {MAX_FACTOR} are not served")
    return up, down


def out_len(n, up, down):
    """outputs of a row of n samples"""
    return (int(n) * up) // down


def poly_taps(up, down):
    """g[k], k = -(H - 1) .. H - 1 (float64, 2 H - 1 values, g[0] at index H - 1), H = Z * max(up, down):
    g[k] = s * rho * sinc(rho * s * k / up) * I0(beta * sqrt(1 - (s k / (up Z))^2)) / I0(beta), s = min(1, up / down).
    s k / up = k / max(up, down) and s k / (up Z) = k / H exactly, which is how they are evaluated."""
    m = max(int(up), int(down))
    h = _ZEROS * m
    k = np.arange(-(h - 1), h, dtype=np.float64)
    s = min(1.0, up / down)
    taper = np.i0(_BETA * np.sqrt(1.0 - (k / h) ** 2.0)) / np.i0(float(_BETA))
    return s * (_ROLLOFF * np.sinc(_ROLLOFF * k / m)) * taper


def table_shape(up, down):
    """(R, J): R = ceil(H / up) input samples on either side of an output's centre, J = 2 R + 1 taps per phase padded to a
    multiple of 4"""
    h = _ZEROS * max(int(up), int(down))
    r = -(-h // int(up))
    return r, (2 * r + 1 + 3) // 4 * 4


def phase_rows(up, down):
    """T[p][j] = g[p + (R - j) * up] (float64 [up, J]), zero where |p + (R - j) up| >= H and in the padding j > 2 R: output m
    with m * down = q * up + p is sum_j T[p][j] * x[q - R + j]"""
    g = poly_taps(up, down)
    h = (len(g) + 1) // 2
    r, j_pad = table_shape(up, down)
    k = np.arange(up)[:, None] + (r - np.arange(j_pad)[None, :]) * up
    live = (np.abs(k) < h) & (np.arange(j_pad)[None, :] <= 2 * r)
    return np.where(live, g[np.clip(k + h - 1, 0, len(g) - 1)], 0.0)


_TABLES = {}


def phase_table(up, down, device):
    """phase_rows rounded once to fp32, on the device; kept per (up, down, device)"""
    device = torch.device(device)
    key = (int(up), int(down), device.type, device.index)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(phase_rows(up, down).astype(np.float32)).to(device).contiguous()
    return t


@dataclass
class PackedAudio:
    """data: 1-D device tensor (int16 or float32) holding every row and `gap` zeros behind each; row b lies at
    data[offsets[b] : offsets[b] + lengths[b]]"""
    data: torch.Tensor
    offsets: List[int]
    lengths: List[int]
    rate: int
    gap: int = 0

    def row(self, b, gap=False):
        """a view of row b, without (or with) the silence behind it"""
        return self.data[self.offsets[b]:self.offsets[b] + self.lengths[b] + (self.gap if gap else 0)]

    def __len__(self):
        return len(self.lengths)


def resample_pack(x, lens, mul, in_rate, out_rate, out_format, order=None, interval=0.0, lens_dev=None, owner=None):
    """x [nseq, L] (or [nseq, L, 1], or one row [L]) contiguous fp32 / bf16 / f16 on the GPU; row s has
    n_s = min(lens[s] * mul, L) live samples.  lens: a sequence of ints (the host sizes the buffer from them); lens_dev:
    the same values as an int32 tensor on x's device where the caller has one (decode_batch does), uploaded otherwise.
    -> PackedAudio at out_rate in out_format ("int16" / "float32"): row s resampled to (n_s * up) // down samples (the
    operator of include/evt.h; out_rate == in_rate passes the values through), gap = int(out_rate * interval) zeros behind
    every row (the reference's zero_wav).  order: a permutation of the rows, the sequence in which they lie in the buffer
    (default: 0, 1, ...); offsets are the host's prefix sum of To_s + gap in that sequence.  One launch writes every
    element of the buffer: no memset in front of it."""
    if out_format not in FORMATS:
        raise L.EvtError(f"out_format must be one of {sorted(FORMATS)}, got {out_format!r}")
    code, out_dtype = FORMATS[out_format]
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() == 3 and x.size(2) == 1:
        x = x.squeeze(2)
    if x.dim() != 2 or not x.is_contiguous() or x.size(0) < 1 or x.size(1) < 1:
        raise L.EvtError(f"resample_pack takes contiguous rows [nseq, L], got {tuple(x.shape)}")
    nseq, length = x.size(0), x.size(1)
    lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    mul = int(mul)
    if len(lens) != nseq or mul < 1 or min(lens) < 0:
        raise L.EvtError(f"resample_pack: {nseq} lengths >= 0 and mul >= 1 expected, got {lens} and mul = {mul}")
    if lens_dev is None:
        lens_dev = torch.tensor(lens, dtype=torch.int32).to(x.device)
    L.check_lens("resample_pack", x, lens_dev, mul)
    up, down = rate_ratio(in_rate, out_rate)
    if interval < 0:
        raise L.EvtError(f"interval = {interval} must be >= 0")
    gap = int(out_rate * interval)
    order = list(range(nseq)) if order is None else [int(b) for b in order]
    if sorted(order) != list(range(nseq)):
        raise L.EvtError(f"order must be a permutation of the {nseq} rows, got {order}")
    lengths = [out_len(min(n * mul, length), up, down) for n in lens]
    offsets, total = [0] * nseq, 0
    for b in order:
        offsets[b] = total
        total += lengths[b] + gap
    data = torch.empty(total, dtype=out_dtype, device=x.device)
    if total == 0:
        return PackedAudio(data, offsets, lengths, int(out_rate), gap)
    off_dev = torch.tensor(offsets, dtype=torch.int64).to(x.device)
    table, j_pad = (None, 0) if up == down == 1 else (phase_table(up, down, x.device), table_shape(up, down)[1])
    e0 = T.t0()
    L.check(L.lib().evt_resample_pack_rows(L.dt_of(x), L.ptr(x), L.ptr(lens_dev), mul, nseq, length, up, down, L.ptr(table),
                                           j_pad, code, L.ptr(data), total, L.ptr(off_dev), gap, L.stream_ptr()),
            "evt_resample_pack_rows")
    if e0 is not None:
        T.t1_elt(e0, "resample_pack_kernel", x.numel() * x.element_size() + data.numel() * data.element_size(), owner)
    return PackedAudio(data, offsets, lengths, int(out_rate), gap)


def upload_raw(batch, device):
    """the staged bytes of an audiokit.wav.RawBatch on the device: one copy from page-locked memory, asynchronous on the
    current stream"""
    return batch.raw.to(torch.device(device), non_blocking=True)


def ingest_pcm(batch, out_rate, device="cuda:0", raw_dev=None, out=None, offsets=None):
    """batch: audiokit.wav.RawBatch (the sample bytes of WAV files of any served encoding, channel count and rate in one
    page-locked buffer) -> PackedAudio at out_rate, float32, gap 0, rows in the batch's order: every recording decoded, mixed
    down to mono and resampled on the GPU (csrc/pcm_ingest.hip::evt_pcm_ingest_rows; include/evt.h has the operator).  One
    upload of the buffer, then one launch per distinct input rate.  rate_ratio's MAX_FACTOR rule holds for every input rate
    of the batch: EvtError otherwise, before anything is uploaded.
    raw_dev: the buffer on the device where the caller has uploaded it (upload_raw) -- a second call then ingests the same
    upload at another rate.  out / offsets: a 1-D float32 device tensor and the element at which each row starts in it,
    where the rows go next to other data (slice_batch); by default a buffer of their own, back to back.
    An empty batch, or one whose rows all come out empty, touches no device: the PackedAudio then holds an empty CPU tensor
    (or `out` as it is)."""
    infos = list(batch.infos)
    ratios = {rate: rate_ratio(rate, out_rate) for rate in batch.by_rate}
    lengths = [out_len(i.frames, *ratios[i.rate]) for i in infos]
    if offsets is None:
        offsets, total = [], 0
        for n in lengths:
            offsets.append(total)
            total += n
    else:
        offsets = [int(v) for v in offsets]
        if out is None or len(offsets) != len(infos):
            raise L.EvtError(f"ingest_pcm: offsets go with `out` and number {len(infos)}, one per recording")
    if out is not None and (out.dtype != torch.float32 or out.dim() != 1 or not out.is_cuda or not out.is_contiguous()
                            or any(o < 0 or o + n > out.numel() for o, n in zip(offsets, lengths))):
        raise L.EvtError("ingest_pcm: `out` is a contiguous 1-D float32 device tensor that holds every row at its offset")
    if not any(lengths):
        return PackedAudio(torch.empty(0, dtype=torch.float32) if out is None else out, offsets, lengths, int(out_rate), 0)
    device = torch.device(device) if out is None else out.device
    with torch.cuda.device(device):
        if raw_dev is None:
            raw_dev = upload_raw(batch, device)
        if raw_dev.dtype != torch.uint8 or raw_dev.dim() != 1 or raw_dev.numel() != batch.raw.numel() or not raw_dev.is_cuda:
            raise L.EvtError(f"ingest_pcm: raw_dev must be the batch's {batch.raw.numel()} bytes as a uint8 tensor on the GPU")
        if out is None:
            out = torch.empty(sum(lengths), dtype=torch.float32, device=device)
        order = [r for rows in batch.by_rate.values() for r in rows]             # group by group
        wide = torch.tensor([[batch.byte_off[r] for r in order], [infos[r].frames for r in order],
                             [offsets[r] for r in order]], dtype=torch.int64).to(device)
        narrow = torch.tensor([[infos[r].fmt for r in order], [infos[r].channels for r in order]],
                              dtype=torch.int32).to(device)
        first = 0
        for rate, rows in batch.by_rate.items():
            k, (up, down) = len(rows), ratios[rate]
            max_frames = max(infos[r].frames for r in rows)
            if out_len(max_frames, up, down) > 0:
                table, j_pad = (None, 0) if up == down == 1 else (phase_table(up, down, device), table_shape(up, down)[1])
                cols = slice(first, first + k)
                e0 = T.t0()
                L.check(L.lib().evt_pcm_ingest_rows(L.ptr(raw_dev), raw_dev.numel(), L.ptr(wide[0, cols]), L.ptr(wide[1, cols]),
                                                    L.ptr(narrow[0, cols]), L.ptr(narrow[1, cols]), k, max_frames, up, down,
                                                    L.ptr(table), j_pad, L.ptr(out), out.numel(), L.ptr(wide[2, cols]),
                                                    L.stream_ptr()), "evt_pcm_ingest_rows")
                if e0 is not None:
                    T.t1_elt(e0, "pcm_ingest_kernel", sum(infos[r].data_bytes + 4 * lengths[r] for r in rows), None)
            first += k
    return PackedAudio(out, offsets, lengths, int(out_rate), 0)


def load_audio_batch(paths, out_rate=32000, device="cuda:0"):
    """The batch form of the reference's load_audio(file, sr) (utils/audio/__init__.py:13-32) and of librosa.load(path,
    sr=...): WAV files of any served encoding, channel count and rate (audiokit/wav.py) -> PackedAudio of mono float32 rows
    at out_rate on the device -- probe, stage, ingest_pcm.
    The boundary: the reference's load_audio runs ffmpeg, whose swr resampler is a different filter that cannot be pinned
    offline; no sample parity with ffmpeg's output at a changed rate is claimed.  At an unchanged rate and PCM16 the samples
    are the reference's (x / 32768, the mean of the channels).  Against librosa.load the filter is the same one (resampy's
    kaiser_best, straight from the file's own rate) with fp32 accumulation in place of float64."""
    from ..audiokit import wav

    return ingest_pcm(wav.stage(paths), out_rate, device)


REF_NFFT = 2048        # the transform of csrc/stft_mel.hip


def ref_frames(n, hop=640):
    """frames of a clip of n samples (include/evt.h): n // 640 at hop 640, 0 for a clip the reflect padding refuses"""
    pad = (REF_NFFT - hop) // 2
    return (n + 2 * pad - REF_NFFT) // hop + 1 if n > pad and n + 2 * pad >= REF_NFFT else 0


def ref_spec_rows(x, lens, hop=640, bins=704, lens_dev=None):
    """The reference's _get_ref_spec (inference/tts.py:390-409) for a ragged batch of reference clips, two launches and no
    host synchronisation (csrc/stft_mel.hip::evt_ref_spec_rows; include/evt.h has the operator's definition).  x [nseq, N]
    contiguous fp32 on the GPU (or one clip [N]), row s with lens[s] live samples, never read behind them; lens: a sequence
    of ints, uploaded unless lens_dev (the same values as an int32 tensor on x's device) is given.
    -> (spec fp32 [nseq, Fmax, bins] channels-last -- the first `bins` bins of sqrt(re^2 + im^2 + 1e-6) of the clip divided
    by min(2, peak) where its peak exceeds 1, exact zeros behind a row's frames --, frames: list of F_s, peak fp32 [nseq]).
    A row of at most pad = (2048 - hop) // 2 samples is an EvtError, as torch's reflect padding refuses it."""
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.size(0) < 1 or x.size(1) < 1:
        raise L.EvtError(f"ref_spec_rows takes contiguous fp32 rows [nseq, N] on the GPU, got {x.dtype} {tuple(x.shape)} on {x.device}")
    nseq, n = x.size(0), x.size(1)
    lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    hop, bins = int(hop), int(bins)
    if hop <= 0 or hop > REF_NFFT or not 1 <= bins <= REF_NFFT // 2 + 1:
        raise L.EvtError(f"ref_spec_rows: hop in [1, {REF_NFFT}] and bins in [1, {REF_NFFT // 2 + 1}] expected, got {hop} and {bins}")
    if len(lens) != nseq or max(lens) > n:
        raise L.EvtError(f"ref_spec_rows: {nseq} lengths of at most {n} samples expected, got {lens}")
    frames = [ref_frames(v, hop) for v in lens]
    if min(frames) < 1:
        raise L.EvtError(f"ref_spec_rows: clip {frames.index(min(frames))} has {lens[frames.index(min(frames))]} samples, "
                         f"too few for the reflect padding of {(REF_NFFT - hop) // 2} and one frame")
    if lens_dev is None:
        lens_dev = torch.tensor(lens, dtype=torch.int32).to(x.device)
    L.check_lens("ref_spec_rows", x, lens_dev)
    from ..module.mel_processing import _window

    window = _window(REF_NFFT, x.device)              # the tensor spectrogram_torch hands its kernel
    spec = torch.empty((nseq, ref_frames(n, hop), bins), dtype=torch.float32, device=x.device)
    peak = torch.empty(nseq, dtype=torch.float32, device=x.device)
    e0 = T.t0()
    L.check(L.lib().evt_ref_spec_rows(L.ptr(x), L.ptr(lens_dev), nseq, n, L.ptr(window), REF_NFFT, hop, bins,
                                      L.ptr(spec), L.ptr(peak), L.stream_ptr()), "evt_ref_spec_rows")
    if e0 is not None:
        T.t1_elt(e0, "ref_spec_kernel", (x.numel() + spec.numel()) * 4, None)
    return spec, frames, peak
