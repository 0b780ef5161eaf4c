"""The audio slicer (src/audiokit/slicer/slicer.py and AudioService.slicer, src/service/audio.py:142-183 of the reference)
for a ragged batch of recordings: long recordings in, the 4 s+ clips that every later step consumes out, as int16 PCM.

The arithmetic runs on the GPU (hip/slicer.py): the recordings are uploaded once as one packed fp32 buffer, one launch takes
their peaks, one launch their RMS frames (bit for bit the reference's get_rms), the frames come back to the host, the tag
logic below walks them, and one peak launch plus one pack launch rescale every chunk of every recording into one packed
int16 buffer.  The tag logic is host work by nature: a few comparisons per silent run.

Recordings are float32 arrays at the slicer's rate, or WAV files of any encoding, channel count and rate audiokit/wav.py
serves: their bytes are uploaded as they are and decoded, mixed down and resampled to the slicer's rate by one launch per
input rate (hip/audio.py::ingest_pcm) into the same packed buffer.  Compressed formats (mp3, flac, ogg) still need a
decoder in front."""
import os
import time
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

SLICE_RATE = 32000          # AudioService.slicer loads, slices and writes at this rate


@dataclass(frozen=True)
class SlicerParams:
    """Slicer.__init__ (slicer.py:17-31): the arguments in dB / milliseconds, and what it derives from them with Python's
    round -- hop and win in samples, min_length / min_interval / max_sil_kept in frames, the threshold as a linear level"""
    sr: int = SLICE_RATE
    threshold: float = -34.0
    min_length: int = 4000
    min_interval: int = 300
    hop_size: int = 10
    max_sil_kept: int = 500
    hop: int = field(init=False)
    win: int = field(init=False)
    min_length_frames: int = field(init=False)
    min_interval_frames: int = field(init=False)
    max_sil_kept_frames: int = field(init=False)
    threshold_lin: float = field(init=False)

    def __post_init__(self):
        if not self.min_length >= self.min_interval >= self.hop_size:
            raise ValueError("The following condition must be satisfied: min_length >= min_interval >= hop_size")
        if not self.max_sil_kept >= self.hop_size:
            raise ValueError("The following condition must be satisfied: max_sil_kept >= hop_size")
        sr = self.sr
        min_interval = sr * self.min_interval / 1000
        hop = round(sr * self.hop_size / 1000)
        derived = dict(hop=hop, win=min(round(min_interval), 4 * hop),
                       min_length_frames=round(sr * self.min_length / 1000 / hop),
                       min_interval_frames=round(min_interval / hop),
                       max_sil_kept_frames=round(sr * self.max_sil_kept / 1000 / hop),
                       threshold_lin=10 ** (self.threshold / 20.0))
        for k, v in derived.items():
            object.__setattr__(self, k, v)

    def too_short(self, n_samples) -> bool:
        """slicer.py:48: the reference compares the SAMPLE count with min_length in frames and hands such a recording back
        unsliced (the service then writes nothing for it)"""
        return n_samples <= self.min_length_frames


def silence_tags(rms, params):
    """rms: the float32 frames of one recording -> the reference's sil_tags (slicer.py:53-131), a list of (begin, end)
    frame pairs of the silence that is cut out.

    The reference's frame loop only acts at the first loud frame behind a silent run, so the frames are run-length encoded
    and the runs walked; the argmin calls run on the same sub-windows of rms (numpy's argmin: the first minimum wins).
    `rms < threshold` is taken in float32 -- what NumPy 2 does with a float32 scalar against a Python float, and what the
    goldens record.  Kept as they are: the leading-silence tag (0, pos) and the trailing tag (pos, frames + 1)."""
    rms = np.ascontiguousarray(rms, dtype=np.float32)
    frames = rms.shape[0]
    silent = rms < np.float32(params.threshold_lin)
    edge = np.flatnonzero(silent[1:] != silent[:-1]) + 1
    bounds = np.concatenate(([0], edge, [frames]))
    first = 0 if frames and silent[0] else 1             # runs alternate: silent ones are every second
    keep, min_interval, min_length = params.max_sil_kept_frames, params.min_interval_frames, params.min_length_frames
    tags, clip_start = [], 0
    for k in range(first, len(bounds) - 1, 2):
        start, i = int(bounds[k]), int(bounds[k + 1])    # silent frames [start, i); frame i is loud, or i == frames
        if i == frames:                                   # trailing silence
            if frames - start >= min_interval:
                end = min(frames, start + keep)
                tags.append((int(rms[start:end + 1].argmin()) + start, frames + 1))
            break
        leading = start == 0 and i > keep
        middle = i - start >= min_interval and i - clip_start >= min_length
        if not leading and not middle:
            continue
        if i - start <= keep:
            pos = int(rms[start:i + 1].argmin()) + start
            tags.append((0, pos) if start == 0 else (pos, pos))
            clip_start = pos
            continue
        pos_l = int(rms[start:start + keep + 1].argmin()) + start
        pos_r = int(rms[i - keep:i + 1].argmin()) + i - keep
        if i - start <= keep * 2 and start != 0:
            pos = int(rms[i - keep:start + keep + 1].argmin()) + i - keep
            pos_l, pos_r = min(pos_l, pos), max(pos_r, pos)
        tags.append((0, pos_r) if start == 0 else (pos_l, pos_r))
        clip_start = pos_r
    return tags


def chunk_spans(tags, n_samples, frames, hop):
    """sil_tags -> the reference's chunks (slicer.py:132-147) as (start, end, begin, n): the labels that go into the file
    name, and the samples [begin, begin + n) of the recording.  The `end` label is frame * hop and may exceed the sample
    count; the chunk itself is clipped.  No tags: one chunk, the whole recording, labelled (0, frames * hop)."""
    if not tags:
        return [(0, frames * hop, 0, n_samples)]
    cuts = []
    if tags[0][0] > 0:
        cuts.append((0, tags[0][0]))
    cuts.extend((tags[k][1], tags[k + 1][0]) for k in range(len(tags) - 1))
    if tags[-1][1] < frames:
        cuts.append((tags[-1][1], frames))
    return [(b * hop, e * hop, b * hop, max(min(n_samples, e * hop) - b * hop, 0)) for b, e in cuts]


class Slice(NamedTuple):
    name: str            # "<recording>_<start>_<end>.wav", the reference's file name
    start: int
    end: int
    pcm: object          # int16 view into the call's PackedAudio, on the GPU
    peak: object         # 0-d float32 view on the GPU: the chunk's max |x| before the rescale


def slice_name(name, start, end):
    return "%s_%010d_%010d.wav" % (os.path.basename(name).split(".")[0], start, end)


def _is_path(rec):
    return isinstance(rec, (str, os.PathLike))


def _check(rec):
    if not isinstance(rec, np.ndarray) or rec.dtype != np.float32 or rec.ndim != 1:
        raise ValueError("slice_batch: a recording is a 1-D float32 numpy array or the path of a wav file, got "
                         f"{type(rec).__name__}" + (f" {rec.dtype} {rec.shape}" if isinstance(rec, np.ndarray) else ""))
    return rec


def _upload(recs, device):
    """the array recordings back to back in one fp32 device buffer: one copy from pinned memory"""
    import torch

    host = torch.empty(sum(r.shape[0] for r in recs), dtype=torch.float32, pin_memory=True)
    view, pos = host.numpy(), 0
    for r in recs:
        view[pos:pos + r.shape[0]] = r
        pos += r.shape[0]
    return host.to(device, non_blocking=True)


def slice_batch(names, recordings, params=SlicerParams(), normalize_max=0.9, alpha_mix=0.25, out_dir=None, device="cuda:0",
                stats=None):
    """AudioService.slicer for a batch: names[r] names recordings[r], a 1-D float32 array at params.sr (32000, the
    service's rate) or the path of a WAV file (audiokit/wav.py: six encodings, 1 .. 8 channels, any rate hip/audio.py's
    rate_ratio serves; decoded, mixed down and resampled to params.sr on the GPU, the reference's load_audio(file, 32000)
    with the boundary hip/audio.py::load_audio_batch states; a 32 kHz PCM16 file gives the samples it always gave).
    params: one SlicerParams, or one per recording
    (recordings that share win and hop share an RMS launch: one launch for one SlicerParams).

    -> per recording (ok, [Slice(name, start, end, pcm, peak)]): pcm an int16 view into one packed device buffer (a
    hip.audio.PackedAudio at 32000, gap 0, holding every chunk of the call), bit for bit the samples the reference writes.
    With out_dir the buffer is copied to the host once and every slice written to <out_dir>/slices/<name> with
    scipy.io.wavfile.write(path, 32000, int16): the reference's bytes.

    ok = False with no slices: a recording of at most min_length (in frames, the reference's own comparison) samples,
    which the reference does not slice and its service writes nothing for; and a recording whose peak is not finite (no
    launch beyond the recordings' peak launch sees it).  Where a chunk comes out empty the reference fails on it after
    having written the chunks in front of it: those are returned, with ok = False.  An all-zero chunk, for which the
    reference casts NaN to int16 (undefined in numpy), is written as zeros.

    stats: a dict that receives upload_s and walk_s (host clock; the upload -- arrays and file bytes -- is synchronised
    for it), stage_s where files are given (their headers and the reads into page-locked memory, in front of upload_s)
    and the event pairs ingest_events / rms_events / pack_events around the three groups of launches -- the benchmark's
    hooks, no cost when None."""
    names, recordings = list(names), list(recordings)
    if len(names) != len(recordings):
        raise ValueError(f"slice_batch: {len(names)} names for {len(recordings)} recordings")
    plist = list(params) if isinstance(params, (list, tuple)) else [params] * len(names)
    if len(plist) != len(names) or not all(isinstance(p, SlicerParams) for p in plist):
        raise ValueError("slice_batch: params is one SlicerParams or one per recording")
    if any(p.sr != SLICE_RATE for p in plist):
        raise ValueError(f"slice_batch slices at {SLICE_RATE} Hz, as the service does")
    if not names:
        return []
    files = [r for r, rec in enumerate(recordings) if _is_path(rec)]
    arrays = [r for r, rec in enumerate(recordings) if not _is_path(rec)]
    for r in arrays:
        _check(recordings[r])
    lens = [0 if _is_path(rec) else rec.shape[0] for rec in recordings]
    batch = None
    if files:
        from . import wav
        from ..hip.audio import out_len, rate_ratio

        t0 = time.perf_counter()
        infos = [wav.probe(recordings[r]) for r in files]
        for r, info in zip(files, infos):                 # EvtError for a rate pair that is not served: nothing is read yet
            lens[r] = out_len(info.frames, *rate_ratio(info.rate, SLICE_RATE))
        batch = wav.stage([recordings[r] for r in files], infos=infos)
        if stats is not None:
            stats["stage_s"] = time.perf_counter() - t0
    results = [(False, []) for _ in names]
    if not any(lens):
        return results

    import torch

    from ..hip import audio as A
    from ..hip import slicer as S

    device = torch.device(device)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    t0 = time.perf_counter()
    with torch.no_grad(), torch.cuda.device(device):
        x = _upload([recordings[r] for r in arrays], device) if arrays else None
        raw_dev = A.upload_raw(batch, device) if files and any(lens[r] for r in files) else None
        if stats is not None:
            torch.cuda.synchronize()
            stats["upload_s"] = time.perf_counter() - t0
        if files:
            if stats is not None:
                stats["ingest_events"] = ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            staged, x = x, torch.empty(offs[-1], dtype=torch.float32, device=device)
            pos = 0
            for r in arrays:                              # arrays between files: from the staging buffer to their place
                x[offs[r]:offs[r] + lens[r]] = staged[pos:pos + lens[r]]
                pos += lens[r]
            A.ingest_pcm(batch, SLICE_RATE, device, raw_dev=raw_dev, out=x, offsets=[offs[r] for r in files])
            if stats is not None:
                ev[1].record()
        if stats is not None:
            stats["rms_events"] = ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        live = [r for r, n in enumerate(lens) if n >= 1]
        peaks = S.span_peaks(x, S.Spans(x, [offs[r] for r in live], [lens[r] for r in live])).cpu().numpy()
        todo = [r for r, pk in zip(live, peaks) if np.isfinite(pk) and not plist[r].too_short(lens[r])]
        groups = {}
        for r in todo:
            groups.setdefault((plist[r].win, plist[r].hop), []).append(r)
        launched = [(rs, S.rms_frames_rows(x, [offs[r] for r in rs], [lens[r] for r in rs], win, hop))
                    for (win, hop), rs in groups.items()]
        if stats is not None:
            ev[1].record()
        frames_of = {}
        for rs, (rms, frame_off) in launched:
            rms = rms.cpu().numpy()
            for k, r in enumerate(rs):
                frames_of[r] = rms[frame_off[k]:frame_off[k + 1]]
        t1 = time.perf_counter()
        chunks = []                                       # (recording, start label, end label, offset in x, samples)
        ok = [False] * len(names)
        for r in todo:
            p, rms = plist[r], frames_of[r]
            spans = chunk_spans(silence_tags(rms, p), lens[r], rms.shape[0], p.hop)
            ok[r] = True
            for start, end, begin, n in spans:
                if n == 0:
                    ok[r] = False
                    break
                chunks.append((r, start, end, offs[r] + begin, n))
        if stats is not None:
            stats["walk_s"] = time.perf_counter() - t1
            stats["chunks"] = len(chunks)
        if not chunks:
            return [(ok[r], []) for r in range(len(names))]
        if stats is not None:
            stats["pack_events"] = ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        table = S.Spans(x, [c[3] for c in chunks], [c[4] for c in chunks])
        peak = S.span_peaks(x, table)
        c1, c2 = np.float32(float(normalize_max) * float(alpha_mix)), np.float32(1 - float(alpha_mix))
        packed = A.PackedAudio(S.slice_pack(x, table, peak, float(c1), float(c2)), table.dst, table.n, SLICE_RATE, 0)
        if stats is not None:
            ev[1].record()
        out = [[] for _ in names]
        for k, (r, start, end, _, _) in enumerate(chunks):
            out[r].append(Slice(slice_name(names[r], start, end), start, end, packed.row(k), peak[k]))
        if out_dir is not None:
            from scipy.io import wavfile

            os.makedirs(os.path.join(out_dir, "slices"), exist_ok=True)
            host = packed.data.cpu().numpy()
            for k, (r, start, end, _, _) in enumerate(chunks):
                wavfile.write(os.path.join(out_dir, "slices", slice_name(names[r], start, end)), SLICE_RATE,
                              host[packed.offsets[k]:packed.offsets[k] + packed.lengths[k]])
    return [(ok[r], out[r]) for r in range(len(names))]
