"""The audio slicer on ragged batches of recordings against a numpy host path (profiles/slicer_batch.json).

Workload: one hour of synthetic audio at 32 kHz from a seed -- bursts of 2..9 s of noise separated by 0.2..1.2 s of low
noise -- cut into 1, 6 and 60 recordings of equal length.  Two modes per split, both without file writes:

  gpu   audiokit.slicer.slice_batch: one upload of the packed buffer, the recordings' peaks and RMS frames on the GPU, the tag
        walk on the host, every chunk's peak and rescale-and-pack on the GPU.  Inside a pass the upload is timed on the host
        clock (synchronised), the two groups of launches by device events, the tag walk on the host clock.
  host  the way before it, written here in numpy: per recording a strided-window mean of squares (the [win, frames]
        float32 temporary), a Python loop over the frames, and the rescale and int16 cast per chunk.

Protocol: every mode runs once untimed, then --reps passes with the modes alternated; a pass is timed on the host clock and,
for `gpu`, ends in a device synchronisation.  Reported per mode: median, min and max seconds of a pass.  The two modes must
give the same chunks and the same int16 samples: checked on the warm-up pass, a difference is an error.  A measurement path
without a GPU fails.

    python tools/bench_slicer.py [--reps 3] [--seconds 3600] [--out profiles/slicer_batch.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 32000


def workload(seconds, seed=41):
    rng = np.random.default_rng(seed)
    total = int(seconds * SR)
    x = np.empty(total, dtype=np.float32)
    pos = 0
    while pos < total:
        for lo, hi, amp in ((2.0, 9.0, 0.3), (0.2, 1.2, 2e-3)):
            n = min(int(rng.uniform(lo, hi) * SR), total - pos)
            x[pos:pos + n] = rng.uniform(-amp, amp, n).astype(np.float32)
            pos += n
    return x


def host_rms(x, win, hop):
    """one windowed energy per hop, the window centred: a [win, frames] view of the padded signal, squared and averaged"""
    y = np.pad(x, (win // 2, win // 2))
    frames = (y.shape[0] - win) // hop + 1
    view = np.lib.stride_tricks.as_strided(y, shape=(win, frames), strides=(y.strides[0], hop * y.strides[0]))
    return np.sqrt(np.mean(np.abs(view) ** 2, axis=0))


def host_tags(rms, p):
    """the slicer's cut points, one frame at a time: a silent run that ends is cut where it is quietest if it is long enough
    and the clip in front of it is; long runs keep max_sil_kept frames of silence on both sides"""
    thr, keep = np.float32(p.threshold_lin), p.max_sil_kept_frames
    tags, run, clip = [], None, 0
    for i, level in enumerate(rms):
        if level < thr:
            if run is None:
                run = i
            continue
        if run is None:
            continue
        start, run = run, None
        if not ((start == 0 and i > keep) or (i - start >= p.min_interval_frames and i - clip >= p.min_length_frames)):
            continue
        if i - start <= keep:
            lo = hi = int(rms[start:i + 1].argmin()) + start
        else:
            lo = int(rms[start:start + keep + 1].argmin()) + start
            hi = int(rms[i - keep:i + 1].argmin()) + i - keep
            if i - start <= 2 * keep and start:
                mid = int(rms[i - keep:start + keep + 1].argmin()) + i - keep
                lo, hi = min(lo, mid), max(hi, mid)
        tags.append((0 if start == 0 else lo, hi))
        clip = hi
    frames = len(rms)
    if run is not None and frames - run >= p.min_interval_frames:
        tags.append((int(rms[run:min(frames, run + keep) + 1].argmin()) + run, frames + 1))
    return tags


def host_slice(names, recs, p, normalize_max=0.9, alpha_mix=0.25):
    from easevoice_trainer_amd.audiokit.slicer import chunk_spans, slice_name

    out = []
    for name, x in zip(names, recs):
        rms = host_rms(x, p.win, p.hop)
        for start, end, begin, n in chunk_spans(host_tags(rms, p), x.shape[0], rms.shape[0], p.hop):
            chunk = x[begin:begin + n]
            peak = np.abs(chunk).max()
            if peak > 1:
                chunk = chunk / peak
            chunk = (chunk / peak * (normalize_max * alpha_mix)) + (1 - alpha_mix) * chunk
            out.append((slice_name(name, start, end), (chunk * 32767).astype(np.int16)))
    return out


def digest(slices):
    h = hashlib.sha256()
    for name, pcm in slices:
        h.update(name.encode())
        h.update(np.ascontiguousarray(pcm).tobytes())
    return h.hexdigest()


def stat(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def measure(hour, nrec, reps):
    from easevoice_trainer_amd.audiokit.slicer import SlicerParams, slice_batch

    p = SlicerParams()
    recs = np.array_split(hour, nrec)
    names = [f"rec{k:02d}.wav" for k in range(nrec)]
    seconds = hour.shape[0] / SR

    def gpu(stats=None):
        res = slice_batch(names, recs, p, stats=stats)
        torch.cuda.synchronize()
        return res

    got = gpu()                                                     # warm-up, and what the two modes compute
    assert all(ok for ok, _ in got)
    g = digest([(s.name, s.pcm.cpu().numpy()) for _, sl in got for s in sl])
    h_slices = host_slice(names, recs, p)
    if g != digest(h_slices):
        raise RuntimeError(f"{nrec} recordings: the GPU path and the host path give different slices")
    times = {"gpu": [], "host": []}
    parts = {"upload_s": [], "walk_s": [], "rms_group_ms": [], "pack_group_ms": []}
    for _ in range(reps):
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gpu(st)
        times["gpu"].append(time.perf_counter() - t0)
        parts["upload_s"].append(st["upload_s"])
        parts["walk_s"].append(st["walk_s"])
        parts["rms_group_ms"].append(st["rms_events"][0].elapsed_time(st["rms_events"][1]))
        parts["pack_group_ms"].append(st["pack_events"][0].elapsed_time(st["pack_events"][1]))
        t0 = time.perf_counter()
        host_slice(names, recs, p)
        times["host"].append(time.perf_counter() - t0)
    res = {"recordings": nrec, "chunks": len(h_slices), "slices_sha256": g[:16],
           "modes": {k: dict(seconds=stat(v), audio_seconds_per_s=round(seconds / stat(v)["median"], 1)) for k, v in times.items()},
           "gpu_parts": {k: stat(v) for k, v in parts.items()}}
    res["ratio_host_over_gpu"] = round(res["modes"]["host"]["seconds"]["median"] / res["modes"]["gpu"]["seconds"]["median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--splits", type=int, nargs="+", default=[1, 6, 60])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slicer_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_slicer needs a GPU: nothing is measured without one")
    hour = workload(args.seconds)
    doc = {"tool": "tools/bench_slicer.py", "device": torch.cuda.get_device_name(0), "audio_seconds": round(hour.shape[0] / SR, 1),
           "sample_rate": SR, "reps": args.reps,
           "timing": "host clock per pass, the gpu mode ending in a device synchronisation; modes alternated, one untimed pass "
                     "of each first; median / min / max.  gpu_parts: inside the gpu passes -- upload_s and walk_s on the host "
                     "clock (the upload synchronised), rms_group_ms (recordings' peaks + RMS frames) and pack_group_ms "
                     "(chunks' peaks + rescale and pack) by device events, which include the launches' own small uploads",
           "baseline": "modes.host of the same run: numpy strided-window mean of squares, a Python frame loop, per-chunk "
                       "rescale; no file writes in either mode",
           "runs": [measure(hour, n, args.reps) for n in args.splits]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
