"""WAV files into the slicer: the bytes uploaded raw and decoded, mixed down and resampled on the GPU (hip/audio.py::ingest_pcm,
csrc/pcm_ingest.hip) against the routes open before it (profiles/ingest_batch.json).

Workload: one hour of synthetic audio from a seed -- bursts of 2..9 s of noise separated by 0.2..1.2 s of low noise, the
second channel of a stereo file at half the level -- as 6 recordings written to temporary files, in three forms: 32 kHz mono
PCM16, 48 kHz stereo PCM16, 44.1 kHz stereo 24-bit.

  (a) 32 kHz mono PCM16 through audiokit.slicer.slice_batch:
        files    the paths handed to slice_batch: bytes staged in page-locked memory, one upload, one ingest launch;
        parent   what slice_batch did with a path before ingest existed: train/dataset.py::read_wav_pcm16 per file on the
                 host (int16 -> float32), then the float32 arrays through slice_batch (that half is unchanged code).
      Both must give the same slices, checked on the warm-up pass.
  (b) 48 kHz stereo PCM16 and 44.1 kHz stereo 24-bit through slice_batch:
        files    as above;
        host     the route open before: numpy decode and channel mean, scipy.signal.resample_poly to 32 kHz, slice_batch on
                 the arrays.  Another resampling filter: the slices are not the same samples, the chunk counts are reported.
  (c) the ingest launch alone for the three forms, the bytes already on the device: device events around ingest_pcm.

Protocol: every mode runs once untimed, then --reps passes with the modes alternated; a pass is timed on the host clock from
the paths to a device synchronisation behind slice_batch.  Reported: median, min and max.  Inside the passes: stage_s (headers
and file reads into page-locked memory), upload_s (host clock, synchronised), ingest_ms / rms_ms / pack_ms (device events).
The files were just written: they are read from the page cache, not from a disk.  A measurement path without a GPU fails.

    python tools/bench_ingest.py [--reps 3] [--seconds 3600] [--out profiles/ingest_batch.json]
"""
import argparse
import hashlib
import json
import math
import os
import struct
import sys
import tempfile
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NREC = 6
FORMS = [("32000 Hz mono s16", 32000, 1, 16), ("48000 Hz stereo s16", 48000, 2, 16), ("44100 Hz stereo s24", 44100, 2, 24)]


def recording(seconds, rate, seed):
    rng = np.random.default_rng(seed)
    total = int(seconds * rate)
    x = np.empty(total, dtype=np.float32)
    pos = 0
    while pos < total:
        for lo, hi, amp in ((2.0, 9.0, 0.3), (0.2, 1.2, 2e-3)):
            n = min(int(rng.uniform(lo, hi) * rate), total - pos)
            x[pos:pos + n] = rng.uniform(-amp, amp, n).astype(np.float32)
            pos += n
    return x


def write_wav(path, x, rate, channels, bits):
    """x: float32 mono in (-1, 1) -> a PCM file; the second channel is the first at half the level"""
    q = np.round(x * np.float32(2 ** (bits - 1) - 1)).astype(np.int32)
    if channels == 2:
        q = np.stack([q, q // 2], axis=1)
    data = q.astype("<i2").tobytes() if bits == 16 else np.ascontiguousarray(q.astype("<i4")).reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    block = channels * bits // 8
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * block, block, bits) + b"data" + struct.pack("<I", len(data)))
        f.write(data)
    return len(data)


def host_decode(path, channels, bits):
    """the numpy decode and channel mean of the route before: the data chunk of the files write_wav makes"""
    with open(path, "rb") as f:
        blob = f.read()
    body = np.frombuffer(blob, dtype=np.uint8, offset=44)
    if bits == 16:
        v = body.view("<i2").astype(np.float32) * np.float32(2.0 ** -15)
    else:
        b = body.reshape(-1, 3).astype(np.int32)
        v = (((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) ^ 0x800000) - 0x800000).astype(np.float32) * np.float32(2.0 ** -23)
    return v.reshape(-1, channels).mean(axis=1, dtype=np.float32) if channels > 1 else v


def digest(results):
    h = hashlib.sha256()
    for _ok, slices in results:
        for s in slices:
            h.update(s.name.encode())
            h.update(s.pcm.cpu().numpy().tobytes())
    return h.hexdigest()


def stat(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def ms(pair):
    return pair[0].elapsed_time(pair[1])


def sliced(names, recs):
    """one slice_batch pass with its parts; ends in a device synchronisation"""
    from easevoice_trainer_amd.audiokit.slicer import slice_batch

    st = {}
    res = slice_batch(names, recs, stats=st)
    torch.cuda.synchronize()
    parts = {"upload_s": st["upload_s"], "walk_s": st["walk_s"], "rms_ms": ms(st["rms_events"]), "pack_ms": ms(st["pack_events"])}
    if "ingest_events" in st:
        parts.update(stage_s=st["stage_s"], ingest_ms=ms(st["ingest_events"]))
    return res, parts


def alternate(modes, reps):
    """modes: {name: function -> (results, parts)}; one untimed pass of each, then reps alternated passes"""
    first = {k: fn()[0] for k, fn in modes.items()}
    times, parts = {k: [] for k in modes}, {k: {} for k in modes}
    for _ in range(reps):
        for k, fn in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _res, p = fn()
            times[k].append(time.perf_counter() - t0)
            for name, v in p.items():
                parts[k].setdefault(name, []).append(v)
    return first, {k: {"seconds": stat(times[k]), "parts": {n: stat(v) for n, v in parts[k].items()}} for k in modes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_ingest needs a GPU: nothing is measured without one")
    from scipy.signal import resample_poly

    from easevoice_trainer_amd.audiokit import wav
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.train.dataset import read_wav_pcm16

    names = [f"rec{k:02d}.wav" for k in range(NREC)]
    doc = {"tool": "tools/bench_ingest.py", "device": torch.cuda.get_device_name(0), "audio_seconds": args.seconds,
           "recordings": NREC, "reps": args.reps,
           "timing": "host clock per pass from the paths to a device synchronisation behind slice_batch; modes alternated, one "
                     "untimed pass of each first; median / min / max.  parts: stage_s (headers + file reads into page-locked "
                     "memory, from the page cache), upload_s (host clock, synchronised), walk_s, ingest_ms / rms_ms / pack_ms by "
                     "device events; host routes add decode_s and resample_s on the host clock.  kernel_alone: device events "
                     "around ingest_pcm with the bytes already on the device",
           "slice_batch": [], "kernel_alone": []}
    with tempfile.TemporaryDirectory() as tmp:
        for label, rate, channels, bits in FORMS:
            paths, nbytes = [], 0
            for k in range(NREC):
                paths.append(os.path.join(tmp, f"{rate}_{k}.wav"))
                nbytes += write_wav(paths[-1], recording(args.seconds / NREC, rate, 41 + k), rate, channels, bits)

            def files():
                return sliced(names, paths)

            if rate == 32000:
                def before():
                    t0 = time.perf_counter()
                    recs = [read_wav_pcm16(p, 32000) for p in paths]
                    t1 = time.perf_counter()
                    res, parts = sliced(names, recs)
                    return res, dict(parts, decode_s=t1 - t0)
                other, baseline = "parent", ("read_wav_pcm16 per file on the host, then slice_batch on the float32 arrays: what "
                                             "slice_batch ran for a path before ingest existed")
            else:
                up, down = 32000 // math.gcd(rate, 32000), rate // math.gcd(rate, 32000)

                def before():
                    t0 = time.perf_counter()
                    recs = [host_decode(p, channels, bits) for p in paths]
                    t1 = time.perf_counter()
                    recs = [resample_poly(r, up, down).astype(np.float32) for r in recs]
                    t2 = time.perf_counter()
                    res, parts = sliced(names, recs)
                    return res, dict(parts, decode_s=t1 - t0, resample_s=t2 - t1)
                other, baseline = "host", "numpy decode and channel mean, scipy.signal.resample_poly to 32 kHz, slice_batch on the arrays"
            first, modes = alternate({"files": files, other: before}, args.reps)
            chunks = {k: sum(len(s) for _ok, s in r) for k, r in first.items()}
            run = {"input": label, "file_bytes": nbytes, "fp32_bytes_at_32k": int(args.seconds * 32000) * 4, "baseline": baseline,
                   "chunks": chunks, "modes": modes}
            if rate == 32000:
                run["same_slices"] = digest(first["files"]) == digest(first[other])
                if not run["same_slices"]:
                    raise RuntimeError("32 kHz PCM16 files: the ingest path and the parent's path give different slices")
            run["ratio_other_over_files"] = round(modes[other]["seconds"]["median"] / modes["files"]["seconds"]["median"], 2)
            doc["slice_batch"].append(run)
            del first
            # (c) the launch alone
            batch = wav.stage(paths)
            raw_dev = audio.upload_raw(batch, "cuda:0")
            audio.ingest_pcm(batch, 32000, "cuda:0", raw_dev=raw_dev)
            torch.cuda.synchronize()
            took = []
            for _ in range(max(args.reps, 3)):
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
                pa = audio.ingest_pcm(batch, 32000, "cuda:0", raw_dev=raw_dev)
                ev[1].record()
                torch.cuda.synchronize()
                took.append(ms(ev))
            moved = nbytes + 4 * sum(pa.lengths)
            doc["kernel_alone"].append({"input": label, "ingest_ms": stat(took), "bytes_read_and_written": moved,
                                        "gb_per_s": round(moved / (stat(took)["median"] * 1e-3) / 1e9, 1)})
            del batch, raw_dev, pa
            torch.cuda.empty_cache()
            print(f"{label}: measured", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
