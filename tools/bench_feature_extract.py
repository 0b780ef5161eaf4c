"""Throughput of the `ssl` step of the data-set normalisation (CN-HuBERT content features): FeatureWriter.ssl one clip at a
time -- peak, rescale and the 255-tap half-band filter on the host, then a single-row pass of the model -- against
FeatureWriter.ssl_batch on groups of 1, 4, 8 and 16 clips (rescale and resampling on the GPU, one ragged pass of the model
per group), in the same process.

Workload: 64 synthetic 32 kHz clips of 2..10 s (seeded lengths, uniform noise of peak 0.5), the base HuBERT architecture with
random-init weights, bf16 and fp32.  For the batched modes the clips are sorted by length, so that a group pads little; the
one-at-a-time baseline takes them in the same order.  Every pass writes its 64 feature files and 64 wav files into a fresh
temporary directory (an existing file would be skipped), so the file writes are in every mode's time.

Protocol: every mode runs once untimed (all its shapes are then warm), then --reps timed passes with the modes alternated;
a pass is timed on the host clock between two device synchronisations, because the baseline's time is mostly host work.
Reported per mode: the median pass, clips/s and the spread (min / max seconds).  The yardstick is the `ssl` line of the same
run and dtype.  `host_front_seconds` is the host part of the baseline alone (rescale_clip + resample_half over the 64 clips).
The first layer is timed on its own with device events on the 16 kHz rows of every group: evt_hubert_front_rows (five
launches, the convolution never stored) against the parent's convolution + evt_channel_norm_gelu_fwd row by row.
A measurement path without a GPU fails.

    python tools/bench_feature_extract.py [--reps 3] [--clips 64] [--out profiles/hubert_batch.json]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(n, seed=17):
    rnd = random.Random(seed)
    rs = np.random.RandomState(seed)
    clips = [(rs.rand(int(rnd.uniform(2.0, 10.0) * 32000)) - 0.5).astype(np.float32) for _ in range(n)]
    return sorted(clips, key=len)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_feature_extract needs a GPU: nothing is measured without one")
    from easevoice_trainer_amd.feature_extractor import CNHubert
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter, resample_half, rescale_clip
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.feat import hubert_front_rows

    dev = torch.device("cuda:0")
    clips = workload(args.clips)
    names = [f"clip{i:03d}.wav" for i in range(len(clips))]
    audio_s = sum(len(c) for c in clips) / 32000.0
    t0 = time.perf_counter()
    rows16 = [resample_half(rescale_clip(c)[1]) for c in clips]
    host_front = time.perf_counter() - t0
    res = {"tool": "tools/bench_feature_extract.py", "device": torch.cuda.get_device_name(0), "clips": len(clips),
           "audio_seconds": round(audio_s, 2), "clip_seconds_min_max": [round(len(clips[0]) / 32000, 2), round(len(clips[-1]) / 32000, 2)],
           "reps": args.reps, "timing": "host clock between device synchronisations per pass, modes alternated, one untimed "
                                        "pass of every mode first; medians",
           "baseline": "modes.ssl of the same run and dtype: FeatureWriter.ssl one clip at a time",
           "host_front_seconds": round(host_front, 3), "dtypes": {}}
    for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        torch.manual_seed(0)
        hub = CNHubert(None, dev, dtype)

        def run_one():
            with tempfile.TemporaryDirectory() as d:
                w = FeatureWriter(d, hub, None)
                return [w.ssl(n, c) for n, c in zip(names, clips)]

        def run_batch(k):
            with tempfile.TemporaryDirectory() as d:
                w = FeatureWriter(d, hub, None)
                out = []
                for i in range(0, len(clips), k):
                    out += w.ssl_batch(names[i:i + k], clips[i:i + k])
                return out

        modes = [("ssl", run_one)] + [(f"ssl_batch{k}", (lambda k=k: run_batch(k))) for k in args.batches]
        for name, fn in modes:
            assert all(fn()), name
            torch.cuda.synchronize()
        times = {name: [] for name, _ in modes}
        for _ in range(args.reps):
            for name, fn in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
                print(f"{tag} {name}: {times[name][-1]:.3f} s", file=sys.stderr, flush=True)
        out = {"modes": {}}
        for name, _ in modes:
            v = sorted(times[name])
            med = _median(v)
            out["modes"][name] = {"seconds_median": round(med, 4), "seconds_min": round(v[0], 4), "seconds_max": round(v[-1], 4),
                                  "clips_per_s": round(len(clips) / med, 1), "audio_s_per_s": round(audio_s / med, 1)}
        base = out["modes"]["ssl"]["seconds_median"]
        for m in out["modes"].values():
            m["ratio_vs_ssl"] = round(base / m["seconds_median"], 3)
        out["host_front_share_of_ssl"] = round(host_front / base, 3)
        # the first layer alone on the 16 kHz rows of every group: device events, median over groups and reps
        L.set_half(dtype)
        first = hub.model.feature_extractor.conv_layers[0]
        wgt = first.conv.weight.data.view(512, 10)
        front = {}
        with torch.no_grad():
            for k in args.batches:
                groups = []
                for i in range(0, len(rows16), k):
                    rs = rows16[i:i + k]
                    x = torch.zeros(len(rs), max(len(r) for r in rs))
                    for b, r in enumerate(rs):
                        x[b, :len(r)] = torch.from_numpy(r)
                    x = x.to(dev)
                    groups.append((x, torch.tensor([len(r) for r in rs], dtype=torch.int32).to(dev),
                                   [x[b:b + 1, :len(r)].to(dtype).unsqueeze(-1).contiguous() for b, r in enumerate(rs)]))
                new_us, old_us = [], []
                for rep in range(args.reps + 1):
                    for x, lens, alone in groups:
                        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                        e[0].record()
                        hubert_front_rows(x, lens, wgt, first.layer_norm.weight.data, first.layer_norm.bias.data, 1e-5, dtype)
                        e[1].record()
                        for a in alone:
                            first(a)
                        e[2].record()
                        torch.cuda.synchronize()
                        if rep:
                            new_us.append(e[0].elapsed_time(e[1]) * 1e3)
                            old_us.append(e[1].elapsed_time(e[2]) * 1e3)
                front[f"group{k}"] = {"front_rows_us_median": round(_median(new_us), 1),
                                      "conv_plus_channel_norm_gelu_us_median": round(_median(old_us), 1)}
        out["first_layer_per_group"] = front
        res["dtypes"][tag] = out
        del hub
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
