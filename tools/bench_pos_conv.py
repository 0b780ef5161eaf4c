"""The positional-convolution stage of CN-HuBERT alone (HubertModel.encoder.pos_conv_embed: grouped conv 768 -> 768, k = 128,
16 groups, + bias + GELU), on the frame counts of tools/bench_feature_extract.py's 64 clips, in groups of 1 / 4 / 8 / 16.

Timed with device events around the stage's launches per group, after one untimed pass over all groups; --reps passes, the
median per group summed over the groups = milliseconds per 64 clips.  FLOPs are the algorithm's: 2 * frames * 768 * 48 * 128
per clip (live frames only).  The script runs on any tree of this project (--root): on one whose stage takes no frame counts
it calls the one-argument form, so that two trees can be compared in one call, alternated by the caller.
A measurement path without a GPU fails.

    python tools/bench_pos_conv.py [--root .] [--reps 5] [--out pos_conv.json]
"""
import argparse
import inspect
import json
import os
import random
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_pos_conv needs a GPU: nothing is measured without one")
    sys.path.insert(0, os.path.abspath(args.root))
    from easevoice_trainer_amd.feature_extractor import CNHubert
    from easevoice_trainer_amd.feature_extractor.cnhubert import HubertModel
    from easevoice_trainer_amd.hip import lib as L

    dev = torch.device("cuda:0")
    rnd = random.Random(17)                                        # bench_feature_extract.workload's lengths
    frames = sorted(HubertModel.frames(int(rnd.uniform(2.0, 10.0) * 32000) // 2) for _ in range(args.clips))
    flop = sum(2.0 * t * 768 * 48 * 128 for t in frames)
    res = {"tool": "tools/bench_pos_conv.py", "root": os.path.abspath(args.root), "device": torch.cuda.get_device_name(0),
           "clips": len(frames), "frames": sum(frames), "gflop_per_pass": round(flop / 1e9, 1), "reps": args.reps,
           "timing": "device events per group, median over reps, summed over the groups", "dtypes": {}}
    for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        torch.manual_seed(0)
        hub = CNHubert(None, dev, dtype)
        stage = hub.model.encoder.pos_conv_embed
        ragged = "lens" in inspect.signature(stage.forward).parameters
        L.set_half(dtype)
        out = {"ragged_entry": ragged}
        with torch.no_grad():
            for k in args.batches:
                groups = []
                for i in range(0, len(frames), k):
                    fl = frames[i:i + k]
                    x = (0.5 * torch.randn(len(fl), max(fl), 768, device=dev)).to(dtype)
                    for b, t in enumerate(fl):
                        x[b, t:] = 0
                    groups.append((x, torch.tensor(fl, dtype=torch.int32).to(dev)))
                times = [[] for _ in groups]
                for rep in range(args.reps + 1):
                    for gi, (x, lens) in enumerate(groups):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        stage(x, lens) if ragged else stage(x)
                        e1.record()
                        torch.cuda.synchronize()
                        if rep:
                            times[gi].append(e0.elapsed_time(e1))
                ms = sum(sorted(t)[len(t) // 2] for t in times)
                lo, hi = sum(min(t) for t in times), sum(max(t) for t in times)
                out[f"group{k}"] = {"ms_per_pass": round(ms, 3), "ms_min_max": [round(lo, 3), round(hi, 3)],
                                    "tflops": round(flop / ms / 1e9, 2)}
        res["dtypes"][tag] = out
        del hub
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
