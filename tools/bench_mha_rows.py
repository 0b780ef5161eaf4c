"""The fp32 attention core of the feature extractors alone: evt_mha_rows_f32 (csrc/mha_rows.hip, the fp32 MFMA flash kernel)
against evt_mha_fwd's fp32 core (csrc/mha.hip: mha_fwd_f32) on the same resident packed [q | k | v] rows, in one process.

Shapes: HuBERT's (12 heads of 64) on the frame counts of tools/bench_feature_extract.py's 64 clips in groups of 1 / 4 / 8 / 16,
BERT's (16 heads of 64) on the token counts of tools/bench_text_features.py's 256 sentences in groups of 1 / 16 / 32; rows
sorted by length as both tools group them.  Timed with device events around the one launch per group, the two cores alternated
group by group, after one untimed pass; --reps passes, the median per group summed over the groups = milliseconds per pass
over all rows (ONE layer).  FLOPs are the algorithm's: 4 * H * D * n^2 per row of n live positions.  The largest difference
between the two outputs is reported with the times.  A measurement path without a GPU fails.

    python tools/bench_mha_rows.py [--reps 5] [--out profiles/mha_rows_stage.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mha_rows_stage.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_mha_rows needs a GPU: nothing is measured without one")
    if args.reps < 3:
        raise RuntimeError("at least 3 timed passes")
    from easevoice_trainer_amd.feature_extractor.cnhubert import HubertModel
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.enc import _mha_params
    from easevoice_trainer_amd.hip.feat import mha_rows_launch

    dev = torch.device("cuda:0")
    rnd = random.Random(17)                                        # bench_feature_extract.workload's lengths
    frames = sorted(HubertModel.frames(int(rnd.uniform(2.0, 10.0) * 32000) // 2) for _ in range(64))
    rnd = random.Random(23)                                        # bench_text_features.workload's: characters + [CLS] + [SEP]
    tokens = sorted(rnd.randint(5, 120) + 2 for _ in range(256))
    res = {"tool": "tools/bench_mha_rows.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "device events per group, cores alternated, median over reps, summed over the groups: ms per pass over all "
                     "rows of ONE layer", "shapes": {}}
    for tag, heads, lengths, batches in (("hubert_h12_d64", 12, frames, (1, 4, 8, 16)), ("bert_h16_d64", 16, tokens, (1, 16, 32))):
        Cc, D = heads * 64, 64
        flop = sum(4.0 * heads * D * n * n for n in lengths)
        out = {"rows": len(lengths), "positions": sum(lengths), "gflop_per_pass": round(flop / 1e9, 2)}
        for kgrp in batches:
            groups = []
            for i in range(0, len(lengths), kgrp):
                ln = lengths[i:i + kgrp]
                qkv = torch.randn(len(ln), max(ln), 3 * Cc, device=dev)
                groups.append((qkv, torch.tensor(ln, dtype=torch.int32).to(dev)))

            def old(qkv, lens):      # as RelSelfAttnFn.forward calls it: the output and the lse row are allocated per call
                B, T, _ = qkv.shape
                o, lse = torch.empty(B, T, Cc, device=dev), torch.empty(B * heads, T, device=dev)
                prm = _mha_params(torch.float32, B, heads, D, T, T, None, 1, 3 * Cc, 3 * Cc, Cc, D ** -0.5, 0.0, 0, dev)
                base = qkv.data_ptr()
                L.check(L.lib().evt_mha_fwd(C.byref(prm), base, base + 4 * Cc, base + 8 * Cc, None, None, lens.data_ptr(),
                                            lens.data_ptr(), o.data_ptr(), lse.data_ptr(), L.stream_ptr()), "evt_mha_fwd")
                return o

            def new(qkv, lens):      # as hip/enc.py's route calls it
                B, T, _ = qkv.shape
                base = qkv.data_ptr()
                return mha_rows_launch(base, base + 4 * Cc, base + 8 * Cc, lens, lens, B, T, T, heads, D, 3 * Cc, 3 * Cc,
                                       D ** -0.5, dev)

            times = {"old": [[] for _ in groups], "new": [[] for _ in groups]}
            diff = 0.0
            with torch.no_grad():
                for rep in range(args.reps + 1):
                    for gi, g in enumerate(groups):
                        got = {}
                        for name, fn in (("old", old), ("new", new)) if rep % 2 else (("new", new), ("old", old)):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            got[name] = fn(*g)
                            e1.record()
                            torch.cuda.synchronize()
                            if rep:
                                times[name][gi].append(e0.elapsed_time(e1))
                        if not rep:
                            diff = max(diff, float((got["old"] - got["new"]).abs().max()))
            ms = {name: sum(sorted(t)[len(t) // 2] for t in ts) for name, ts in times.items()}
            narrow = [gi for gi, g in enumerate(groups) if g[0].size(1) <= 64]      # groups of one query tile
            ms_narrow = {name: sum(sorted(ts[gi])[len(ts[gi]) // 2] for gi in narrow) for name, ts in times.items()}
            out[f"group{kgrp}"] = {
                "old_ms": round(ms["old"], 3), "new_ms": round(ms["new"], 3), "old_over_new": round(ms["old"] / ms["new"], 2),
                "new_ms_min_max": [round(sum(min(t) for t in times["new"]), 3), round(sum(max(t) for t in times["new"]), 3)],
                "old_ms_min_max": [round(sum(min(t) for t in times["old"]), 3), round(sum(max(t) for t in times["old"]), 3)],
                "groups_up_to_64_wide": {"groups": len(narrow), "old_ms": round(ms_narrow["old"], 3),
                                         "new_ms": round(ms_narrow["new"], 3)},
                "new_tflops": round(flop / ms["new"] / 1e9, 2), "max_abs_diff_old_new": diff}
            del groups
            torch.cuda.empty_cache()
        res["shapes"][tag] = out
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
