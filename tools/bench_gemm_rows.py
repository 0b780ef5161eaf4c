"""The fp32 dense layers and strided convolutions of the feature extractors alone: evt_gemm_rows_f32 (csrc/gemm_rows.hip, bias and
GELU fused) against the route it replaces -- evt_conv1d_fwd's fp32 kernels plus evt_gelu_rows_fwd -- on the same resident
inputs and parameters, in one process.

Shapes: HuBERT's 768 -> 768, 768 -> 3072 + GELU, 3072 -> 768, 512 -> 768 and its six k 3 / k 2, stride 2 convolutions 512 -> 512
+ GELU at their layers' frame counts, for the 64 clips of tools/bench_feature_extract.py in groups of 1 / 4 / 8 / 16; BERT's
1024 -> 1024, 1024 -> 4096 + GELU, 4096 -> 1024 for the 256 sentences of tools/bench_text_features.py in groups of 1 / 16 / 32;
items sorted by length as both tools group them.  A dense layer runs over the padded [B, Tmax] rows, as the extractors run it;
a convolution takes its layer's frame counts as lens on the new route.  Timed with device events around a group's launches,
the two routes alternated group by group, after one untimed pass; --reps passes, the median per group summed over the groups =
milliseconds per pass over all items (ONE layer; the convolution classes sum their layers).  TFLOP/s count the live rows only.
The largest difference between the two outputs on live rows is reported with the times.  A measurement path without a GPU
fails.

    python tools/bench_gemm_rows.py [--reps 7] [--out profiles/gemm_rows_stage.json]
"""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_rows_stage.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_gemm_rows needs a GPU: nothing is measured without one")
    if args.reps < 3:
        raise RuntimeError("at least 3 timed passes")
    from easevoice_trainer_amd.feature_extractor.cnhubert import CONV_KERNEL, HubertModel, _ConvLayer
    from easevoice_trainer_amd.hip.enc import dense_rows
    from easevoice_trainer_amd.hip.feat import gelu_rows
    from easevoice_trainer_amd.module.attentions import linear_rows
    from easevoice_trainer_amd.runtime import ModelRuntime

    dev = torch.device("cuda:0")
    rnd = random.Random(17)                                        # bench_feature_extract.workload's lengths
    clips = sorted(int(rnd.uniform(2.0, 10.0) * 32000) // 2 for _ in range(64))
    per_layer = [HubertModel.layer_frames(n) for n in clips]       # frames behind each of the seven convolutions, per clip
    rnd = random.Random(23)                                        # bench_text_features.workload's: characters + [CLS] + [SEP]
    tokens = sorted(rnd.randint(5, 120) + 2 for _ in range(256))

    # class -> [(layer, lengths in, lengths out)]; a dense layer keeps the lengths
    dense = lambda k, n: linear_rows(k, n)    # noqa: E731
    frames = [f[-1] for f in per_layer]
    hubert = {"dense_768_768": (False, [(dense(768, 768), frames, frames)]),
              "dense_768_3072_gelu": (True, [(dense(768, 3072), frames, frames)]),
              "dense_3072_768": (False, [(dense(3072, 768), frames, frames)]),
              "dense_512_768": (False, [(dense(512, 768), frames, frames)])}
    for name, ids in (("conv_512_k3_s2_gelu", (1, 2, 3, 4)), ("conv_512_k2_s2_gelu", (5, 6))):
        hubert[name] = (True, [(_ConvLayer(512, 512, CONV_KERNEL[i], 2, False), [f[i - 1] for f in per_layer],
                                [f[i] for f in per_layer]) for i in ids])
    bert = {"dense_1024_1024": (False, [(dense(1024, 1024), tokens, tokens)]),
            "dense_1024_4096_gelu": (True, [(dense(1024, 4096), tokens, tokens)]),
            "dense_4096_1024": (False, [(dense(4096, 1024), tokens, tokens)])}
    holder = torch.nn.ModuleList(m for table in (hubert, bert) for _g, layers in table.values() for m, _i, _o in layers).eval()
    rt = ModelRuntime(holder, dtype=torch.float32, device=dev)
    rt.bank.weight_grads = False
    rt.prepare(force=True)

    def old(m, x, lens, gelu):
        if isinstance(m, _ConvLayer):
            return gelu_rows(m.conv(x))
        return gelu_rows(m(x)) if gelu else m(x)

    def new(m, x, lens, gelu):
        return m(x, lens) if isinstance(m, _ConvLayer) else dense_rows(m, x, gelu)

    res = {"tool": "tools/bench_gemm_rows.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "device events per group, routes alternated, median over reps, summed over the groups (and a class's "
                     "layers): ms per pass over all items", "shapes": {}}
    for tag, table, batches in (("hubert_64_clips", hubert, (1, 4, 8, 16)), ("bert_256_sentences", bert, (1, 16, 32))):
        for cls, (gelu, layers) in table.items():
            flop = sum(2.0 * n * (m.conv if isinstance(m, _ConvLayer) else m).weight.numel() for m, _i, lo in layers for n in lo)
            out = {"live_rows": sum(sum(lo) for _m, _i, lo in layers), "gflop_per_pass": round(flop / 1e9, 2)}
            for kgrp in batches:
                groups = []
                for m, li, lo in layers:
                    cin = (m.conv if isinstance(m, _ConvLayer) else m).cin
                    for i in range(0, len(li), kgrp):
                        x = torch.randn(len(li[i:i + kgrp]), max(li[i:i + kgrp]), cin, device=dev)
                        groups.append((m, x, torch.tensor(lo[i:i + kgrp], dtype=torch.int32).to(dev), gelu))
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
                                for b, n in enumerate(g[2].tolist()):
                                    diff = max(diff, float((got["old"][b, :n] - got["new"][b, :n]).abs().max()))
                ms = {name: sum(sorted(t)[len(t) // 2] for t in ts) for name, ts in times.items()}
                out[f"group{kgrp}"] = {
                    "old_ms": round(ms["old"], 3), "new_ms": round(ms["new"], 3), "old_over_new": round(ms["old"] / ms["new"], 2),
                    "old_ms_min_max": [round(sum(min(t) for t in times["old"]), 3), round(sum(max(t) for t in times["old"]), 3)],
                    "new_ms_min_max": [round(sum(min(t) for t in times["new"]), 3), round(sum(max(t) for t in times["new"]), 3)],
                    "old_tflops": round(flop / ms["old"] / 1e9, 2), "new_tflops": round(flop / ms["new"] / 1e9, 2),
                    "max_abs_diff_old_new": diff}
                print(tag, cls, f"group{kgrp}", json.dumps(out[f"group{kgrp}"]), flush=True)
                del groups
                torch.cuda.empty_cache()
            res["shapes"].setdefault(tag, {})[cls] = out
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
