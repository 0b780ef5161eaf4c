"""The `token` step on ragged batches, four measurements in one process (profiles/token_batch.json):

(a) `write_semantic_tsv`: the parent's path and this file's baseline -- per item a file read, an upload, the transposed copy,
    two convolution launches, evt_rvq_norms, evt_rvq_select and a synchronising .tolist().
(b) `write_semantic_tsv_batch` in groups of 1 / 4 / 8 / 16: per group the file reads, one upload of the zero-padded
    channels-last group from a page-locked buffer, ONE launch of evt_semantic_codes_rows, one read-back.  Groups are taken
    in the given order (no sorting by length), so a group pads to its longest item.  The two files are compared code by
    code (`codes_differing_from_baseline`).  `alternative_end_to_end/<k>` is a form that was tried and is kept in this
    tool only: the group's items laid end to end as [1, 768, sum] (no padding), evt_ncl_to_nlc on the device, the group
    tokenised as one row.
(c) the device-resident path: `FeatureWriter.ssl_batch` over 32 kHz clips of the same lengths in groups of 16 with and
    without tokens=True, every pass into a fresh directory; the difference is what the codes cost while the features are
    still on the device.  Random-init base HuBERT, fp32.  The passes take over a second and scatter by more than the
    difference, so the part tokens=True adds -- extract_latent_rows on the resident group and the codes' read-back -- is
    also timed alone on the same four groups (`tokens_of_resident_features_seconds`).
(d) the kernel alone, by device events: one evt_semantic_codes_rows launch per group of 16 device-resident channels-last
    items against SynthesizerTrn.extract_latent per device-resident [1, 768, T] item (the transposed copy and the four
    launches it replaces), 64 items each way.

Workload: 64 items of 2..10 s (100..500 frames of 768 random-normal features, seeded lengths, arrival order; the files are
written as CNHubert writes them: a transposed view of [1, T, 768], whose strides torch.save keeps), configs/s2.json
with random-init weights and a random codebook, fp32.  Protocol: every mode runs once untimed, then --reps passes with the
modes alternated; a pass is timed on the host clock between two synchronisations; median, min and max per mode.  A
measurement path without a GPU fails.

    python tools/bench_token_step.py [--reps 3] [--items 64] [--out profiles/token_batch.json]
"""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_s2_decode import build_voice  # noqa: E402


def stats(v, digits=4):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def alternate(modes, reps):
    for _name, fn in modes:                       # warm-up: every shape of every mode once
        fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in modes}
    for _ in range(reps):
        for name, fn in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_token_step needs a GPU: nothing is measured without one")
    from easevoice_trainer_amd.feature_extractor import CNHubert
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter
    from easevoice_trainer_amd.inference.semantic import write_semantic_tsv, write_semantic_tsv_batch

    dev = torch.device("cuda:0")
    voice = build_voice(dev, torch.float32)
    rnd = random.Random(41)
    seconds = [rnd.uniform(2.0, 10.0) for _ in range(args.items)]
    frames = [int(s * 50) for s in seconds]
    names = [f"item{i:03d}.wav" for i in range(args.items)]
    work = tempfile.mkdtemp(prefix="token_step_")
    doc = {"tool": "tools/bench_token_step.py", "device": torch.cuda.get_device_name(0), "items": args.items,
           "frames_min_max": [min(frames), max(frames)], "codes": sum(t // 2 for t in frames), "reps": args.reps,
           "clock": "host (perf_counter between synchronisations); kernel_alone by device events",
           "baseline": "write_semantic_tsv: one item at a time (the parent's path) on the same files"}
    try:
        # ---- (a), (b): from feature files ----
        hdir = os.path.join(work, "4-cnhubert")
        os.makedirs(hdir)
        g = torch.Generator().manual_seed(42)
        for n, t in zip(names, frames):
            torch.save(torch.randn(1, t, 768, generator=g).transpose(1, 2), os.path.join(hdir, n + ".pt"))
        one = lambda: write_semantic_tsv(voice.extract_latent, names, hdir, os.path.join(work, "one.tsv"), device=dev)
        modes = [("write_semantic_tsv", one)]
        for k in args.groups:
            modes.append((f"write_semantic_tsv_batch/{k}", lambda k=k: write_semantic_tsv_batch(
                voice.extract_latent_rows, names, hdir, os.path.join(work, f"rows{k}.tsv"), group=k, device=dev)))

        def end_to_end(k):
            from easevoice_trainer_amd.hip.frontend import ncl_to_nlc
            from easevoice_trainer_amd.inference.semantic import codes_to_host

            out, stage = [], None
            for i in range(0, len(names), k):
                fs = [torch.load(os.path.join(hdir, n + ".pt"), map_location="cpu").float() for n in names[i:i + k]]
                starts, total = [], 0
                for f in fs:
                    starts.append(total)
                    total += f.size(2) + (f.size(2) & 1)
                if stage is None or stage.numel() < 768 * total:
                    stage = torch.empty(768 * total, dtype=torch.float32, pin_memory=True)
                host = stage[: 768 * total].view(1, 768, total)
                for f, at in zip(fs, starts):
                    host[0, :, at: at + f.size(2)] = f[0]
                    if f.size(2) & 1:
                        host[0, :, at + f.size(2)] = 0.0
                with torch.no_grad():
                    flat = codes_to_host(voice.extract_latent_rows(ncl_to_nlc(host.to(dev)), [total]))[0]
                out.extend(flat[at // 2: at // 2 + f.size(2) // 2] for f, at in zip(fs, starts))
            return out

        for k in args.groups:
            modes.append((f"alternative_end_to_end/{k}", lambda k=k: end_to_end(k)))
        times = alternate(modes, args.reps)
        base = stats(times["write_semantic_tsv"])["median"]
        want = open(os.path.join(work, "one.tsv")).read().split("\n")
        doc["from_files"] = {}
        for name, _ in modes:
            s = stats(times[name])
            doc["from_files"][name] = {"seconds": s, "items_per_s": round(args.items / s["median"], 1),
                                       "ratio_vs_baseline": round(base / s["median"], 3)}
        for k in args.groups:
            got = open(os.path.join(work, f"rows{k}.tsv")).read().split("\n")
            codes = sum(len(a.split(" ")) for a in want[1:-1])
            diff = sum(int(x != y) for a, b in zip(want[1:-1], got[1:-1]) for x, y in zip(a.split(" "), b.split(" ")))
            doc["from_files"][f"write_semantic_tsv_batch/{k}"]["codes_differing_from_baseline"] = [diff, codes]

        # ---- (c): behind ssl_batch ----
        hub = CNHubert(None, dev, torch.float32)
        rs = np.random.RandomState(43)
        clips = [((rs.rand(int(s * 32000)) - 0.5) * 1.2).astype(np.float32) for s in seconds]
        count = [0]

        def ssl_pass(tokens):
            count[0] += 1
            d = os.path.join(work, f"pass{count[0]}")
            fw = FeatureWriter(d, hub, None, voice=voice)
            for i in range(0, len(names), 16):
                fw.ssl_batch(names[i:i + 16], clips[i:i + 16], tokens=tokens)
            if tokens:
                fw.write_semantic(names)
            torch.cuda.synchronize()
            shutil.rmtree(d)

        times = alternate([("ssl_batch", lambda: ssl_pass(False)), ("ssl_batch_tokens", lambda: ssl_pass(True))], args.reps)
        a, b = stats(times["ssl_batch"]), stats(times["ssl_batch_tokens"])
        doc["behind_ssl_batch"] = {"group": 16, "ssl_batch": {"seconds": a}, "ssl_batch_tokens_and_write_semantic": {"seconds": b},
                                   "added_seconds_median": round(b["median"] - a["median"], 4),
                                   "baseline_token_step_seconds_median": base}

        # ---- (d): the kernel alone ----
        feats = [torch.load(os.path.join(hdir, n + ".pt")).to(dev) for n in names]               # [1, 768, T]
        groups = []
        for i in range(0, len(feats), 16):
            fr = frames[i:i + 16]
            hs = torch.zeros(len(fr), max(fr), 768, device=dev)
            for b_, f in enumerate(feats[i:i + 16]):
                hs[b_, :fr[b_]] = f[0].t()
            groups.append((hs, fr))
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def timed(fn):
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        with torch.no_grad():
            rows = lambda: [voice.extract_latent_rows(hs, fr) for hs, fr in groups]
            four = lambda: [voice.extract_latent(f) for f in feats]
            rows(), four()
            tr, tf = [], []
            for _ in range(max(args.reps, 5)):
                tr.append(timed(rows))
                tf.append(timed(four))
        from easevoice_trainer_amd.inference.semantic import codes_to_host

        def resident():                       # what tokens=True adds inside ssl_batch: the launch and the codes' read-back
            with torch.no_grad():
                for hs, fr in groups:
                    codes_to_host(voice.extract_latent_rows(hs, fr))

        doc["behind_ssl_batch"]["tokens_of_resident_features_seconds"] = stats(alternate([("r", resident)], max(args.reps, 5))["r"], 5)
        doc["kernel_alone_ms"] = {"semantic_codes_rows_4_groups_of_16": stats(tr, 3), "extract_latent_64_items": stats(tf, 3),
                                  "ratio": round(stats(tf, 3)["median"] / stats(tr, 3)["median"], 2)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
