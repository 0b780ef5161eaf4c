"""Reference voices on ragged batches, two measurements in one process (profiles/ref_voices.json):

(a) clip -> style vector.  `one`: one clip at a time, the way before the ragged entry points -- the host's peak and division
    (the reference's _get_ref_spec, inference/tts.py:390-409), the clip's upload, spectrogram_torch, SynthesizerTrn._style --
    against `rows<k>`: groups of k clips padded on the host, one upload, hip/audio.py::ref_spec_rows and
    SynthesizerTrn.style_rows, k = 1 / 4 / 8 / 16.  Groups are taken in the given order (no sorting by length), so a group
    pads to its longest clip.
(b) decode_batch with 16 voices.  Groups of 16 fragments (tools/bench_s2_decode.py's fragments) whose rows all have their own
    voice: `refer16` hands decode_batch 16 reference spectrograms (16 passes of the style encoder inside the call) against
    `style16`, which hands it the 16 precomputed style vectors ([16, gin]).  `shared16` (one reference for all rows: one
    pass) is timed next to them: refer16 - shared16 is what 15 style passes cost inside a group decode.

Workload: 64 clips of 3..10 s at 32 kHz (seeded lengths, uniform noise with peaks on both sides of 1 and 2), configs/s2.json
with random-init weights, bf16 and fp32.  Protocol: every mode runs once untimed, then --reps passes with the modes
alternated; a pass is timed on the host clock between two synchronisations.  Reported per mode: median, min and max seconds
of a pass and the ratio of the baseline's median to the mode's (`one` for (a), `refer16` for (b)).  A measurement path
without a GPU fails.

    python tools/bench_ref_voices.py [--reps 3] [--clips 64] [--out profiles/ref_voices.json]
"""
import argparse
import json
import os
import random
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_s2_decode import build_voice, workload  # noqa: E402


def clips_workload(n, seed=29):
    rnd = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        m = int(rnd.uniform(3.0, 10.0) * 32000)
        out.append(((torch.rand(m, generator=g) * 2 - 1) * rnd.choice([0.6, 0.95, 1.4, 2.6])).float())
    return out


def measure(dev, dtype, clips, reps, ks):
    from easevoice_trainer_amd.hip.audio import ref_spec_rows
    from easevoice_trainer_amd.module.mel_processing import spectrogram_torch

    voice = build_voice(dev, dtype)
    model = voice.model
    amp = dtype != torch.float32
    autocast = lambda: torch.autocast("cuda", dtype=dtype if amp else torch.bfloat16, enabled=amp)

    def one_spec(c):
        audio = c.clone()
        maxx = audio.abs().max()
        if maxx > 1:
            audio /= min(2, maxx)
        return spectrogram_torch(audio.unsqueeze(0).to(dev), 2048, 32000, 640, 2048)

    def style_one():
        out = []
        with torch.no_grad(), autocast():
            for c in clips:
                out.append(model._style(one_spec(c)))
        return out

    def style_rows(k):
        out = []
        with torch.no_grad():
            for i in range(0, len(clips), k):
                grp = clips[i:i + k]
                lens = [c.numel() for c in grp]
                host = torch.zeros(len(grp), max(lens))
                for b, c in enumerate(grp):
                    host[b, :lens[b]] = c
                spec, frames, _peak = ref_spec_rows(host.to(dev), lens)
                out.append(voice.style_rows(spec, frames))
        return out

    # (b): 16 voices per group
    codes, texts, refer = workload(64)
    codes, texts, refer = [c.to(dev) for c in codes], [t.to(dev) for t in texts], refer.to(dev)
    with torch.no_grad():
        specs = [one_spec(c) for c in clips[:16]]                         # 16 distinct reference spectrograms [1, 1025, F]
        with autocast():
            styles = torch.cat([model._style(s) for s in specs], 0)       # [16, gin]
    pad = torch.nn.utils.rnn.pad_sequence

    def decode16(kind):
        out = []
        for i in range(0, len(codes), 16):
            cs, ts = codes[i:i + 16], texts[i:i + 16]
            a = (pad(cs, batch_first=True).unsqueeze(0), [c.numel() for c in cs], pad(ts, batch_first=True), [t.numel() for t in ts])
            if kind == "refer":
                out += voice.decode_batch(*a, list(specs[:len(cs)]))
            elif kind == "shared":
                out += voice.decode_batch(*a, specs[0])
            else:
                out += voice.decode_batch(*a, None, style=styles[:len(cs)])
        return out

    modes = [("a/one", style_one)] + [(f"a/rows{k}", lambda k=k: style_rows(k)) for k in ks]
    modes += [("b/refer16", lambda: decode16("refer")), ("b/shared16", lambda: decode16("shared")),
              ("b/style16", lambda: decode16("style"))]
    for _name, fn in modes:                       # warm-up: every shape of every mode once
        fn()
        torch.cuda.synchronize()
    # what the two ways of (a) compute: the largest difference between style_rows and _style, relative to the largest component
    a, b = torch.cat(style_one(), 0).float(), torch.cat(style_rows(16), 0).float()
    agree = float((a - b).abs().max() / a.abs().max())
    times = {name: [] for name, _ in modes}
    for _ in range(reps):
        for name, fn in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    res = {"style_rows_vs_style_rel_maxabs": round(agree, 5), "modes": {}}
    for name, _ in modes:
        v = sorted(times[name])
        res["modes"][name] = {"seconds_median": round(v[len(v) // 2], 4), "seconds_min": round(v[0], 4), "seconds_max": round(v[-1], 4)}
    for name, m in res["modes"].items():
        base = res["modes"]["a/one" if name.startswith("a/") else "b/refer16"]["seconds_median"]
        m["ratio_vs_baseline"] = round(base / m["seconds_median"], 3)
    m = res["modes"]
    res["clips_per_s"] = {k: round(len(clips) / v["seconds_median"], 1) for k, v in m.items() if k.startswith("a/")}
    res["style_passes_share_of_refer16"] = round(1.0 - m["b/shared16"]["seconds_median"] / m["b/refer16"]["seconds_median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_voices.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_ref_voices needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    clips = clips_workload(args.clips)
    doc = {"tool": "tools/bench_ref_voices.py", "device": torch.cuda.get_device_name(0), "clips": len(clips),
           "clip_seconds_min_max": [round(min(c.numel() for c in clips) / 32000, 2), round(max(c.numel() for c in clips) / 32000, 2)],
           "audio_seconds": round(sum(c.numel() for c in clips) / 32000, 1), "reps": args.reps, "clock": "host (perf_counter between synchronisations)",
           "baselines": {"a": "a/one: host peak and division, upload, spectrogram_torch, _style, one clip at a time",
                         "b": "b/refer16: decode_batch(refer=[16 spectrograms]), 64 fragments in groups of 16"},
           "runs": {}}
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        doc["runs"][name] = measure(dev, dtype, clips, args.reps, args.groups)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
