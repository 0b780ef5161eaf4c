"""Throughput of the s2 decoder on finished fragments: SynthesizerTrn.decode one fragment at a time (what
inference/pipeline.py::synthesize_stream does per fragment) against SynthesizerTrn.decode_batch on groups of 4, 8 and 16
fragments of different lengths, in the same process.

Workload: 64 fragments of 2..10 s (seeded lengths, 25 codes and 12 phonemes per second), one reference spectrogram,
configs/s2.json at the benchmark's model size with random-init weights, bf16.  Groups are taken in arrival order (no
sorting by length: a stream cannot choose which fragments finish together), so a group pads to its longest member.

Protocol: every mode runs once untimed (all its shapes are then warm), then --reps timed passes with the modes alternated;
a pass is timed with device events around all its calls and ends in a synchronise.  Reported per mode: the median pass,
fragments/s and audio-seconds/s, and the spread (min / max seconds).  The yardstick is the `one` line of the same run.
A measurement path without a GPU fails.

--speed S (one speed for all fragments) or --mixed-speeds (a seeded choice out of 0.8, 1.0 and 1.25 per fragment) time the
same modes at those speeds: decode(speed=...) one at a time against decode_batch(speed=[...]) on the groups, whose rows are
resampled on their own lengths (evt_resample_rows).  Such a run is kept under its own name ("speed_1.25", "mixed") in
profiles/s2_decode_batch_speed.json, next to the runs the file already holds.

--pcm times the way from finished fragments to PCM (profiles/s2_decode_pcm.json), in groups of 1 / 4 / 8 / 16, under these
conditions: `device` -- waveforms on the device, as above; `host_int16` -- the same decode, then per fragment
.float().cpu().numpy() * 32768, astype(int16) and one concatenate with the 0.3 s of zeros behind each: the way to the
reference's int16 bytes without the finishing launch, and the BASELINE of this run; `pcm_<rate>` -- decode_batch(out_rate=rate,
out_format="int16", interval=0.3): one more launch per group, a packed buffer on the device, at 32000 and at every
--out-rate (default 16000 48000); `pcm_32000_host` -- that buffer copied to the host, one copy per group: the same bytes
as the baseline.  A lone fragment (groups of 1) takes decode and then resample_pack with one row, as synthesize_stream does.
The finishing launch alone is timed with device events on the rows of every group.

    python tools/bench_s2_decode.py [--reps 5] [--fragments 64] [--out profiles/s2_decode_batch.json]
    python tools/bench_s2_decode.py --speed 1.25
    python tools/bench_s2_decode.py --mixed-speeds
    python tools/bench_s2_decode.py --pcm [--out-rate 16000 48000]
"""
import argparse
import json
import os
import random
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(n, seed=11):
    rnd = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    secs = [rnd.uniform(2.0, 10.0) for _ in range(n)]
    codes = [torch.randint(0, 1024, (max(1, round(s * 25)),), generator=g) for s in secs]
    texts = [torch.randint(0, 732, (max(1, round(s * 12)),), generator=g) for s in secs]
    refer = torch.rand(1, 1025, 200, generator=g) * 2.0
    return codes, texts, refer


def build_voice(dev, dtype):
    from easevoice_trainer_amd.inference.sovits import SoVITSVoice
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    torch.manual_seed(hps["train"]["seed"])
    net = models.SynthesizerTrn(hps["data"]["filter_length"] // 2 + 1, hps["train"]["segment_size"] // hps["data"]["hop_length"],
                                n_speakers=hps["data"]["n_speakers"], **hps["model"])
    cb = net.quantizer.vq.layers[0]._codebook
    with torch.no_grad():
        cb.embed.normal_()
        cb.inited.fill_(1.0)
    weight = {k: v.detach().clone() for k, v in net.state_dict().items() if "enc_q" not in k}
    return SoVITSVoice({"weight": weight, "config": hps, "info": "bench"}, device=str(dev), dtype=dtype)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main_pcm(args):
    """--pcm: see the module docstring"""
    import numpy as np

    from easevoice_trainer_amd.hip.audio import resample_pack

    interval = 0.3
    dev = torch.device("cuda:0")
    voice = build_voice(dev, torch.bfloat16)
    codes, texts, refer = workload(args.fragments)
    codes, texts, refer = [c.to(dev) for c in codes], [t.to(dev) for t in texts], refer.to(dev)
    audio_s = sum(2 * c.numel() for c in codes) / 50.0
    pad = torch.nn.utils.rnn.pad_sequence
    rates = [32000] + [r for r in args.out_rate if r != 32000]
    ks = [1] + [k for k in args.batches if k != 1]

    def groups(k, **kw):
        """every group of k through the s2 decoder -> per group a list of waveforms, or a PackedAudio"""
        for i in range(0, len(codes), k):
            cs, ts = codes[i:i + k], texts[i:i + k]
            if k == 1:
                w = voice.decode(cs[0].view(1, 1, -1), ts[0].view(1, -1), refer)[0, 0]
                yield (resample_pack(w, [w.numel()], 1, 32000, kw["out_rate"], kw["out_format"], interval=kw["interval"])
                       if kw else [w])
            else:
                yield voice.decode_batch(pad(cs, batch_first=True).unsqueeze(0), [c.numel() for c in cs],
                                         pad(ts, batch_first=True), [t.numel() for t in ts], refer, **kw)

    def host_int16(k):
        zero = np.zeros(int(32000 * interval), dtype=np.int16)
        out = []
        for ws in groups(k):
            out.append(np.concatenate([a for w in ws for a in ((w.float().cpu().numpy() * 32768).astype(np.int16), zero)]))
        return out

    def pcm(k, rate, host=False):
        out = []
        for pa in groups(k, out_rate=rate, out_format="int16", interval=interval):
            out.append(pa.data.cpu() if host else pa.data)
        return out

    modes = []
    for k in ks:
        modes.append((f"device/{k}", lambda k=k: [w for ws in groups(k) for w in ws]))
        modes.append((f"host_int16/{k}", lambda k=k: host_int16(k)))
        modes.append((f"pcm_32000_host/{k}", lambda k=k: pcm(k, 32000, True)))
        modes += [(f"pcm_{r}/{k}", lambda k=k, r=r: pcm(k, r)) for r in rates]
    for _name, fn in modes:                       # warm-up: every shape of every mode once
        fn()
        torch.cuda.synchronize()
    # the bytes: the packed buffer at 32 kHz against the baseline's, first group of 4 under one prior noise.  They may differ
    # only where |x| * 32768 reaches 32768 (numpy wraps around, the launch saturates)
    noise = torch.randn(4, 192, 2 * max(c.numel() for c in codes[:4]) + 8, device=dev)
    a4 = (pad(codes[:4], batch_first=True).unsqueeze(0), [c.numel() for c in codes[:4]], pad(texts[:4], batch_first=True),
          [t.numel() for t in texts[:4]], refer)
    ws = voice.decode_batch(*a4, noise=noise)
    pa = voice.decode_batch(*a4, noise=noise, out_rate=32000, out_format="int16", interval=interval)
    zero = np.zeros(int(32000 * interval), dtype=np.int16)
    want = np.concatenate([a for w in ws for a in ((w.float().cpu().numpy() * 32768).astype(np.int16), zero)])
    differing = int((pa.data.cpu().numpy() != want).sum())
    times = {name: [] for name, _ in modes}
    for _ in range(args.reps):
        for name, fn in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 1e3)
    # the finishing launch alone, on the rows of every group (device events around the call, median over groups and reps)
    finish = {}
    for k in ks:
        rows = []
        for ws in groups(k):
            rows.append((pad(list(ws), batch_first=True).contiguous(), [w.numel() for w in ws]))
        for r in rates:
            us = []
            for _ in range(args.reps + 1):
                for x, lens in rows:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    resample_pack(x, lens, 1, 32000, r, "int16", interval=interval)
                    e1.record()
                    torch.cuda.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3)
            finish[f"{r}/{k}"] = round(_median(us[len(rows):]), 1)
    res = {"tool": "tools/bench_s2_decode.py --pcm", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "fragments": len(codes), "audio_seconds": round(audio_s, 2), "reps": args.reps, "interval_s": interval,
           "baseline": "host_int16/<k> of this run: the same decode, then per fragment .float().cpu().numpy() * 32768, "
                       "astype(int16), concatenated with the zeros behind each fragment",
           "samples_differing_from_baseline_bytes_first_group": differing,
           "finish_launch_us_median_per_group": finish, "modes": {}}
    for name, _ in modes:
        v = sorted(times[name])
        med = _median(v)
        res["modes"][name] = {"seconds_median": round(med, 4), "seconds_min": round(v[0], 4), "seconds_max": round(v[-1], 4),
                              "fragments_per_s": round(len(codes) / med, 1)}
    for name, m in res["modes"].items():
        m["ratio_vs_host_int16"] = round(res["modes"]["host_int16/" + name.split("/")[1]]["seconds_median"] / m["seconds_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fragments", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--speed", type=float, default=None, help="one speed for every fragment")
    ap.add_argument("--mixed-speeds", action="store_true", help="a seeded choice out of 0.8, 1.0, 1.25 per fragment")
    ap.add_argument("--pcm", action="store_true", help="time the way to packed int16 PCM (profiles/s2_decode_pcm.json)")
    ap.add_argument("--out-rate", type=int, nargs="+", default=[16000, 48000], help="with --pcm: output rates next to 32000")
    ap.add_argument("--out", default=None, help="default: profiles/s2_decode_batch.json, at a speed profiles/s2_decode_batch_speed.json")
    args = ap.parse_args()
    if args.pcm:
        if args.speed is not None or args.mixed_speeds:
            raise SystemExit("--pcm is measured at speed 1")
        if not torch.cuda.is_available():
            raise RuntimeError("bench_s2_decode needs a GPU: nothing is measured without one")
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "s2_decode_pcm.json")
        return main_pcm(args)
    if args.speed is not None and args.mixed_speeds:
        raise SystemExit("--speed and --mixed-speeds exclude each other")
    at_speed = args.speed is not None or args.mixed_speeds
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "s2_decode_batch_speed.json" if at_speed else "s2_decode_batch.json")
    if not torch.cuda.is_available():
        raise RuntimeError("bench_s2_decode needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    voice = build_voice(dev, torch.bfloat16)
    codes, texts, refer = workload(args.fragments)
    codes = [c.to(dev) for c in codes]
    texts = [t.to(dev) for t in texts]
    refer = refer.to(dev)
    if args.mixed_speeds:
        rnd = random.Random(23)
        speeds = [rnd.choice([0.8, 1.0, 1.25]) for _ in codes]
    else:
        speeds = [1.0 if args.speed is None else float(args.speed)] * len(codes)
    # frames per fragment behind the resampler (50 per second of output): the reference's int(T / speed) + 1
    frames = [2 * c.numel() if v == 1 else int(2 * c.numel() / v) + 1 for c, v in zip(codes, speeds)]
    audio_s = sum(frames) / 50.0
    pad = torch.nn.utils.rnn.pad_sequence

    def run_one():
        return [voice.decode(c.view(1, 1, -1), t.view(1, -1), refer, speed=v)[0, 0] for c, t, v in zip(codes, texts, speeds)]

    def run_batch(k):
        out = []
        for i in range(0, len(codes), k):
            cs, ts = codes[i:i + k], texts[i:i + k]
            kw = dict(speed=speeds[i:i + k]) if at_speed else {}
            out += voice.decode_batch(pad(cs, batch_first=True).unsqueeze(0), [c.numel() for c in cs],
                                      pad(ts, batch_first=True), [t.numel() for t in ts], refer, **kw)
        return out

    modes = [("one", run_one)] + [(f"batch{k}", (lambda k=k: run_batch(k))) for k in args.batches]
    for name, fn in modes:                        # warm-up: every shape of every mode once
        outs = fn()
        torch.cuda.synchronize()
        assert [o.numel() for o in outs] == [n * 640 for n in frames], name
        assert all(bool(torch.isfinite(o).all()) for o in outs), name
    # same inputs, same prior noise: a batched row against the row alone (bf16)
    noise = torch.randn(4, 192, max(2 * max(c.numel() for c in codes[:4]), max(frames[:4])) + 8, device=dev)
    got = voice.decode_batch(pad(codes[:4], batch_first=True).unsqueeze(0), [c.numel() for c in codes[:4]],
                             pad(texts[:4], batch_first=True), [t.numel() for t in texts[:4]], refer, noise=noise,
                             **(dict(speed=speeds[:4]) if at_speed else {}))
    check = []
    for b in range(4):
        a = voice.decode(codes[b].view(1, 1, -1), texts[b].view(1, -1), refer, speed=speeds[b],
                         noise=noise[b:b + 1])[0, 0].float()
        check.append(float((got[b].float() - a).abs().max() / (a.abs().max() + 1e-12)))
    times = {name: [] for name, _ in modes}
    for _ in range(args.reps):
        for name, fn in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 1e3)
    res = {"tool": "tools/bench_s2_decode.py", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "fragments": len(codes), "audio_seconds": round(audio_s, 2), "reps": args.reps,
           "speed": ("mixed: seeded choice out of 0.8, 1.0, 1.25 per fragment" if args.mixed_speeds else speeds[0]),
           "fragment_seconds_min_max": [min(c.numel() for c in codes) / 25.0, max(c.numel() for c in codes) / 25.0],
           "batched_row_vs_alone_rel_maxabs": [round(v, 5) for v in check], "modes": {}}
    for name, _ in modes:
        v = sorted(times[name])
        med = v[len(v) // 2]
        res["modes"][name] = {"seconds_median": round(med, 4), "seconds_min": round(v[0], 4), "seconds_max": round(v[-1], 4),
                              "fragments_per_s": round(len(codes) / med, 1), "audio_s_per_s": round(audio_s / med, 1)}
    base = res["modes"]["one"]["seconds_median"]
    for name, m in res["modes"].items():
        m["speedup_vs_one"] = round(base / m["seconds_median"], 3)
    best = max((n for n in res["modes"] if n != "one"), key=lambda n: res["modes"][n]["speedup_vs_one"])
    res["verdict"] = (f"{best} is {res['modes'][best]['speedup_vs_one']}x the one-at-a-time path"
                      if res["modes"][best]["speedup_vs_one"] > 1.0 else "no batch size beats the one-at-a-time path")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    doc = res
    if at_speed:
        # one file for the runs at a speed: the `one` line of each run is that run's baseline (nobody measured this before)
        res["baseline"] = "modes.one of this run: decode(speed=...) one fragment at a time"
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {"tool": res["tool"], "runs": {}}
        doc["runs"]["mixed" if args.mixed_speeds else f"speed_{speeds[0]:g}"] = res
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
