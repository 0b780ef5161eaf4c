"""Decoding throughput of the s1 model: tokens/s of infer_panel_naive for one sequence, HIP-graph
replay vs eager launches, with the algorithmic HBM bytes per token (every block matrix once + the key/value cache read).
--rows R [R ...] (R <= 64) also times infer_panel_batch_infer on R texts of different lengths, two modes alternated in
the same process: batch{R}_graph (one call: one session of up to 32 rows) and batch{R}_groups4_graph (the same texts in
consecutive calls of <= 4 rows, one session each); algorithmic bytes per step = every matrix once + R caches.

--stream times continuous batching: N texts (--stream-n, default 96) whose lives are spread over 64..512 steps in seeded
random order (EOS forced at each text's step through the noise table, so both paths stop every text at the same step) go
through infer_panel_batch_infer (groups of 32, each waiting for its slowest row) and then through the refilled session
(infer_panel_batch_infer_refill / decode_stream, 32 slots) in the same process; one JSON line with steps, useful tokens,
tokens/s and us per step of both, the stream's admissions and prefill time, median and last completion time, the step
time of both sessions with 32 rows alive for --tokens steps, and the prefill time of 1, 8 and 32 admitted rows.

--stream --slots S [S ...] times the refilled session alone at each of the slot counts (wide=True above 32), the same
seeded texts through every one, the slot counts alternated --reps times each, and asserts that every slot count produced
identical tokens; one JSON line with, per slot count, the median run's seconds, steps, useful tokens/s, us per step with
the prompt passes excluded, admissions and the share of the time spent in prompt passes.  --slots has no default value:
without it --stream keeps running the comparison above (grouped against refilled, 32 slots, with its rows32 and
admission sections), whose JSON line earlier profiles were recorded with; `--slots 32` is the 32-slot line of the new form.

    python tools/bench_s1_decode.py [--tokens 512] [--x-len 96] [--prompt 128] [--dtype bf16] [--rows 4 20 32]
    python tools/bench_s1_decode.py --stream [--stream-n 96]
    python tools/bench_s1_decode.py --stream --stream-n 512 --slots 32 64 96 128      (see run_slots)
    python tools/bench_s1_decode.py --stream --mixed 4      (per-request sampling parameters, see run_mixed)
    python tools/bench_s1_decode.py --stream --candidates 4 --logprobs      (see run_candidates)
    python tools/bench_s1_decode.py --stream --force 64      (forced first tokens of every request, see run_force)
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _stream_workload(args, dev, x, bert, prompts):
    """the texts of --stream: (lives, xs, berts, prompts, noise table, decode arguments, the noise generator)"""
    import random

    N, lo, hi, poll = args.stream_n, 64, 512, 8
    rnd = random.Random(7)
    lives = [lo + (hi - lo) * r // max(1, N - 1) for r in range(N)]       # step at which text r meets EOS
    rnd.shuffle(lives)
    lens = [max(1, args.x_len - 7 * (r % 12)) for r in range(N)]
    xs = [x[0][:n].contiguous() for n in lens]
    berts = [bert[0][:, :n].contiguous() for n in lens]
    pr = prompts.expand(N, -1).contiguous()
    g = torch.Generator().manual_seed(5)
    noise = torch.empty(hi + 2, N, 1025).exponential_(1, generator=g)
    noise[:, :, 1024] = 1e30                  # EOS never wins ...
    for r, s in enumerate(lives):
        noise[s, r, 1024] = 1e-30             # ... except at the text's own step (top_k covers the whole vocabulary)
    noise = noise.to(dev)
    kw = dict(top_k=1100, top_p=1, early_stop_num=hi + 8, repetition_penalty=1.35, poll=poll)
    return lives, xs, berts, pr, noise, kw, g


def run_mixed(args, m, dev, x, bert, prompts):
    """--mixed N: request r samples with parameter set r % N.  One refilled session that holds all sets (per-request
    values) against what a caller without them has to do: N uniform streams, one per set, one after the other.  The sets
    differ in temperature and repetition penalty only, so the forced EOS steps and with them the useful tokens are the
    same in both."""
    lives, xs, berts, pr, noise, kw, _g = _stream_workload(args, dev, x, bert, prompts)
    N, M = args.stream_n, args.mixed
    sets = [dict(temperature=1.0 + 0.05 * k, repetition_penalty=1.35 - 0.05 * k) for k in range(M)]
    kw = {k: v for k, v in kw.items() if k != "repetition_penalty"}
    cap = dict(max_text_len=args.x_len, max_prompt_len=args.prompt)      # one capacity: every stream may share a session
    infer = m._infer()
    groups = [list(range(k, N, M)) for k in range(M)]
    tables = [noise[:, members].contiguous() for members in groups]      # stream k reads its members' columns

    def mixed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reqs = [(xs[r], berts[r], pr[r], sets[r % M]) for r in range(N)]
        ys = [None] * N
        for r, y, _i in m.decode_stream(reqs, slots=32, noise=noise, **cap, **kw):
            ys[r] = y
        torch.cuda.synchronize()
        st = infer.stream_stats
        return ys, time.perf_counter() - t0, st["steps"], [bool(st["graph_captured"])]

    def uniform():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys, steps, captured = [None] * N, 0, []
        for k in range(M):
            members = groups[k]
            reqs = [(xs[r], berts[r], pr[r]) for r in members]
            for i, y, _i in m.decode_stream(reqs, slots=32, noise=tables[k], **cap, **kw, **sets[k]):
                ys[members[i]] = y
            steps += infer.stream_stats["steps"]
            captured.append(bool(infer.stream_stats["graph_captured"]))
        torch.cuda.synchronize()
        return ys, time.perf_counter() - t0, steps, captured

    runs = dict(uniform=[], mixed=[])
    for rep in range(args.reps + 1):
        for name, fn in (("uniform", uniform), ("mixed", mixed)):      # alternated: both see the same state of the device
            ys, t, steps, captured = fn()
            assert [y.numel() for y in ys] == [args.prompt + s for s in lives], name
            runs[name].append((t, steps, captured))
    useful, out = sum(lives), {}
    for name, v in runs.items():
        t, steps, _c = sorted(v[1:], key=lambda e: e[0])[len(v[1:]) // 2]
        out[name] = dict(seconds=round(t, 4), steps=steps, useful_tokens=useful, tokens_per_s=round(useful / t, 1),
                         seconds_all_runs=[round(e[0], 4) for e in v[1:]],
                         graph_captures_first_pass=sum(v[0][2]), graph_captures_timed_passes=sum(sum(e[2]) for e in v[1:]))
    out["mixed_over_uniform"] = round(out["uniform"]["seconds"] / out["mixed"]["seconds"], 3)
    print(json.dumps(dict(workload=f"s1 decode stream, {N} texts living 64..512 steps, {M} parameter sets (request r: "
                                   f"set r % {M}), x_len<={args.x_len}, prompt={args.prompt}, {args.dtype}, 32 slots; "
                                   f"uniform = {M} streams of {N // M} texts one after the other, mixed = one session; "
                                   "all streams share one capacity and one session; the step graph is keyed by the "
                                   "noise table, so each uniform stream (own table) captures again, as a stream per "
                                   "parameter set did when the parameters were part of the key", **out)))


def run_candidates(args, m, dev, x, bert, prompts):
    """--candidates N and / or --logprobs.  (1) 32 slots alive for --tokens steps (32 // N requests with N candidates
    each), log-probabilities off and -- with --logprobs -- on, alternated in one process: time per replay with the
    prompt pass excluded.  (2) the admission of ONE request with N candidates (one prompt row copied into N slots)
    against N single requests (N prompt rows).  One JSON line with prefill_rows, prefill_s and the per-replay times."""
    lives, xs, berts, pr, _noise, _kw, g = _stream_workload(args, dev, x, bert, prompts)
    N, T = max(1, args.candidates), args.tokens
    R = 32 // N
    infer = m._infer()
    nz = torch.empty(T + 2, R, N, 1025).exponential_(1, generator=g)
    nz[..., 1024] = 1e30
    nz = nz.to(dev)
    kw = dict(top_k=15, top_p=1, early_stop_num=T, repetition_penalty=1.35)
    reqs = [(xs[r], berts[r], pr[r]) for r in range(R)]
    modes = [False, True] if args.logprobs else [False]
    runs = {lp: [] for lp in modes}
    for rep in range(args.reps + 1):
        for lp in modes:                       # alternated: both see the same state of the device
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = list(m.decode_stream(reqs, slots=R * N, n=N, logprobs=lp, noise=nz, **kw))
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            st = infer.stream_stats
            assert len(outs) == R * N and all(o[1].numel() == args.prompt + T for o in outs)
            runs[lp].append(dict(seconds=t, prefill_s=sum(st["prefill_s"]), steps=st["steps"],
                                 prefill_rows=list(st["prefill_rows"]), admitted=list(st["admitted"])))
    out = {}
    for lp in modes:
        rs = runs[lp][1:]
        out["logprobs_on" if lp else "logprobs_off"] = dict(
            prefill_rows=rs[0]["prefill_rows"], admitted=rs[0]["admitted"],
            prefill_s=[round(r["prefill_s"], 5) for r in rs],
            us_per_replay_all_runs=[round(1e6 * (r["seconds"] - r["prefill_s"]) / r["steps"], 1) for r in rs])
    if args.logprobs:
        med = lambda k: _median(out[k]["us_per_replay_all_runs"])
        out["logprobs_on_over_off"] = round(med("logprobs_on") / med("logprobs_off"), 4)
    # ---- admission: one request with N candidates against N single requests ----
    adm = {}
    for name, rq, n, tab in (("one_request_n", reqs[:1], N, nz[:, :1].contiguous()),
                             ("n_single_requests", [reqs[0]] * N, 1, nz[:, 0].contiguous())):
        ms = []
        for rep in range(4):
            list(m.decode_stream([(*q, 1) for q in rq], slots=N, n=n, noise=tab, logprobs=args.logprobs, **kw))
            ms.append(1e3 * infer.stream_stats["prefill_s"][0])
        adm[name] = dict(prefill_ms=round(min(ms[1:]), 3), prefill_rows=infer.stream_stats["prefill_rows"],
                         admitted=infer.stream_stats["admitted"])
    out["admission"] = adm
    print(json.dumps(dict(workload=f"s1 decode stream, {R} requests x {N} candidates alive for {T} steps, "
                                   f"x_len<={args.x_len}, prompt={args.prompt}, {args.dtype}, {R * N} slots", **out)))


def run_force(args, m, dev, x, bert, prompts):
    """--force K: 32 slots alive for --tokens steps, every request with its first K tokens given ("force": the sampler
    launch evt_dec_sample_embed_rows_f, K forced steps and --tokens - K sampled ones) against the same requests without
    them (evt_dec_sample_embed_rows_p), alternated in one process: time per replay with the prompt pass excluded.  With
    --logprobs both sides record log-probabilities (the forced launch against evt_dec_sample_embed_rows_lp)."""
    _lives, xs, berts, pr, _noise, _kw, g = _stream_workload(args, dev, x, bert, prompts)
    T, R, K = args.tokens, 32, args.force
    assert 1 <= K <= T, (K, T)
    infer = m._infer()
    nz = torch.empty(T + 2, R, 1025).exponential_(1, generator=g)
    nz[..., 1024] = 1e30
    nz = nz.to(dev)
    kw = dict(top_k=15, top_p=1, early_stop_num=T, repetition_penalty=1.35, logprobs=args.logprobs, noise=nz)
    given = torch.randint(0, 1024, (R, K), generator=g)
    plain = [(xs[r], berts[r], pr[r]) for r in range(R)]
    forced = [(*q, dict(force=given[r])) for r, q in enumerate(plain)]
    runs = {False: [], True: []}
    for rep in range(args.reps + 1):
        for f in (False, True):                # alternated: both see the same state of the device
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = list(m.decode_stream(forced if f else plain, slots=R, **kw))
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            st = infer.stream_stats
            assert len(outs) == R and all(o[1].numel() == args.prompt + T for o in outs)
            if f:
                assert all(torch.equal(o[1][args.prompt:args.prompt + K].cpu(), given[o[0]]) for o in outs)
            runs[f].append(1e6 * (t - sum(st["prefill_s"])) / st["steps"])
    out = dict(plain_us_per_replay_all_runs=[round(v, 1) for v in runs[False][1:]],
               forced_us_per_replay_all_runs=[round(v, 1) for v in runs[True][1:]])
    out["forced_over_plain"] = round(_median(runs[True][1:]) / _median(runs[False][1:]), 4)
    print(json.dumps(dict(workload=f"s1 decode stream, {R} requests alive for {T} steps, the first {K} tokens of each "
                                   f"forced against none, logprobs={args.logprobs}, x_len<={args.x_len}, "
                                   f"prompt={args.prompt}, {args.dtype}, {R} slots", **out)))


def run_slots(args, m, dev, x, bert, prompts):
    """--slots S [S ...]: the texts of --stream through one refilled session per slot count.  Every session is kept for
    the whole run (the tool raises the model's WIDE_SESSIONS to the number of slot counts), so a timed pass neither
    allocates a cache nor captures a graph; the first pass of each slot count does both and is not timed."""
    lives, xs, berts, pr, noise, kw, _g = _stream_workload(args, dev, x, bert, prompts)
    N, poll = args.stream_n, kw["poll"]
    infer = m._infer()
    infer.WIDE_SESSIONS = max(infer.WIDE_SESSIONS, len(args.slots))
    reqs = [(xs[r], berts[r], pr[r]) for r in range(N)]
    useful = sum(lives)
    runs, first = {S: [] for S in args.slots}, None
    identical = True
    for rep in range(args.reps + 1):
        for S in args.slots:                   # alternated: every slot count sees the same state of the device
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ys = [None] * N
            for r, y, _i in m.decode_stream(reqs, slots=S, wide=S > 32, noise=noise, **kw):
                ys[r] = y
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            st = infer.stream_stats
            assert [y.numel() for y in ys] == [args.prompt + s for s in lives], S
            if first is None:
                first = ys
            elif not all(torch.equal(a, b) for a, b in zip(first, ys)):
                identical = False
            runs[S].append(dict(seconds=t, steps=st["steps"], prefill_s=sum(st["prefill_s"]), admissions=st["admissions"],
                                captured=bool(st["graph_captured"])))
    out = {}
    for S, v in runs.items():
        timed = v[1:]
        med = sorted(timed, key=lambda e: e["seconds"])[len(timed) // 2]
        t, pre = med["seconds"], med["prefill_s"]
        out[str(S)] = dict(seconds=round(t, 4), steps=med["steps"], useful_tokens=useful,
                           tokens_per_s=round(useful / t, 1), us_per_step=round(1e6 * (t - pre) / med["steps"], 1),
                           admissions=med["admissions"], prefill_share=round(pre / t, 4),
                           seconds_all_runs=[round(e["seconds"], 4) for e in timed],
                           graph_captures_timed_passes=sum(e["captured"] for e in timed))
    base = out[str(args.slots[0])]["tokens_per_s"]
    for S in args.slots[1:]:
        out[str(S)]["tokens_per_s_over_first"] = round(out[str(S)]["tokens_per_s"] / base, 3)
    print(json.dumps(dict(workload=f"s1 decode stream, {N} texts living 64..512 steps, x_len<={args.x_len}, "
                                   f"prompt={args.prompt}, {args.dtype}, poll {poll}, slots {args.slots} alternated, "
                                   f"median of {args.reps}; us_per_step excludes the prompt passes, prefill_share is "
                                   "their share of the seconds", identical_tokens=identical, slots=out)), flush=True)
    assert identical, "the slot counts did not produce identical tokens"


def run_stream(args, m, dev, x, bert, prompts):
    """grouped against refilled decoding of the same requests (see the module docstring)"""
    lives, xs, berts, pr, noise, kw, g = _stream_workload(args, dev, x, bert, prompts)
    N, lo, hi, poll = args.stream_n, 64, 512, 8
    infer = m._infer()

    def grouped():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys, idxs, done = [], [], []
        for g0 in range(0, N, 32):            # infer_panel_batch_infer's own grouping, timed per group
            rows = list(range(g0, min(N, g0 + 32)))
            y, i = m.infer_panel_batch_infer([xs[r] for r in rows], None, pr[rows], [berts[r] for r in rows],
                                             noise=noise[:, rows].contiguous(), **kw)
            torch.cuda.synchronize()
            ys += y
            idxs += i
            done += [time.perf_counter() - t0] * len(rows)
        return ys, idxs, done, time.perf_counter() - t0

    def refilled():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys, done = [None] * N, [None] * N
        reqs = [(xs[r], berts[r], pr[r]) for r in range(N)]
        for r, y, _i in m.decode_stream(reqs, slots=32, noise=noise, **kw):
            ys[r], done[r] = y, time.perf_counter() - t0
        torch.cuda.synchronize()
        return ys, done, time.perf_counter() - t0, dict(infer.stream_stats)

    out = {}
    gt, st = [], []
    for rep in range(args.reps + 1):
        ys_g, idx_g, done_g, t_g = grouped()
        ys_s, done_s, t_s, stats = refilled()
        assert [y.numel() for y in ys_g] == [y.numel() for y in ys_s] == [args.prompt + s for s in lives]
        gt.append((t_g, done_g))
        st.append((t_s, done_s, stats))
    useful = sum(lives)
    # replays of the grouped path: each group steps until the poll after its slowest row's stop
    steps_g = sum(-(-(max(lives[g0:g0 + 32]) + 1) // poll) * poll for g0 in range(0, N, 32))
    t_g, done_g = _median(gt[1:])
    t_s, done_s, stats = sorted(st[1:], key=lambda v: v[0])[len(st[1:]) // 2]
    pre = sum(stats["prefill_s"])
    out["grouped"] = dict(seconds=round(t_g, 4), steps=steps_g, useful_tokens=useful, tokens_per_s=round(useful / t_g, 1),
                          us_per_step=round(1e6 * t_g / steps_g, 1), median_completion_s=round(_median(done_g), 4),
                          last_completion_s=round(max(done_g), 4))
    out["stream"] = dict(seconds=round(t_s, 4), steps=stats["steps"], useful_tokens=useful,
                         tokens_per_s=round(useful / t_s, 1), us_per_step=round(1e6 * (t_s - pre) / stats["steps"], 1),
                         admissions=stats["admissions"], admitted=stats["admitted"], prefill_ms=round(1e3 * pre, 2),
                         median_completion_s=round(_median(done_s), 4), last_completion_s=round(max(done_s), 4))
    out["stream_over_grouped"] = round(t_g / t_s, 3)
    out["grouped_seconds_all_runs"] = [round(v[0], 4) for v in gt[1:]]
    out["stream_seconds_all_runs"] = [round(v[0], 4) for v in st[1:]]
    # ---- step time with 32 rows alive for --tokens steps (the workload of --rows 32) ----
    T = args.tokens
    nz = torch.empty(T + 2, 1025).exponential_(1, generator=g)
    nz[:, 1024] = 1e30
    nz = nz.to(dev)
    kw32 = dict(top_k=15, top_p=1, early_stop_num=T, repetition_penalty=1.35, noise=nz)
    rows = list(range(32))
    tg, ts = [], []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.infer_panel_batch_infer([xs[r] for r in rows], None, pr[rows], [berts[r] for r in rows], **kw32)
        torch.cuda.synchronize()
        tg.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ys = m.infer_panel_batch_infer_refill([xs[r] for r in rows], None, pr[rows], [berts[r] for r in rows], slots=32,
                                              **kw32)[0]
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0, sum(infer.stream_stats["prefill_s"]), infer.stream_stats["steps"]))
        assert all(y.numel() == args.prompt + T for y in ys)
    out["rows32"] = dict(
        tokens=T,
        grouped_us_per_step_all_runs=[round(1e6 * t / (T + 1), 1) for t in tg[1:]],
        stream_us_per_step_all_runs=[round(1e6 * t / (T + 1), 1) for t, _p, _n in ts[1:]],
        stream_us_per_replay_all_runs=[round(1e6 * (t - p) / n, 1) for t, p, n in ts[1:]],
        note="per step: whole call / (tokens + 1), prompt pass included, as batch32_graph; per replay: prefill excluded")
    # ---- cost of an admission: prompt pass + cache copy + step 0 for k rows ----
    adm = {}
    for k in (1, 8, 32):
        reqs = [(xs[r], berts[r], pr[r], 1) for r in range(k)]
        ms = []
        for rep in range(3):
            list(m.decode_stream(reqs, slots=k, noise=nz, top_k=15, top_p=1, early_stop_num=T))
            ms.append(1e3 * infer.stream_stats["prefill_s"][0])
        adm[str(k)] = round(min(ms[1:]), 2)
    out["admission_prefill_ms"] = adm
    print(json.dumps(dict(workload=f"s1 decode stream, {N} texts living {lo}..{hi} steps, x_len<={args.x_len}, "
                                   f"prompt={args.prompt}, {args.dtype}, 32 slots, poll {poll}", **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--x-len", type=int, default=96)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=[],
                    help="also time infer_panel_batch_infer with this many texts (each <= 64)")
    ap.add_argument("--rows-only", action="store_true",
                    help="time batch{R}_graph alone (no single-sequence lines, no groups of 4): for a kernel trace")
    ap.add_argument("--stream", action="store_true",
                    help="time the refilled session against infer_panel_batch_infer on --stream-n texts (nothing else)")
    ap.add_argument("--stream-n", type=int, default=96)
    ap.add_argument("--slots", type=int, nargs="+", default=None, metavar="S",
                    help="with --stream: the refilled session alone at each of these slot counts (1..128, wide=True above "
                         "32), alternated, with identical tokens asserted (nothing else); default: the comparison with "
                         "infer_panel_batch_infer at 32 slots")
    ap.add_argument("--mixed", type=int, default=0, metavar="N",
                    help="with --stream: request r samples with parameter set r %% N; one session holding all sets "
                         "against N uniform streams run one after the other (nothing else)")
    ap.add_argument("--candidates", type=int, default=0, metavar="N",
                    help="with --stream: 32 // N requests with N candidates each in one session, and the admission of "
                         "one request with N candidates against N single requests (nothing else)")
    ap.add_argument("--force", type=int, default=0, metavar="K",
                    help="with --stream: time per replay with the first K tokens of every request forced (the forced "
                         "sampler launch) against the plain stream; --logprobs turns them on for both (nothing else)")
    ap.add_argument("--logprobs", action="store_true",
                    help="with --stream: time per replay with per-token log-probabilities on against off (nothing else)")
    args = ap.parse_args()
    from easevoice_trainer_amd.train.s1_engine import S1Engine

    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    torch.manual_seed(1234)
    m = S1Engine(cfg, dev, dtype).model
    m.eval()
    with torch.no_grad():
        m.ar_predict_layer.weight[-1].zero_()      # EOS logit 0: never the arg-max of 1025 random logits
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 732, (1, args.x_len), generator=g).to(dev)
    bert = torch.randn(1, 1024, args.x_len, generator=g).to(dev)
    prompts = torch.randint(0, 1024, (1, args.prompt), generator=g).to(dev)
    # a noise table that never lets EOS win keeps every run at exactly --tokens steps
    noise = torch.empty(args.tokens + 2, 1025).exponential_(1, generator=g)
    noise[:, 1024] = 1e30
    noise = noise.to(dev)
    if args.stream:
        os.environ["EVT_DECODE_GRAPH"] = "1"
        if args.slots:
            assert all(1 <= S <= 128 for S in args.slots), args.slots
            run_slots(args, m, dev, x, bert, prompts)
            return
        if args.mixed:
            assert 1 <= args.mixed <= 8, args.mixed
            run_mixed(args, m, dev, x, bert, prompts)
            return
        if args.force:
            run_force(args, m, dev, x, bert, prompts)
            return
        if args.candidates or args.logprobs:
            assert 0 <= args.candidates <= 32, args.candidates
            run_candidates(args, m, dev, x, bert, prompts)
            return
        run_stream(args, m, dev, x, bert, prompts)
        return
    esz = 2 if dtype == torch.bfloat16 else 4
    E, nl = 512, 24
    w_bytes = (nl * (3 * E * E + E * E + 8 * E * E) + 1025 * E) * esz
    out = {}
    for mode in () if args.rows_only else ("1", "0"):
        os.environ["EVT_DECODE_GRAPH"] = mode
        times = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y, idx = m.infer_panel_naive(x, None, prompts, bert, top_k=15, top_p=1, early_stop_num=args.tokens, noise=noise,
                                         repetition_penalty=1.35)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            assert y.size(1) == args.prompt + args.tokens, (y.shape, idx)
        t = sorted(times[1:])[len(times[1:]) // 2]
        out["graph" if mode == "1" else "eager"] = dict(seconds=round(t, 4), tokens_per_s=round((args.tokens + 1) / t, 1),
                                                        us_per_token=round(1e6 * t / (args.tokens + 1), 1))
    L_avg = args.x_len + args.prompt + args.tokens / 2
    cache_bytes = nl * 2 * L_avg * E * esz
    for R in args.rows:
        assert 1 <= R <= 64, R
        os.environ["EVT_DECODE_GRAPH"] = "1"
        # different text lengths (a padded batch), cycling past 12 rows so that every text stays non-empty
        lens = [max(1, args.x_len - 7 * (r % 12)) for r in range(R)]
        xs = [x[0][:n].contiguous() for n in lens]
        berts = [bert[0][:, :n].contiguous() for n in lens]
        pr = prompts.expand(R, -1).contiguous()

        def call(rows):
            return m.infer_panel_batch_infer([xs[r] for r in rows], None, pr[rows], [berts[r] for r in rows], top_k=15,
                                             top_p=1, early_stop_num=args.tokens, noise=noise, repetition_penalty=1.35)

        modes = {f"batch{R}_graph": [list(range(R))]}
        if R > 4 and not args.rows_only:
            modes[f"batch{R}_groups4_graph"] = [list(range(g, min(R, g + 4))) for g in range(0, R, 4)]
        times = {k: [] for k in modes}
        for rep in range(args.reps + 1):
            for k, calls in modes.items():           # alternated: both modes see the same state of the device
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for rows in calls:
                    ys, idxs = call(rows)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
                assert all(y.numel() == args.prompt + args.tokens for y in ys), [y.shape for y in ys]
        bytes_step = w_bytes + R * cache_bytes
        for k in modes:
            t = sorted(times[k][1:])[len(times[k][1:]) // 2]
            us = 1e6 * t / (args.tokens + 1)
            out[k] = dict(seconds=round(t, 4), tokens_per_s=round(R * (args.tokens + 1) / t, 1), us_per_step=round(us, 1),
                          algorithmic_bytes_per_step=int(bytes_step), GBps=round(bytes_step / (us * 1e-6) / 1e9, 1))
    per_tok = w_bytes + cache_bytes
    if args.rows_only:
        print(json.dumps(dict(workload=f"s1 decode, rows {args.rows}, x_len={args.x_len}, prompt={args.prompt}, "
                                       f"{args.tokens} tokens, {args.dtype}, top_k=15 (prompt pass included)", **out)))
        return
    gps = per_tok / (out["graph"]["us_per_token"] * 1e-6) / 1e9
    print(json.dumps(dict(workload=f"s1 decode, 1 sequence, x_len={args.x_len}, prompt={args.prompt}, {args.tokens} tokens, "
                                   f"{args.dtype}, top_k=15 (prompt pass included)",
                          **out, algorithmic_bytes_per_token=int(per_tok), achieved_GBps=round(gps, 1),
                          hbm_peak_GBps=8000, frac=round(gps / 8000, 4))))


if __name__ == "__main__":
    main()
