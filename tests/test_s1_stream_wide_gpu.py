"""GPU: evt_dec_gemm_rows for 33..128 rows (row groups of 32 on one more grid dimension, csrc/s1_decode_rows.hip) and
stream sessions of up to 128 slots (decode_stream(..., wide=True), auto_reg/t2s_infer.py).  The property pinned for the
kernel: every output row of a wide launch has the bits of a launch of at most 32 rows on that row's group.  For the
session: the reference's token lists through 64 slots, and the same tokens through 128 slots as through 32."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F
import yaml

import exact_inputs as X
from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

SHAPES = [(1536, 512), (512, 512), (2048, 512), (512, 2048), (1025, 512)]   # test_s1_decode_rows_gpu.py::SHAPES
WIDE_B = [33, 48, 64, 100, 128]
Y_MARK, X_MARK = -3.0, -7.0


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _linear(gpu, Wg, bias, a, r, lg, lb, relu, use_ln):
    """one evt_dec_gemm_rows launch on all rows of `a`; y and x_out carry two sentinel rows behind the last row"""
    from easevoice_trainer_amd.hip import lib as L

    (N, K), B = Wg.shape, a.size(0)
    y = torch.full((B + 2, N), Y_MARK, device=gpu)
    xo = torch.full((B + 2, K), X_MARK, device=gpu)
    args = [a, r, lg, lb] if use_ln else [a, None, None, None]
    L.check(L.lib().evt_dec_gemm_rows(L.dt_of(Wg), L.ptr(Wg), L.ptr(bias), L.ptr(args[0]), L.ptr(args[1]),
                                      L.ptr(args[2]), L.ptr(args[3]), C.c_float(1e-5), L.ptr(xo) if use_ln else None,
                                      L.ptr(y), B, N, K, relu, L.stream_ptr()), "evt_dec_gemm_rows")
    torch.cuda.synchronize()
    assert torch.equal(y[B:], torch.full((2, N), Y_MARK, device=gpu)), "y: written behind the last row"
    assert torch.equal(xo[B:], torch.full((2, K), X_MARK, device=gpu)), "x_out: written behind the last row"
    return y[:B], xo[:B]


def _case(B, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    bias, a, r = torch.randn(N, generator=g), torch.randn(B, K, generator=g), torch.randn(B, K, generator=g)
    lg, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    return W, bias, a, r, lg, lb


def _check_groups(gpu, Wg, bg, a, r, lg, lb, B, tag=""):
    """all four (LayerNorm prologue, relu) variants of one wide launch: group by group the bits of a launch of at most 32
    rows on that slice of a / r.  Returns {(use_ln, relu): (y, x_out)}"""
    out = {}
    for use_ln in (False, True):
        for relu in (0, 1):
            y, xo = _linear(gpu, Wg, bg, a, r, lg, lb, relu, use_ln)
            for g0 in range(0, B, 32):
                rows = slice(g0, min(g0 + 32, B))
                yg, xg = _linear(gpu, Wg, bg, a[rows], r[rows], lg, lb, relu, use_ln)
                assert torch.equal(y[rows], yg), (tag, use_ln, relu, g0)
                if use_ln:
                    assert torch.equal(xo[rows], xg), (tag, use_ln, relu, g0)
            if not use_ln:      # no LayerNorm side output without the prologue
                assert torch.equal(xo, torch.full_like(xo, X_MARK))
            out[use_ln, relu] = (y, xo)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
@pytest.mark.parametrize("B", WIDE_B)
def test_wide_launch_equals_row_group_launches(gpu, dtype, shape, B):
    """33..128 rows (full groups, a last group of 1, 4, 16 rows): bit-identical to the row groups launched alone, nothing
    written behind row B - 1, and within test_dec_gemm_rows' tolerances of torch fp32; N = 1025 has no bias"""
    N, K = shape
    W, bias, a, r, lg, lb = _case(B, N, K, dtype, N + K + B)
    dev = lambda t: t.to(gpu)
    Wg, bg = dev(W), (None if N == 1025 else dev(bias))
    got = _check_groups(gpu, Wg, bg, dev(a), dev(r), dev(lg), dev(lb), B)
    for (use_ln, relu), (y, xo) in got.items():
        x = F.layer_norm(a + r, (K,), lg, lb, 1e-5) if use_ln else a
        want = x @ W.float().t() + (0.0 if N == 1025 else bias)
        want = want.clamp(min=0) if relu else want
        assert rel(y, want) < 2e-5, (use_ln, relu)
        if use_ln:
            assert rel(xo, x) < 1e-5


@pytest.mark.parametrize("wdn", ["f32", "bf16"])
@pytest.mark.parametrize("B", [33, 128])
def test_wide_linear_exact(gpu, B, wdn):
    """test_dec_linear_exact at 33 and 128 rows: integer operands make every sum exact below 2^24, so y equals the
    reference in any order"""
    from easevoice_trainer_amd.hip import lib as L

    for N, K in X.DEC_SHAPES:
        g = X.gen("dec", B, N, K, wdn)
        W, a = X.dense_pm((N, K), g), X.small_int((B, K), g, 3)
        bias = None if N == 1025 else X.small_int((N,), g, 3)
        Wg, ag = W.to(gpu, torch.float32 if wdn == "f32" else torch.bfloat16), a.float().to(gpu)
        bg = bias.float().to(gpu) if bias is not None else None
        for relu in (0, 1):
            want = a @ W.t() + (bias if bias is not None else 0.0)
            want = want.clamp(min=0) if relu else want
            assert float(want.abs().max()) < X.F32_EXACT
            y = torch.full((B, N), float("nan"), device=gpu)
            L.check(L.lib().evt_dec_gemm_rows(L.dt_of(Wg), L.ptr(Wg), L.ptr(bg), L.ptr(ag), None, None, None,
                                              C.c_float(1e-5), None, L.ptr(y), B, N, K, relu, L.stream_ptr()),
                    "evt_dec_gemm_rows")
            torch.cuda.synchronize()
            X.assert_exact(y, want, torch.float32, "evt_dec_gemm_rows", nlc=False,
                           context=f"[B={B} N={N} K={K} {wdn} relu={relu}]")


def test_wide_launch_f16_build(gpu):
    """the IEEE-half build serves 64 rows the same way"""
    from easevoice_trainer_amd.hip import lib as L

    B, N, K = 64, 2048, 512
    W, bias, a, r, lg, lb = _case(B, N, K, torch.float16, 5)
    L.set_half(torch.float16)
    try:
        got = _check_groups(gpu, *(t.to(gpu) for t in (W, bias, a, r, lg, lb)), B, tag="f16")
    finally:
        L.set_half(torch.bfloat16)
    x = F.layer_norm(a + r, (K,), lg, lb, 1e-5)
    y, xo = got[True, 1]
    assert rel(y, (x @ W.float().t() + bias).clamp(min=0)) < 2e-5 and rel(xo, x) < 1e-5


def test_129_rows_are_not_supported(gpu):
    """EVT_ENOTSUP (95), nothing launched"""
    from easevoice_trainer_amd.hip import lib as L

    B, N, K = 129, 512, 512
    W, a, y = torch.zeros(N, K, device=gpu), torch.zeros(B, K, device=gpu), torch.full((B, N), Y_MARK, device=gpu)
    rc = L.lib().evt_dec_gemm_rows(L.dt_of(W), L.ptr(W), None, L.ptr(a), None, None, None, C.c_float(1e-5), None,
                                   L.ptr(y), B, N, K, 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 95 and torch.equal(y, torch.full_like(y, Y_MARK))


# ---- whole streams ----
@pytest.fixture(scope="module")
def model(gpu):
    from easevoice_trainer_amd.train.s1_engine import S1Engine

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    eng = S1Engine(cfg, gpu, torch.float32)
    fill_module(eng.model, 3)
    eng.model.eval()
    return eng.model


def _stream(m, gpu, d, R, slots, **kw):
    """R texts through decode_stream itself (infer_panel_batch_infer_refill clamps the slots to the number of texts), in
    input order; the session made for the stream has exactly `slots` rows, more than R of them stay idle"""
    reqs = [(d["x"][r].to(gpu), d["bert"][r].to(gpu), d["prompts"][r].to(gpu)) for r in range(R)]
    ys, idxs = [None] * R, [None] * R
    for r, y, i in m.decode_stream(reqs, slots=slots, wide=slots > 32, **kw):
        ys[r], idxs[r] = y, i
    inf = m._infer()
    assert inf._sessions[inf._wide[-1]].B == slots
    return ys, idxs


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_reference_tokens_through_64_slots(gpu, model, graph, monkeypatch):
    """the fixture's 36 texts in one admission of a 64-slot session, rows 32..35 in the second row group: the
    reference's token lists, fp32"""
    from make_golden_s1_rows import rows_inputs

    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    gold = {c["args"]["R"]: c for c in torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"),
                                                  weights_only=False)["cases"]}[36]
    a = {k: v for k, v in gold["args"].items() if k != "R"}
    d = rows_inputs(36)
    reqs = [(d["x"][r].to(gpu), d["bert"][r].to(gpu), d["prompts"][r].to(gpu)) for r in range(36)]
    out = {r: (y, i) for r, y, i in model.decode_stream(reqs, slots=64, wide=True, noise=d["q"], **a)}
    st = model._infer().stream_stats
    assert st["admitted"] == [36] and {slot for k, _s, _r, slot in st["events"] if k == "admit"} == set(range(36))
    assert [out[r][1] for r in range(36)] == gold["idx"]
    for r, g in enumerate(gold["y"]):
        assert torch.equal(out[r][0].cpu().long(), g.long()), r


@pytest.mark.parametrize("noise", ["table", "seed"])
def test_100_texts_same_tokens_through_128_as_through_32_slots(gpu, model, noise):
    """a row's tokens do not depend on the number of slots (fp32): with the injected noise table and under one
    built-in seed.  The wide session has 128 rows, 28 of them idle: gemm, attention and sampler launch at B = 128"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(100)
    kw = dict(top_k=1100, top_p=1, noise=d["q"]) if noise == "table" else dict(top_k=15, top_p=1, seed=4242)
    kw["early_stop_num"] = 12
    rows = list(range(100))
    ys, idxs = _stream(model, gpu, d, 100, 128, **kw)
    assert model._infer().stream_stats["admitted"] == [100]
    y2, i2 = _stream(model, gpu, d, 100, 32, **kw)
    adm = model._infer().stream_stats["admitted"]
    assert adm[0] == 32 and sum(adm) == 100
    assert idxs == i2
    for r in rows:
        assert torch.equal(ys[r], y2[r]), r
    if noise == "table":      # the table's EOS schedule: rows of different lives, so the wide session is refilled too
        assert len(set(idxs)) > 2
    else:                     # rows draw their own lanes: the texts do not share one token sequence
        assert len({tuple(y[12:].tolist()) for y in ys}) > 50


def test_wide_bf16_repeatable(gpu, model):
    """100 requests through a session of 128 slots (28 idle) in bf16 under one seed: the same tokens twice, all of them
    valid, every index within its limit"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(100)
    model.cd = torch.bfloat16
    try:
        out = [_stream(model, gpu, d, 100, 128, top_k=15, top_p=1, early_stop_num=30, seed=77) for _ in range(2)]
        adm = model._infer().stream_stats["admitted"]
    finally:
        model.cd = torch.float32
    (ys1, i1), (ys2, i2) = out
    assert i1 == i2 and len(ys1) == 100 and adm == [100]
    assert all(torch.equal(a, b) for a, b in zip(ys1, ys2))
    for y, i in zip(ys1, i1):
        assert 0 <= i <= 30 and int(y.min()) >= 0 and int(y[12:].max()) <= 1024 and y.numel() > 12


def test_40_candidates_in_64_slots(gpu, model):
    """n = 40 with log-probabilities in a 64-slot session (lanes r % 4 + 4c up to 159): 40 outputs per request, candidate
    0 is the n = 1 run, the log-probabilities of every drawn token are finite"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    reqs = [(d["x"][r].to(gpu), d["bert"][r].to(gpu), d["prompts"][r].to(gpu)) for r in range(2)]
    kw = dict(slots=64, wide=True, top_k=15, top_p=1, early_stop_num=12, seed=4242, logprobs=True)
    outs = list(model.decode_stream(reqs, n=40, **kw))
    assert model._infer().stream_stats["prefill_rows"] == [1, 1]
    one = {o.request: o for o in model.decode_stream(reqs, **kw)}
    P = d["prompts"].size(1)
    for r in range(2):
        mine = {o.candidate: o for o in outs if o.request == r}
        assert sorted(mine) == list(range(40)) and len({tuple(o.y.tolist()) for o in mine.values()}) > 1
        assert mine[0].idx == one[r].idx and torch.equal(mine[0].y, one[r].y)
        assert torch.equal(mine[0].logprobs, one[r].logprobs)
        for o in mine.values():
            drawn = o.y.numel() - P
            assert o.logprobs.shape[1] == 2 and o.logprobs.shape[0] >= drawn
            assert torch.isfinite(o.logprobs[:drawn]).all(), (r, o.candidate)
