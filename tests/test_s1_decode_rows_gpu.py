"""GPU: wide decode sessions of 5..32 rows (csrc/s1_decode_rows.hip, evt_dec_sample_rows, auto_reg/t2s_infer.py).
The wide linear against torch fp32 and evt_dec_gemv, the row-seeded sampler against evt_dec_sample in groups of four, and
the whole batch decode against the reference's token lists (tests/golden/s1_batch_infer_rows.pt) and against the same
texts decoded four at a time."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F
import yaml

from util_fill import fill_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

SHAPES = [(1536, 512), (512, 512), (2048, 512), (512, 2048), (1025, 512)]   # qkv, out-proj, ffn1, ffn2, logits


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _linear(gpu, fn, Wg, bias, a, r, lg, lb, B, relu, use_ln):
    from easevoice_trainer_amd.hip import lib as L

    N, K = Wg.shape
    y = torch.full((B, N), float("nan"), device=gpu)
    xo = torch.full((B, K), -7.0, device=gpu)
    args = [a, r, lg, lb] if use_ln else [a, None, None, None]
    L.check(getattr(L.lib(), fn)(L.dt_of(Wg), L.ptr(Wg), L.ptr(bias), L.ptr(args[0]), L.ptr(args[1]), L.ptr(args[2]),
                                 L.ptr(args[3]), C.c_float(1e-5), L.ptr(xo) if use_ln else None, L.ptr(y), B, N, K, relu,
                                 L.stream_ptr()), fn)
    torch.cuda.synchronize()
    return y, xo


def _case(B, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    bias, a, r = torch.randn(N, generator=g), torch.randn(B, K, generator=g), torch.randn(B, K, generator=g)
    lg, lb = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    return W, bias, a, r, lg, lb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
@pytest.mark.parametrize("B", [5, 8, 20, 32])
def test_dec_gemm_rows(gpu, dtype, shape, B):
    """y = act(bias + W.x) with x = a or LayerNorm(a + r) against torch fp32 (test_dec_gemv's tolerances), bitwise
    repeatable; the logits (N = 1025, not a multiple of 16) have no bias"""
    N, K = shape
    W, bias, a, r, lg, lb = _case(B, N, K, dtype, N + K + B)
    dev = lambda t: t.to(gpu)
    Wg, bg = dev(W), (None if N == 1025 else dev(bias))
    for use_ln in (False, True):
        for relu in (0, 1):
            x = F.layer_norm(a + r, (K,), lg, lb, 1e-5) if use_ln else a
            want = x @ W.float().t() + (0.0 if N == 1025 else bias)
            want = want.clamp(min=0) if relu else want
            y, xo = _linear(gpu, "evt_dec_gemm_rows", Wg, bg, dev(a), dev(r), dev(lg), dev(lb), B, relu, use_ln)
            assert rel(y, want) < 2e-5, (use_ln, relu)
            if use_ln:
                assert rel(xo, x) < 1e-5
            y2, xo2 = _linear(gpu, "evt_dec_gemm_rows", Wg, bg, dev(a), dev(r), dev(lg), dev(lb), B, relu, use_ln)
            assert torch.equal(y, y2) and torch.equal(xo, xo2)


def test_dec_gemm_rows_f16_build(gpu):
    """the IEEE-half build of the library (fp16_run) serves the same entry point"""
    from easevoice_trainer_amd.hip import lib as L

    B, N, K = 20, 2048, 512
    W, bias, a, r, lg, lb = _case(B, N, K, torch.float16, 5)
    L.set_half(torch.float16)
    try:
        x = F.layer_norm(a + r, (K,), lg, lb, 1e-5)
        want = (x @ W.float().t() + bias).clamp(min=0)
        y, xo = _linear(gpu, "evt_dec_gemm_rows", W.to(gpu), bias.to(gpu), a.to(gpu), r.to(gpu), lg.to(gpu), lb.to(gpu),
                        B, 1, True)
        assert rel(y, want) < 2e-5 and rel(xo, x) < 1e-5
    finally:
        L.set_half(torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 4])
def test_dec_gemm_rows_small_batches_match_gemv(gpu, dtype, B):
    """at the row counts evt_dec_gemv serves, both entry points agree (only the order of the fp32 sums differs)"""
    for N, K in SHAPES:
        W, bias, a, r, lg, lb = _case(B, N, K, dtype, 3 * N + K)
        args = [t.to(gpu) for t in (W, bias, a, r, lg, lb)]
        use_ln = K == 512
        y1, x1 = _linear(gpu, "evt_dec_gemv", *args, B, 1, use_ln)
        y2, x2 = _linear(gpu, "evt_dec_gemm_rows", *args, B, 1, use_ln)
        assert rel(y2, y1) < 2e-5, (N, K)
        if use_ln:
            assert rel(x2, x1) < 1e-5


def test_dec_sample_rows_equals_groups_of_four(gpu):
    """12 rows with the row-seed table (s + 4 * (b // 4), b % 4) draw bit for bit what three 4-row evt_dec_sample calls
    seeded s, s + 4, s + 8 draw: tokens, stop flags, probabilities"""
    from easevoice_trainer_amd.hip import lib as L

    B, V, ycount, idx, s = 12, 1025, 20, 14, 0x1234567
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(B, V, generator=g) * 3).to(gpu)
    logits[5, 1024] = 40.0                                    # one row stops on EOS
    y = torch.zeros(B, 512, dtype=torch.int64)
    y[:, :ycount] = torch.randint(0, 1024, (B, ycount), generator=g)
    sp = L.SampleParams(V, 1024, 15, 11, 512, 1.0, 1.0, 1.35, 123, 1)

    def ctr_of(seed):
        return torch.tensor([0, idx, ycount, 0, seed, 0, 0, 0], dtype=torch.int32, device=gpu)

    yw, stop_w, probs_w = y.to(gpu), torch.full((B,), -1, dtype=torch.int32, device=gpu), torch.empty(B, V, device=gpu)
    rs = torch.tensor([[s + 4 * (b // 4), b % 4] for b in range(B)], dtype=torch.int32, device=gpu)
    cw = ctr_of(0)
    L.check(L.lib().evt_dec_sample_rows(C.byref(sp), L.ptr(logits), L.ptr(yw), L.ptr(cw), None, L.ptr(stop_w),
                                        L.ptr(probs_w), L.ptr(rs), B, L.stream_ptr()), "evt_dec_sample_rows")
    yg, stop_g, probs_g = y.to(gpu), torch.full((B,), -1, dtype=torch.int32, device=gpu), torch.empty(B, V, device=gpu)
    ctrs = [ctr_of(s + 4 * k) for k in range(3)]
    for k in range(3):
        rows = slice(4 * k, 4 * k + 4)
        lgk, yk, sk, pk = logits[rows].contiguous(), yg[rows].contiguous(), stop_g[rows].contiguous(), probs_g[rows].contiguous()
        L.check(L.lib().evt_dec_sample(C.byref(sp), L.ptr(lgk), L.ptr(yk), L.ptr(ctrs[k]), None, L.ptr(sk), L.ptr(pk), 4,
                                       L.stream_ptr()), "evt_dec_sample")
        torch.cuda.synchronize()
        yg[rows], stop_g[rows], probs_g[rows] = yk, sk, pk
    torch.cuda.synchronize()
    assert torch.equal(yw, yg) and torch.equal(stop_w, stop_g) and torch.equal(probs_w, probs_g)
    assert int(stop_w[5]) == idx and len(set(yw[:, ycount].tolist())) > 3


@pytest.fixture(scope="module")
def model(gpu):
    from easevoice_trainer_amd.train.s1_engine import S1Engine

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    eng = S1Engine(cfg, gpu, torch.float32)
    fill_module(eng.model, 3)
    eng.model.eval()
    return eng.model


def _batch(m, gpu, d, rows, **kw):
    return m.infer_panel_batch_infer([d["x"][r].to(gpu) for r in rows], d["x_lens"][rows].to(gpu),
                                     d["prompts"][rows].to(gpu), [d["bert"][r].to(gpu) for r in rows], **kw)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_rows_decoding_matches_reference_tokens(gpu, model, graph, monkeypatch):
    """20 texts in one session, 36 texts in a session of 32 and one of 4: the reference's token lists, fp32"""
    from make_golden_s1_rows import rows_inputs

    monkeypatch.setenv("EVT_DECODE_GRAPH", graph)
    for gold in torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"), weights_only=False)["cases"]:
        a = dict(gold["args"])
        R = a.pop("R")
        d = rows_inputs(R)
        ys, idxs = _batch(model, gpu, d, list(range(R)), noise=d["q"], **a)
        assert idxs == gold["idx"], (R, idxs, gold["idx"])
        for r, (y, g) in enumerate(zip(ys, gold["y"])):
            assert torch.equal(y.cpu().long(), g.long()), (R, r)


def test_rows_seeds_match_groups_of_four(gpu, model):
    """the built-in noise of a 10-row session is, row for row, that of the same texts decoded four at a time with the
    group seeds -- seeded, and unseeded under torch.manual_seed (every group holds the longest text, so the key
    positions agree)"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    order = [0, 3, 5, 7, 0, 2, 4, 6, 0, 1]
    kw = dict(top_k=15, top_p=1, early_stop_num=12)
    s = 4242
    ys, idxs = _batch(model, gpu, d, order, seed=s, **kw)
    for k, g0 in enumerate(range(0, 10, 4)):
        rows = order[g0:g0 + 4]
        yg, ig = _batch(model, gpu, d, rows, seed=s + g0, **kw)
        assert ig == idxs[g0:g0 + 4]
        for y1, y2 in zip(ys[g0:g0 + 4], yg):
            assert torch.equal(y1, y2), k
    torch.manual_seed(9)
    ys, idxs = _batch(model, gpu, d, order, **kw)
    torch.manual_seed(9)
    ref = [_batch(model, gpu, d, order[g0:g0 + 4], **kw) for g0 in range(0, 10, 4)]
    assert [i for _, ig in ref for i in ig] == idxs
    assert all(torch.equal(y1, y2) for y1, y2 in zip(ys, [y for yg, _ in ref for y in yg]))
    assert not torch.equal(ys[0], ys[4])                      # the same text in another group draws other noise


def test_rows_bf16_repeatable(gpu, model):
    """20 rows in bf16 under one seed: the same tokens twice, all of them valid"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    model.cd = torch.bfloat16
    try:
        out = [_batch(model, gpu, d, list(range(20)), top_k=15, top_p=1, early_stop_num=30, seed=77) for _ in range(2)]
    finally:
        model.cd = torch.float32
    (ys1, i1), (ys2, i2) = out
    assert i1 == i2 and len(ys1) == 20
    assert all(torch.equal(a, b) for a, b in zip(ys1, ys2))
    for y, i in zip(ys1, i1):
        assert 0 <= i <= 30 and int(y.min()) >= 0 and int(y[12:].max()) <= 1024 and y.numel() > 12
