"""CPU: the conditions tests/test_s1_ops_gpu.py rests on (tests/s1_refs.py).  The float64 references agree with torch's own
float64 autograd; ScaledAdamRef reproduces the reference optimiser's recorded trajectory (tests/golden/s1_small.pt); the
100-step trajectory inputs reach every branch they claim, with margin, so that no branch can flip between precisions; and
sum_bound is far below one dropped addend at the shapes the GPU tests run."""
import os

import pytest
import torch
import torch.nn.functional as F

import s1_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("with_r", [True, False], ids=["r", "nor"])
@pytest.mark.parametrize("C", [8, 520, 1024])
def test_layernorm_refs_match_autograd(C, with_r, family):
    d = R.ln_inputs(C, with_r, family, torch.float32)
    x = d["x"].double().requires_grad_(True)
    r = d["r"].double().requires_grad_(True) if with_r else None
    gm, bt = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    y_t = F.layer_norm(x + r if with_r else x, (C,), gm, bt, R.EPS_LN)
    y_t.backward(d["dy"].double())
    y, mean, rstd = R.add_ln_ref(d["x"], d["r"], d["gamma"], d["beta"], R.EPS_LN)
    dxr, dg, db, ag, ab = R.add_ln_bwd_ref(d["x"], d["r"], d["gamma"], d["dy"], mean, rstd)
    assert _rel(y, y_t.detach()) < 1e-12
    assert _rel(dxr, x.grad) < 1e-12 and (not with_r or torch.equal(x.grad, r.grad))
    assert _rel(dg, gm.grad) < 1e-12 and _rel(db, bt.grad) < 1e-12
    assert bool((ag >= dg.abs()).all()) and bool((ab >= db.abs()).all())
    t = d["x"].double() + (d["r"].double() if with_r else 0)
    assert _rel(mean, t.mean(1)) < 1e-12 and _rel(rstd, (t.var(1, unbiased=False) + R.EPS_LN).rsqrt()) < 1e-12


@pytest.mark.parametrize("kind", ["randn", "ranked", "flat", "hot"])
@pytest.mark.parametrize("V,ld", [(1, 1), (65, 72), (1025, 1088), (1100, 1152)])
def test_ce_ref_matches_autograd(V, ld, kind):
    logits, tg = R.ce_inputs(V, ld, 130, torch.float32, kind)
    ign = R.ce_ignore(V)
    row, tot, dl, hits = R.ce_ref(logits, tg, V, 3, ign, 0.25)
    z = logits[:, :V].double().requires_grad_(True)
    row_t = F.cross_entropy(z, tg, reduction="none")
    tot_t = F.cross_entropy(z, tg, reduction="sum")
    (tot_t * 0.25).backward()
    scale = max(1.0, float(row_t.detach().abs().max()))
    assert float((row - row_t.detach()).abs().max()) <= 1e-12 * scale
    assert abs(float(tot) - float(tot_t.detach())) <= 1e-12 * max(1.0, abs(float(tot_t.detach())))
    assert float((dl[:, :V] - z.grad).abs().max()) <= 1e-12
    assert bool((dl[:, V:] == 0).all()) and dl.shape == (130, ld)
    zz = logits[:, :V]
    keep = tg != ign
    want = int((((zz > zz.gather(1, tg[:, None])).sum(1) < 3) & keep).sum())
    assert hits == (want, int(keep.sum()))


def test_ce_inputs_cover_their_edges():
    for V, ld in R.CE_PAIRS:
        logits, tg = R.ce_inputs(V, ld, 130, torch.float32)
        assert bool(torch.isinf(logits[:, V:]).all()) and bool(torch.isfinite(logits[:, :V]).all())
        assert 0 in tg.tolist() and V - 1 in tg.tolist() and R.ce_ignore(V) in tg.tolist()
        assert torch.equal(logits[:, :V] * 8, torch.round(logits[:, :V] * 8))
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(R.stored(logits[:, :V], dt), logits[:, :V])
    # `ranked`: per top-k, rows on either side of the threshold, and exact ties with the target's logit
    logits, tg = R.ce_inputs(65, 72, 130, torch.float32, "ranked")
    z = logits[:, :65]
    lt = z.gather(1, tg[:, None])
    gt = (z > lt).sum(1)
    for k in (1, 3):
        assert int((gt == k - 1).sum()) > 0 and int((gt >= k).sum()) > 0
    assert int(((z == lt).sum(1) > 1).sum()) > 0


def test_round_bound_is_half_the_spacing():
    v = torch.tensor([1.0, 1.5, 1.999, 3.0, 1e-3, 300.0, 2.0 ** -20], dtype=F64)
    for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        half = 2.0 ** (torch.floor(torch.log2(v)) - bits)       # half the spacing of the binade of v (normal range)
        rb = R.round_bound(v, dt)
        normal = v >= (2.0 ** -14 if dt == torch.float16 else 0.0)
        assert bool((rb[normal] >= half[normal]).all()) and bool((rb[normal] < 2 * half[normal]).all())
        assert bool(((v.to(dt).double() - v).abs() <= rb * (1 + 2.0 ** -10)).all())
    assert float(R.round_bound(v, torch.float32).abs().max()) == 0.0
    assert float(R.round_bound(torch.tensor([1e-9]), torch.float16)) == 2.0 ** -25


def test_scaled_adam_ref_reproduces_the_recorded_trajectory():
    gold = torch.load(os.path.join(HERE, "golden", "s1_small.pt"), weights_only=False)["scaled_adam"]
    for dtype in (F64, torch.float32):
        opt = R.ScaledAdamRef(gold["init"], lr=0.01, betas=(0.9, 0.95), clipping_scale=2.0, clipping_update_period=4,
                              dtype=dtype)
        lr = 0.01
        assert len(gold["grads"]) == 14
        for step, (grads, want) in enumerate(zip(gold["grads"], gold["traj"])):
            opt.step(grads, lr)
            lr = 0.002
            for k, p in opt.params().items():
                assert torch.allclose(p.float(), want[k], rtol=1e-4, atol=3e-6), (dtype, step, k)
        assert opt.counters["clipped"] > 0


@pytest.fixture(scope="module")
def traj():
    run64, opt64 = R.traj_run(F64)
    run32, opt32 = R.traj_run(torch.float32)
    return run64, opt64, run32, opt32


def test_trajectory_reaches_every_branch_with_margin(traj):
    run64, opt64, run32, opt32 = traj
    assert max(max(s) for s in R.TRAJ_SHAPES.values()) <= 300 and all(torch.Size(s).numel() <= 300 for s in R.TRAJ_SHAPES.values())
    for opt in (opt64, opt32):
        c, m = opt.counters, opt.margins
        assert c["rms_above"] >= 1 and c["rms_below"] >= 1 and c["clipped"] >= 1 and c["scalar_clamped"] >= 1, c
        assert c["bc2_low"] >= 1 and c["bc2_high"] >= 1 and c["bc2_low"] + c["bc2_high"] == R.TRAJ_STEPS, c
        assert m["rms"] >= 0.2, m               # param_rms at least 20 % away from both clamps at every size update
        assert m["norms"] > 1e-3, m             # no two entries of the sorted norm history within 1e-3 relative
        assert m["bc2"] > 1e-4, m
    assert opt64.counters == opt32.counters     # the same branches in both precisions
    b = opt64.bc2_by_step
    first_high = next(i for i, v in enumerate(b) if v >= R.f32(0.99))
    assert first_high == 89 and abs(b[88] - 0.99) > 1e-4 and abs(b[89] - 0.99) > 1e-4 and b[88] < 0.99 < b[89]
    tol = R.traj_tolerance(run32, run64)
    worst = {k: max(v) for k, v in tol.items()}
    print("trajectory tolerance (8 x fp32-vs-float64 deviation), largest over the steps:", worst)
    for k, v in worst.items():                  # the yardstick is at fp32 rounding level, not a loose bound
        assert v <= 2e-4 * max(1e-5, float(run64[-1][k].abs().max())), (k, v)


def _droppable(move, bound, allow):
    """number of entries where dropping the addend is NOT more than 10 bounds away"""
    return int((move <= 10 * bound).sum()) <= allow


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("with_r", [True, False], ids=["r", "nor"])
@pytest.mark.parametrize("C", R.LN_CS)
def test_sum_bound_sees_a_dropped_row_layernorm(C, with_r, family):
    """for every row count and EVERY row: without that row dgamma and dbeta move by more than 10 bounds -- in all channels
    but the few (at most max(1, C / 10)) where that row's own term happens to be next to zero.  With the terms' own rounding
    added (the whole tolerance of the GPU test) the row still shows in more than half of the channels."""
    d = R.ln_inputs(C, with_r, family, torch.float32)
    for rows in R.LN_ROWS:
        sl = lambda t: None if t is None else t[:rows]
        y, mean, rstd = R.add_ln_ref(sl(d["x"]), sl(d["r"]), d["gamma"], d["beta"], R.EPS_LN)
        _, dg, db, ag, ab = R.add_ln_bwd_ref(sl(d["x"]), sl(d["r"]), d["gamma"], sl(d["dy"]), mean, rstd)
        depth = R.ln_bwd_depth(rows)
        bg = R.sum_bound(ag + d["pre_g"].abs(), depth)
        bb = R.sum_bound(ab + d["pre_b"].abs(), depth)
        # the whole dgamma tolerance of the GPU test: with the terms' own rounding (100 units per term in the offset family)
        bg_all = bg + R.ln_dgamma_term_error(sl(d["x"]), sl(d["r"]), sl(d["dy"]), rstd, ag)
        t = d["x"][:rows].double() + (d["r"][:rows].double() if with_r else 0)
        terms_g = d["dy"][:rows].double() * (t - mean[:, None]) * rstd[:, None]
        terms_b = d["dy"][:rows].double()
        for i in range(rows):
            assert _droppable(terms_g[i].abs(), bg, max(1, C // 10)), (rows, i)
            assert _droppable(terms_g[i].abs(), bg_all, C // 2), (rows, i)
            assert _droppable(terms_b[i].abs(), bb, max(1, C // 10)), (rows, i)


@pytest.mark.parametrize("V,ld", [p for p in R.CE_PAIRS if p[0] > 1])
def test_sum_bound_sees_a_dropped_row_cross_entropy(V, ld):
    """every row's loss is more than 10 bounds of the summed loss (V = 1 has loss 0 in every row: the bound is then 0 next
    to the preload's own 8 units and the sum has to come back as the preload).  The 8197-row case of the second sweep is
    NOT covered by this: its 2048 atomics make the worst-case bound 1.2e-4 of the sum, about one row; there the dropped row
    is caught by the per-row losses and the exact counters."""
    for rows in R.CE_ROWS:
        logits, tg = R.ce_inputs(V, ld, rows, torch.float32)
        row, tot, _, _ = R.ce_ref(logits, tg, V, 3, R.ce_ignore(V), 1.0)
        bound = R.sum_bound(float(row.abs().sum()) + abs(R.CE_PRELOAD), R.ce_depth(rows, V))
        assert float(row.min()) > 10 * bound, (rows, float(row.min()), bound)
    Vs, lds, rs = R.CE_SWEEP
    assert R.ce_depth(rs, Vs) == 2 + 3 + 2048 and R.ce_depth(130, 65) == 1 + 3 + 33 and R.ce_depth(130, 2500) == 130


def test_launch_geometry_counts():
    assert R.ln_bwd_geometry(67) == (16, 5) and R.ln_bwd_depth(67) == 4 + 3 + 5 and R.ln_bwd_depth(1) == 4 + 3 + 1
    assert R.ln_np(512, torch.float32) == (4, 2) and R.ln_np(520, torch.float32) == (4, 4)
    assert R.ln_np(512, torch.bfloat16) == (8, 1) and R.ln_np(520, torch.float16) == (8, 2)
    offs, total, chunks = R.sa_layout()
    per = [sum(1 for c in chunks if c[2] == t) for t in range(len(R.SA_NUMELS))]
    assert per == [1, 1, 1, 1, 1, 2, 3] and all(e - b <= R.SA_CHUNK for b, e, _ in chunks)
    assert sorted(e - b for b, e, t in chunks if t == 5) == [3, R.SA_CHUNK]
    a = R.sa_arena()
    assert int(a["live"].sum()) == sum(R.SA_NUMELS) and bool(torch.isnan(a["p"][~a["live"]]).all())
    assert bool(torch.isfinite(a["p"][a["live"]]).all()) and float(a["p"][offs[0]]) == 12.0 and float(a["p"][offs[1]]) == -12.0
    assert R.sa_stats_depth(chunks)[6] == 256 + 9 + 3 and R.sa_stats_depth(chunks)[0] == 1 + 9 + 1
    for s in R.SA_STEPS:                                # steps on both sides of the switch, none next to it
        assert abs(1 - R.f32(0.95) ** (s + 1) - 0.99) > 1e-4
    assert 1 - R.f32(0.95) ** 89 < 0.99 < 1 - R.f32(0.95) ** 90
