"""GPU: the s1 training kernels of csrc/s1_ops.hip through the C ABI, element by element against the float64 references of
tests/s1_refs.py: evt_add_layernorm_fwd / _bwd, evt_ce_sum_fwd_bwd_ld / evt_ce_rows_fwd_bwd_ld, evt_scaled_adam_stats /
_apply, and ScaledAdam.step() over 100 steps.  fp32, bf16 and (through hip.lib.set_half) the IEEE-half build.

Every output lies inside a larger buffer filled with a sentinel (NaN, or a bit pattern for the counters); after a launch
every output element is finite, every guard element is bit-identical.  16-bit operands are rounded to the stored type
before the reference sees them.

Tolerances (tests/s1_refs.py).  Element-wise outputs: |got - ref| <= round_bound(ref) * (1 + 2^-10) + slack, where slack is
4 x the largest deviation of the SAME formula evaluated in float32 on the CPU from its float64 evaluation (never the
kernel's numbers), taken once per case over its largest row count.  Sums (mean, rstd, dgamma, dbeta, the summed loss, the
ScaledAdam statistics): sum_bound over the kernel's launch geometry, plus what the terms themselves carry before they are
added (ln_dgamma_term_error; rows x the per-row loss slack; one unit per product).  Counters are exact.

Measured slacks (4 x the deviation of the fp32 CPU evaluation from float64; the largest over the cases of a family, all
three builds' inputs):
  LayerNorm randn family, 67 rows, C in {8 .. 1024}: y 3.6e-6 (|y| <= 4.9), mean 3.4e-7, rstd 8.5e-7, dxr 2.9e-6 (|dxr| <= 5.3)
  LayerNorm offset family (x + r ~ N(100, 1), fp32): y 9.9e-5, mean 7.4e-5, rstd 1.8e-5, dxr 7.6e-5 (|dxr| <= 8.4)
     (t = x + r rounds by 2^-18 at 100: 4e-6 of the normalised value, against 6e-8 in the randn family)
  cross entropy, 130 rows, all ten (V, ld) pairs:    row_loss 2.9e-6 (losses up to 14.6), dlogits 4.2e-7 (|dlogits| <= 1)
  cross entropy, 8197 rows, V 65, ld 72:             row_loss 3.0e-6, dlogits 8.6e-7
  cross entropy, logits + 3e4 (fp32):                row_loss 3.9e-3 (the spacing of fp32 at 3e4 is 2e-3), dlogits 3.6e-7
  cross entropy, +80 / -80 rows:                     row_loss 0 (every operation is exact), dlogits 1.3e-69 (exp(-160) -> 0)
  ScaledAdam apply, steps {0, 3, 88, 89, 500}:       param 1.9e-6 (|param| <= 12), delta 5.1e-9, exp_avg_sq 8.5e-9
All of them are a few fp32 roundings of the output's largest magnitude.  On an MI355X the kernels came to within 0.63 of
the slack at worst (dlogits, V 1089) and to about 0.25 - 0.35 elsewhere.

Trajectory tolerance (traj_tolerance: 8 x the deviation of ScaledAdamRef(float32) from ScaledAdamRef(float64), cumulative
over the steps), at step 99: big [12, 25] 5.0e-5 (|p| <= 16), wide [3, 5, 7] 7.9e-6, mid [17] 1.1e-6, tiny [40] 3.8e-12
(|p| ~ 1e-6), scalars 1.3e-5 / 7.5e-6 (|p| ~ 10) / 2.2e-7 (|p| ~ 0.2).
"""
import ctypes as C

import pytest
import torch

import s1_refs as R

pytestmark = pytest.mark.gpu

G = 64                                    # guard elements on either side (a multiple of 16 bytes in every type)
INT_SENT = 0x5A5A5A5A
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
F64 = torch.float64
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    return t.view(_BITS[t.element_size()])


class _Buf:
    """an output of `shape` at a 16-byte boundary inside a sentinel-filled buffer"""

    def __init__(self, shape, dtype, dev, values=None):
        n = 1
        for s in shape:
            n *= s
        fill = float("nan") if dtype.is_floating_point else INT_SENT
        self.whole = torch.full((n + 2 * G,), fill, dtype=dtype, device=dev)
        self.n = n
        self.view = self.whole[G:G + n].view(shape)
        assert self.view.data_ptr() % 16 == 0
        if values is not None:
            self.view.copy_(values.to(dtype))
        self.before = _bits(self.whole).clone()

    def guards_intact(self):
        now = _bits(self.whole)
        return torch.equal(now[:G], self.before[:G]) and torch.equal(now[G + self.n:], self.before[G + self.n:])

    def untouched(self):
        return torch.equal(_bits(self.whole), self.before)

    def get(self):
        """the output on the CPU; every element written (finite) and no guard element touched"""
        out = self.view.cpu()
        if out.dtype.is_floating_point:
            assert bool(torch.isfinite(out).all()), "an output element was not written (or is not finite)"
        assert self.guards_intact(), "a guard element next to the output was overwritten"
        return out


def _lib(dtype):
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    return L, L.lib(), L.dt_code(dtype)


def _within(got, ref, dtype, slack, what):
    ex = R.elementwise_excess(got, ref, dtype, slack)
    err = float((got.to(F64) - ref.to(F64)).abs().max())
    print(f"{what}: max |got - ref| {err:.3e}, slack {slack:.3e}, excess {ex:.3e}")
    assert ex <= 0.0, (what, err, slack, ex)


def _sum_within(got, ref, tol, what):
    err = (got.to(F64) - ref.to(F64)).abs()
    tol = torch.as_tensor(tol, dtype=F64)
    print(f"{what}: max |got - ref| {float(err.max()):.3e}, bound at that element {float(tol.expand_as(err).flatten()[int(err.argmax())]):.3e}")
    assert bool((err <= tol).all()), (what, float((err - tol).max()))


# ---- add + LayerNorm -------------------------------------------------------------------------------------------------------
def _ln_launch_fwd(L, lib, dt, dev, dtype, x, r, gamma, beta, rows, Cc, outs=None):
    y, mean, rstd = outs or (_Buf((max(rows, 1), Cc), dtype, dev), _Buf((max(rows, 1),), torch.float32, dev),
                             _Buf((max(rows, 1),), torch.float32, dev))
    rc = lib.evt_add_layernorm_fwd(dt, L.ptr(x), L.ptr(r), L.ptr(gamma), L.ptr(beta), L.ptr(y.view), L.ptr(mean.view),
                                   L.ptr(rstd.view), C.c_int64(rows), Cc, C.c_float(R.EPS_LN), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, y, mean, rstd


def _ln_launch_bwd(L, lib, dt, dev, dtype, x, r, gamma, dy, mean, rstd, rows, Cc, pre_g, pre_b):
    dxr = _Buf((max(rows, 1), Cc), dtype, dev)
    dg, db = _Buf((Cc,), torch.float32, dev, pre_g), _Buf((Cc,), torch.float32, dev, pre_b)
    rc = lib.evt_add_layernorm_bwd(dt, L.ptr(x), L.ptr(r), L.ptr(gamma), L.ptr(dy), L.ptr(mean), L.ptr(rstd),
                                   L.ptr(dxr.view), L.ptr(dg.view), L.ptr(db.view), C.c_int64(rows), Cc, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dxr, dg, db


def ln_slacks(d):
    """references over all 67 rows in float64, and the fp32 yardstick's slack per output"""
    ref = R.add_ln_ref(d["x"], d["r"], d["gamma"], d["beta"], R.EPS_LN)
    y32 = R.add_ln_ref(d["x"], d["r"], d["gamma"], d["beta"], R.EPS_LN, torch.float32)
    mean_in, rstd_in = ref[1].float(), ref[2].float()                 # the backward's statistics: fp32-rounded float64 ones
    bwd = R.add_ln_bwd_ref(d["x"], d["r"], d["gamma"], d["dy"], mean_in, rstd_in)
    b32 = R.add_ln_bwd_ref(d["x"], d["r"], d["gamma"], d["dy"], mean_in, rstd_in, torch.float32)
    slack = dict(y=R.slack_of(y32[0], ref[0]), mean=R.slack_of(y32[1], ref[1]), rstd=R.slack_of(y32[2], ref[2]),
                 dxr=R.slack_of(b32[0], bwd[0]))
    return ref, mean_in, rstd_in, bwd, slack


def _ln_case(dev, Cc, with_r, family, dtype):
    L, lib, dt = _lib(dtype)
    d = R.ln_inputs(Cc, with_r, family, dtype)
    (y64, mean64, rstd64), mean_in, rstd_in, (dxr64, _, _, _, _), slack = ln_slacks(d)
    print(f"LayerNorm C {Cc} r {with_r} {family} {dtype}: slacks {slack}")
    gamma, beta = d["gamma"].to(dev), d["beta"].to(dev)
    t64 = d["x"].double() + (d["r"].double() if with_r else 0)
    for rows in R.LN_ROWS:
        tag = f"C {Cc} rows {rows} r {with_r} {family} {dtype}"
        x = d["x"][:rows].to(dev, dtype).contiguous()
        r = d["r"][:rows].to(dev, dtype).contiguous() if with_r else None
        dy = d["dy"][:rows].to(dev, dtype).contiguous()
        # forward
        rc, y, mean, rstd = _ln_launch_fwd(L, lib, dt, dev, dtype, x, r, gamma, beta, rows, Cc)
        assert rc == L.EVT_OK, (tag, rc)
        _within(y.get(), y64[:rows], dtype, slack["y"], tag + " y")
        t = t64[:rows]
        dev_t = t - mean64[:rows, None]
        depth = R.ln_fwd_depth(Cc, dtype)
        abs_t = t.abs().sum(1)
        tol_mean = (R.sum_bound(abs_t, depth) + R.U * abs_t) / Cc + slack["mean"]
        _sum_within(mean.get(), mean64[:rows], tol_mean, tag + " mean")
        # rstd = (var + eps)^-1/2: d rstd = rstd^3 / 2 * d var; var is a sum of depth + 3 roundings (subtraction, square) per
        # chain, and carries the rounding u |t| of t = x + r through 2 |t - mean|
        dvar = (R.sum_bound((dev_t ** 2).sum(1), depth + 3) + 2 * R.U * (dev_t.abs() * t.abs()).sum(1)) / Cc
        tol_rstd = 0.5 * rstd64[:rows] ** 3 * dvar + slack["rstd"]
        _sum_within(rstd.get(), rstd64[:rows], tol_rstd, tag + " rstd")
        # backward on the fp32-rounded float64 statistics
        m_in, r_in = mean_in[:rows].to(dev).contiguous(), rstd_in[:rows].to(dev).contiguous()
        rc, dxr, dg, db = _ln_launch_bwd(L, lib, dt, dev, dtype, x, r, gamma, dy, m_in, r_in, rows, Cc, d["pre_g"], d["pre_b"])
        assert rc == L.EVT_OK, (tag, rc)
        _within(dxr.get(), dxr64[:rows], dtype, slack["dxr"], tag + " dxr")
        sl = lambda v: None if v is None else v[:rows]
        _, dg64, db64, ag, ab = R.add_ln_bwd_ref(sl(d["x"]), sl(d["r"]), d["gamma"], sl(d["dy"]), mean_in[:rows], rstd_in[:rows])
        bdepth = R.ln_bwd_depth(rows)
        tol_g = R.sum_bound(ag + d["pre_g"].abs(), bdepth) + R.ln_dgamma_term_error(sl(d["x"]), sl(d["r"]), sl(d["dy"]),
                                                                                  rstd_in[:rows], ag)
        tol_b = R.sum_bound(ab + d["pre_b"].abs(), bdepth)
        _sum_within(dg.get(), dg64 + d["pre_g"].double(), tol_g, tag + " dgamma")
        _sum_within(db.get(), db64 + d["pre_b"].double(), tol_b, tag + " dbeta")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_r", [True, False], ids=["r", "nor"])
@pytest.mark.parametrize("Cc", R.LN_CS)
def test_add_layernorm(gpu, Cc, with_r, dtype):
    _ln_case(gpu, Cc, with_r, "randn", dtype)


@pytest.mark.parametrize("with_r", [True, False], ids=["r", "nor"])
@pytest.mark.parametrize("Cc", R.LN_CS)
def test_add_layernorm_offset_family(gpu, Cc, with_r):
    """x + r ~ N(100, 1): E[t^2] - E[t]^2 in fp32 would leave 11 bits of the variance"""
    _ln_case(gpu, Cc, with_r, "offset", torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_layernorm_refusals(gpu, dtype):
    """C = 1032 (> 1024) and C = 12 (not a multiple of 8): not supported; rows = 0: invalid; nothing is written"""
    L, lib, dt = _lib(dtype)
    for Cc, rows, want in [(1032, 3, L.EVT_ENOTSUP), (12, 3, L.EVT_ENOTSUP), (512, 0, L.EVT_EINVAL)]:
        n = max(rows, 1)
        x = torch.randn(n, Cc, device=gpu).to(dtype)
        gamma, beta = torch.ones(Cc, device=gpu), torch.zeros(Cc, device=gpu)
        rc, y, mean, rstd = _ln_launch_fwd(L, lib, dt, gpu, dtype, x, x, gamma, beta, rows, Cc)
        assert rc == want, (Cc, rows, rc)
        assert y.untouched() and mean.untouched() and rstd.untouched(), (Cc, rows)
        st = torch.ones(n, device=gpu)
        rc, dxr, dg, db = _ln_launch_bwd(L, lib, dt, gpu, dtype, x, x, gamma, x, st, st, rows, Cc, torch.ones(Cc), torch.ones(Cc))
        assert rc == want, (Cc, rows, rc)
        assert dxr.untouched() and dg.untouched() and db.untouched(), (Cc, rows)


# ---- cross entropy ---------------------------------------------------------------------------------------------------------
def ce_slacks(logits, tg, V, dloss):
    ign = R.ce_ignore(V)
    r64 = R.ce_ref(logits, tg, V, 3, ign, dloss)
    r32 = R.ce_ref(logits, tg, V, 3, ign, dloss, torch.float32)
    return dict(row=R.slack_of(r32[0], r64[0]), dl=R.slack_of(r32[2], r64[2]))


def _ce_run(dev, dtype, logits, tg, V, slack, tag, api="sum", topk=3, dloss=1.0, with_dl=True, with_hits=True):
    """one launch of evt_ce_sum_fwd_bwd_ld (api "sum") or evt_ce_rows_fwd_bwd_ld ("rows") on logits [rows, ld], all checks"""
    L, lib, dt = _lib(dtype)
    rows, ld = logits.shape
    ign = R.ce_ignore(V)
    row64, tot64, dl64, hits64 = R.ce_ref(logits, tg, V, topk, ign, dloss)
    lg = logits.to(dev, dtype).contiguous()
    tgd = tg.to(dev)
    dl = _Buf((rows, ld), dtype, dev) if with_dl else None
    hits = _Buf((2,), torch.int32, dev, torch.tensor(R.HITS_PRELOAD, dtype=torch.int32)) if with_hits else None
    p_dl = L.ptr(dl.view if dl else None)
    p_hits = L.ptr(hits.view if hits else None)
    if api == "sum":
        out = _Buf((1,), torch.float32, dev, torch.tensor([R.CE_PRELOAD]))
        rc = lib.evt_ce_sum_fwd_bwd_ld(dt, L.ptr(lg), L.ptr(tgd), p_dl, L.ptr(out.view), p_hits, C.c_int64(rows), V,
                                       C.c_int64(ld), topk, C.c_int64(ign), C.c_float(dloss), L.stream_ptr())
    else:
        assert dloss == 1.0
        out = _Buf((rows,), torch.float32, dev)
        rc = lib.evt_ce_rows_fwd_bwd_ld(dt, L.ptr(lg), L.ptr(tgd), p_dl, L.ptr(out.view), p_hits, C.c_int64(rows), V,
                                        C.c_int64(ld), topk, C.c_int64(ign), L.stream_ptr())
    torch.cuda.synchronize()
    tag = f"{tag} {api} V {V} ld {ld} rows {rows} topk {topk} {dtype}"
    assert rc == L.EVT_OK, (tag, rc)
    if api == "sum":
        depth = R.ce_depth(rows, V)
        tol = R.sum_bound(float(row64.abs().sum()) + abs(R.CE_PRELOAD), depth) + rows * slack["row"]
        _sum_within(out.get(), (tot64 + R.CE_PRELOAD).reshape(1), tol, tag + " loss")
    else:
        _within(out.get(), row64, torch.float32, slack["row"], tag + " row_loss")
    if with_dl:
        got = dl.get()
        assert bool((got[:, V:] == 0).all()), tag + ": a padding column of dlogits is not an exact zero"
        _within(got, dl64, dtype, slack["dl"], tag + " dlogits")
    if with_hits:
        got = hits.get().tolist()
        want = [R.HITS_PRELOAD[0] + hits64[0], R.HITS_PRELOAD[1] + hits64[1]]
        assert got == want, (tag, got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V,ld", R.CE_PAIRS)
def test_cross_entropy_grid(gpu, V, ld, dtype):
    logits, tg = R.ce_inputs(V, ld, max(R.CE_ROWS), dtype)
    slack = ce_slacks(logits, tg, V, 1.0)
    print(f"CE V {V} ld {ld} {dtype}: slacks {slack}")
    for rows in R.CE_ROWS:
        for api in ("sum", "rows"):
            _ce_run(gpu, dtype, logits[:rows], tg[:rows], V, slack, "grid", api)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cross_entropy_second_sweep(gpu, dtype):
    """8197 rows on the 2048 x 4 waves of the cached kernel: five waves take a second row"""
    V, ld, rows = R.CE_SWEEP
    logits, tg = R.ce_inputs(V, ld, rows, dtype)
    slack = ce_slacks(logits, tg, V, 1.0)
    for api in ("sum", "rows"):
        _ce_run(gpu, dtype, logits, tg, V, slack, "sweep", api)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V,ld", [(65, 72), (1100, 1152)], ids=["cached", "generic"])
def test_cross_entropy_extras(gpu, V, ld, dtype):
    rows = max(R.CE_ROWS)
    logits, tg = R.ce_inputs(V, ld, rows, dtype, "ranked")
    slack = ce_slacks(logits, tg, V, 1.0)
    for topk in (1, 3, V + 1):
        for api in ("sum", "rows"):
            _ce_run(gpu, dtype, logits, tg, V, slack, "ranked", api, topk=topk)
    _ce_run(gpu, dtype, logits, tg, V, ce_slacks(logits, tg, V, 0.25), "dloss", "sum", dloss=0.25)
    for api in ("sum", "rows"):
        _ce_run(gpu, dtype, logits, tg, V, slack, "forward only", api, with_dl=False)
        _ce_run(gpu, dtype, logits, tg, V, slack, "no counters", api, with_hits=False)
    kinds = ["all_ignored", "flat", "hot"] + (["offset"] if dtype == torch.float32 else [])
    for kind in kinds:
        lk, tk = R.ce_inputs(V, ld, rows, dtype, kind)
        sk = ce_slacks(lk, tk, V, 1.0)
        print(f"CE {kind} V {V} {dtype}: slacks {sk}")
        for api in ("sum", "rows"):
            _ce_run(gpu, dtype, lk, tk, V, sk, kind, api)


# ---- ScaledAdam kernels ----------------------------------------------------------------------------------------------------
def _sa_chunks(L, dev, chunks):
    return L.struct_to_device([L.SAChunk(b, e, t, 0) for b, e, t in chunks], dev)


def test_scaled_adam_stats(gpu):
    L, lib, _ = _lib(torch.float32)
    a = R.sa_arena()
    nt = len(R.SA_NUMELS)
    tab = _sa_chunks(L, gpu, a["chunks"])
    p, g = a["p"].to(gpu), a["g"].to(gpu)
    stats = _Buf((nt, 3), torch.float32, gpu, a["pre"])
    rc = lib.evt_scaled_adam_stats(L.ptr(p), L.ptr(g), L.ptr(tab), len(a["chunks"]), L.ptr(stats.view), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.EVT_OK
    s64, abs64 = R.sa_stats_ref(a["p"], a["g"], a["chunks"])
    depth = torch.tensor(R.sa_stats_depth(a["chunks"]), dtype=F64)[:, None]
    tol = R.sum_bound(abs64 + a["pre"].abs().double(), depth) + R.U * abs64          # + one rounding per product
    _sum_within(stats.get(), s64 + a["pre"].double(), tol, "scaled_adam_stats")
    assert torch.equal(_bits(p.cpu()), _bits(a["p"])) and torch.equal(_bits(g.cpu()), _bits(a["g"]))


def sa_apply_refs(a, step):
    hp = R.hp_f32(dict(R.SA_HP, step=step))
    r64 = R.sa_apply_ref(a["p"], a["g"], a["delta"], a["v"], a["chunks"], a["coef"], hp)
    r32 = R.sa_apply_ref(a["p"], a["g"], a["delta"], a["v"], a["chunks"], a["coef"], hp, torch.float32)
    live = a["live"]
    return hp, r64, [R.slack_of(x[live], y[live]) for x, y in zip(r32, r64)]


@pytest.mark.parametrize("step", R.SA_STEPS)
def test_scaled_adam_apply(gpu, step):
    L, lib, _ = _lib(torch.float32)
    a = R.sa_arena()
    tab = _sa_chunks(L, gpu, a["chunks"])
    hp, r64, slacks = sa_apply_refs(a, step)
    print(f"ScaledAdam apply step {step}: slacks param / delta / exp_avg_sq {slacks}")
    g, coef = a["g"].to(gpu), a["coef"].to(gpu)
    bufs = [a[k].to(gpu) for k in ("p", "delta", "v")]
    hps = L.ScaledAdamHP(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["scalar_lr_scale"], hp["scalar_max"], step, 0)
    rc = lib.evt_scaled_adam_apply(L.ptr(bufs[0]), L.ptr(g), L.ptr(bufs[1]), L.ptr(bufs[2]), L.ptr(tab), len(a["chunks"]),
                                   L.ptr(coef), C.byref(hps), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.EVT_OK
    live = a["live"]
    for name, buf, before, ref, slack in zip(("param", "delta", "exp_avg_sq"), bufs, (a["p"], a["delta"], a["v"]), r64, slacks):
        got = buf.cpu()
        assert torch.equal(_bits(got)[~live], _bits(before)[~live]), f"step {step}: a gap element of {name} changed"
        assert bool(torch.isfinite(got[live]).all()), name
        assert not torch.equal(got[live], before[live]), name
        _within(got[live], ref[live], torch.float32, slack, f"step {step} {name}")
    for t in (0, 1):                                                # the scalars were clamped to +-scalar_max before the step
        assert abs(float(bufs[0][a["offs"][t]])) < 10.5


def test_scaled_adam_trajectory(gpu):
    """ScaledAdam.step() for 100 steps against ScaledAdamRef in float64: both rms clamps, a clipped step, the scalar clamp
    and both sides of the bias-correction switch (asserted on the CPU in tests/test_s1_refs_cpu.py).  Tolerance per tensor and
    step: traj_tolerance, 8 x the cumulative deviation of the fp32 reference run from the float64 one; measured at step 99:
    big 5.0e-5 (|p| <= 16), wide 7.9e-6, mid 1.1e-6, tiny 3.8e-12, scalars 1.3e-5 / 7.5e-6 / 2.2e-7."""
    from easevoice_trainer_amd.auto_reg.optim import ScaledAdam
    from easevoice_trainer_amd.runtime import ParamArena

    run64, opt64 = R.traj_run(F64)
    run32, _ = R.traj_run(torch.float32)
    tol = R.traj_tolerance(run32, run64)
    init = R.traj_init()

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for k, v in init.items():
                setattr(self, k, torch.nn.Parameter(v.clone()))

    h = Holder().to(gpu)
    arena = ParamArena(h, gpu)
    opt = ScaledAdam(arena, **R.TRAJ_KW)
    assert opt.names == list(init)
    params = dict(h.named_parameters())
    worst = {k: 0.0 for k in init}
    for step, (grads, want) in enumerate(zip(R.traj_grads(), run64)):
        arena.zero_grad()
        for k, g in grads.items():
            params[k].grad.copy_(g.to(gpu))
        opt.step()
        for k in params:
            err = float((params[k].detach().cpu().double() - want[k]).abs().max())
            worst[k] = max(worst[k], err / tol[k][step])
            assert err <= tol[k][step], (step, k, err, tol[k][step])
    print("trajectory: largest error / tolerance per tensor", worst)
