"""No GPU: the conditions the exact regime of tests/wn_refs.py rests on, checked on every element of every case, and the
teeth of both comparators -- a plain-torch, tile-by-tile emulation of the layer (16 own positions + a halo of 2 per tile,
as csrc/wn_layer.hip walks it) with ONE mistake seeded has to fail the bit-for-bit comparison AND exceed the
tolerance-regime bound by MUTATION_FACTOR on at least one element: a bound that swallows a whole dropped term is too loose.

Largest magnitudes reached, in steps of the tensor's step (limit 256), over the ten shapes (printed by this file under `-s`):
  forward   first_g 153   middle_g 169   middle 217   last_g_acc 170   last 219      (without g: x_in = 876 in steps of 4)
  backward  last_g 256    middle_g 256   middle 243   first_g 256   first_nodx 214   (256: x_in = +-512 - g = +-1024 in steps
            of 4, by construction; dx reaches 243 quarter steps)                     dg: at most 16 (limit 2^24 quarter steps)
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as X
import wn_refs as R

H, K, PAD, TILE = R.H, R.K, R.PAD, R.TILE
BF16 = torch.bfloat16
MUTATION_FACTOR = 100.0      # every seeded mistake is at least this many bounds off on some element (measured: 900 and more)


# ---- conditions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_exact_forward_operands_fit_the_stored_types(shape):
    for role in R.FWD_ROLES:
        p = R.exact_fwd_inputs(shape, role)
        ref = R.layer_forward(p, shape[2], role[1], BF16)
        st = R.fwd_steps(role)
        raw = ref["raw"]
        worst = 0.0
        for name, t in (("x", p["x"]), ("acc", p["acc"]), ("x_in", raw["x_in"]), ("acts", ref["acts"]), ("rs", raw["rs"]),
                        ("x_out", raw["x_out"]), ("acc_out", raw["acc_out"])):
            worst = max(worst, X.check_stored({f"{role[0]} {name}": t}, st[name]))
        print(f"forward {R.shape_id(shape)} {role[0]}: {worst:.0f} steps")
        # the gate stayed on the table's first two rows
        assert set(ref["acts"].unique().tolist()) <= {-1.0, 0.0, 1.0}
        if shape[1] * shape[0] >= 16:
            assert (ref["acts"] != 0).double().mean() > 0.25         # dense enough for rs to test the 1 x 1 convolution
        if not role[2]:          # without g the offset in b_in has to keep the gate saturated: wn_refs, "Forward without g"
            assert 128 <= float(raw["x_in"].abs().min()) and float(raw["x_in"].abs().max()) <= 896
        # no rounding happened anywhere
        assert torch.equal(ref["x_in"], raw["x_in"]) and torch.equal(ref["rs"], raw["rs"])
        assert torch.equal(ref["acc_out"], raw["acc_out"])
        assert ref["x_out"] is None or torch.equal(ref["x_out"], raw["x_out"])


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_exact_backward_operands_fit_the_stored_types(shape):
    for role in R.BWD_ROLES:
        p = R.exact_bwd_inputs(shape, role)
        ref = R.layer_backward(p, shape[2], role[1], BF16)
        raw = ref["raw"]
        worst = 0.0
        for name, t in (("x_in", p["x_in"]), ("dacc", p["dacc"]), ("dx_next", p["dx_next"]), ("drs", ref["drs"]),
                        ("dacts", raw["dacts"]), ("dx_in", raw["dx_in"]), ("dx", raw["dx"])):
            worst = max(worst, X.check_stored({f"{role[0]} {name}": t}, R.BWD_STEPS[name]))
        if ref["dg"] is not None:
            assert X.steps_of(ref["dg"], 0.25)[0]
            X.check_f32({"dg": ref["dg"] / 0.25})
        print(f"backward {R.shape_id(shape)} {role[0]}: {worst:.0f} steps"
              + (f", dg {float(ref['dg'].abs().max())}" if ref["dg"] is not None else ""))
        assert torch.equal(ref["dacts"], raw["dacts"]) and torch.equal(ref["dx_in"], raw["dx_in"])
        assert torch.equal(ref["dx"], raw["dx"])
        # the gradient rows of the table are present (and, with g, reach dg) wherever the shape has room for them
        if shape[0] * shape[1] >= 16:
            assert (ref["dx_in"][:, :H] != 0).any() and (ref["dx_in"][:, H:] != 0).any()
            if ref["dg"] is not None:
                assert (ref["dg"] != 0).sum() >= 4


def test_backward_formulas_are_the_autograd_of_the_forward():
    """wn_refs.layer_backward writes the chain rule out (as wn_layer_bwd's two epilogues do); here it is checked against autograd
    through conv1d / tanh / sigmoid in float64, on ordinary data, with the 16-bit rounding points switched off"""
    shape, lens = (3, 17, (17, 16, 2)), (17, 16, 2)
    for last in (False, True):
        role_f = ("t", last, True, True)
        p = R.tol_fwd_inputs(shape, role_f, torch.float64)
        pb = R.tol_bwd_inputs(shape, ("t", last, True, True), torch.float64)
        x = p["x"].clone().requires_grad_(True)
        g = p["g"].clone().requires_grad_(True)
        x_in = F.conv1d(x, p["w_in"], p["b_in"], padding=PAD)
        acts = torch.tanh(x_in[:, :H] + g[:, :H, None]) * torch.sigmoid(x_in[:, H:] + g[:, H:, None])
        rs = F.conv1d(acts, p["w_rs"], p["b_rs"])
        m = R.live(lens, 17)
        if last:
            loss = ((p["acc"] + rs) * m * pb["dacc"]).sum()
        else:
            loss = ((x + rs[:, :H]) * m * pb["dx_next"]).sum() + ((p["acc"] + rs[:, H:]) * pb["dacc"]).sum()
        dx, dg, dxin = torch.autograd.grad(loss, [x, g, x_in])
        ref = R.layer_backward(dict(pb, w_in=p["w_in"], w_rs=p["w_rs"], x_in=x_in.detach(), g=p["g"]), lens, last,
                               torch.float64)
        for got, want in ((dx, ref["dx"]), (dg, ref["dg"]), (dxin, ref["dx_in"])):
            assert (got - want).abs().max() <= 1e-12 * (1 + want.abs().max())


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_gate_exact_points(dt):
    """the table of tests/wn_refs.py in torch arithmetic: forward value and both gradients, for the two formulas the
    kernels state and for torch's own tanh / sigmoid"""
    d = torch.tensor([3.0, -5.0, 8.0], dtype=dt)
    rows = [  # a, b, acts, da / d, db / d
        (512.0, 512.0, 1.0, 0.0, 0.0), (-512.0, 512.0, -1.0, 0.0, 0.0), (768.0, 256.0, 1.0, 0.0, 0.0),
        (-256.0, 768.0, -1.0, 0.0, 0.0), (0.0, -512.0, 0.0, 0.0, 0.0), (4.0, -512.0, 0.0, 0.0, 0.0),
        (512.0, -512.0, 0.0, 0.0, 0.0), (-300.0, -256.0, 0.0, 0.0, 0.0),
        (0.0, 512.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 0.5, 0.0), (512.0, 0.0, 0.5, 0.0, 0.25), (-512.0, 0.0, -0.5, 0.0, -0.25),
    ]
    for a, b, acts, fa, fb in rows:
        av, bv = torch.full((3,), a, dtype=dt), torch.full((3,), b, dtype=dt)
        for form in ("exp2", "libm", "torch"):
            if form == "torch":
                t, s = torch.tanh(av), torch.sigmoid(bv)
            else:
                t, s = R.tanh_form(av, form), R.sigmoid_form(bv, form)
            got = (t * s).to(BF16).to(dt)          # (sigmoid(-256) is 1e-111 in float64: the stored value is what is owed)
            assert torch.equal(got, torch.full((3,), acts, dtype=dt)), (a, b, form, got)
            da, db = (d * s * (1 - t * t)).to(BF16).to(dt), (d * t * s * (1 - s)).to(BF16).to(dt)
            assert torch.equal(da, d * fa) and torch.equal(db, d * fb), (a, b, form, da, db)


def test_sweep_values_are_what_the_issue_counts():
    for dtype, lo in ((BF16, 2.0 ** -20), (torch.float16, 2.0 ** -24)):
        v = R.sweep_values(dtype)
        flat = v.flatten()
        assert torch.equal(flat.to(dtype).double(), flat)                     # all representable
        nz = flat[flat != 0].abs()
        assert float(nz.min()) == lo and float(nz.max()) == R.SAT
        assert float(nz[nz < R.SAT].max()) == 128.0
        assert flat.unique().numel() == 2 * ((0x4300 - 0x3580 + 1) if dtype == BF16 else 0x5800) + 3


# ---- the emulation: tile by tile, float64, the kernels' rounding points -----------------------------------------------------
def emu_forward(p, lens, last, dtype, mut=None):
    x = p["x"]
    B, _, T = x.shape
    x_in = torch.zeros(B, 2 * H, T, dtype=torch.float64)
    for q0 in range(0, T, TILE):
        rows = torch.zeros(B, H, TILE + 2 * PAD, dtype=torch.float64)            # positions q0 - 2 .. q0 + 17, zero outside
        for r in range(TILE + 2 * PAD):
            pos = q0 - PAD + r
            if 0 <= pos < T:
                rows[:, :, r] = x[:, :, pos]
        if mut == "halo_side":                                                   # the two halos change places
            rows = torch.cat([rows[:, :, TILE + PAD:], rows[:, :, PAD:TILE + PAD], rows[:, :, :PAD]], 2)
        y = F.conv1d(rows, p["w_in"], p["b_in"])                                 # [B, 2H, 16]
        if mut == "tap":                                                         # tap 0 dropped at the tile's first position
            y[:, :, 0] -= torch.einsum("oc,bc->bo", p["w_in"][:, :, 0], rows[:, :, 0])
        n = min(TILE, T - q0)
        x_in[:, :, q0:q0 + n] = y[:, :, :n]
    x_in = R.q(x_in, dtype)
    a, b = R.gate(x_in, p["g"])
    acts = R.q(torch.tanh(a) * torch.sigmoid(b), dtype)
    rs = R.q(F.conv1d(acts, p["w_rs"], p["b_rs"]), dtype)
    m = R.live(lens, T)
    if mut == "mask_L":
        m = torch.ones_like(m)
    acc = torch.zeros_like(x) if (p["acc"] is None or mut == "no_acc") else p["acc"]
    if last:
        return dict(x_in=x_in, acts=acts, x_out=None, acc_out=R.q((acc + rs) * m, dtype))
    return dict(x_in=x_in, acts=acts, x_out=R.q((x + rs[:, :H]) * m, dtype), acc_out=R.q(acc + rs[:, H:], dtype))


def emu_backward(p, lens, last, dtype, mut=None):
    dacc = p["dacc"]
    B, _, T = dacc.shape
    m = R.live(lens, T)
    if last:
        drs = dacc * (torch.ones_like(m) if mut == "last_drs" else m)
        dxn = None
    else:
        dxn = torch.zeros_like(dacc) if p["dx_next"] is None else p["dx_next"] * (torch.ones_like(m) if mut == "dxn" else m)
        drs = torch.cat([dxn, dacc], 1)
    dacts = R.q(torch.einsum("och,bot->bct", p["w_rs"], drs), dtype)
    a, b = R.gate(p["x_in"], p["g"])
    t, s = torch.tanh(a), torch.sigmoid(b)
    dpre = torch.cat([dacts * s * (1 - t * t), dacts * t * s * (1 - s)], 1)
    dx_in = R.q(dpre, dtype)
    dg = None
    if p["g"] is not None:
        dg = torch.zeros(B, 2 * H, dtype=torch.float64)
        for q0 in range(0, T, TILE):
            own = list(range(q0, min(q0 + TILE, T)))
            halo = [q for q in (q0 - 2, q0 - 1, q0 + TILE, q0 + TILE + 1) if 0 <= q < T] if mut == "dg_halo" else []
            dg += dpre[:, :, own + halo].sum(2)
    dx = torch.zeros(B, H, T, dtype=torch.float64)
    for pos in range(T):                                                         # dx[pos] = sum_tap w[:, :, tap]^T dx_in[pos + 2 - tap]
        for tap in range(K):
            src = pos + PAD - tap
            if 0 <= src < T:
                dx[:, :, pos] += torch.einsum("oc,bo->bc", p["w_in"][:, :, tap], dx_in[:, :, src])
    if not last:
        dx = dx + dxn
    return dict(drs=drs, dx_in=dx_in, dx=R.q(dx, dtype), dg=dg)


FWD_MUTATIONS = [("tap", "first_g"), ("tap", "middle"), ("halo_side", "middle_g"), ("halo_side", "last"),
                 ("mask_L", "middle_g"), ("mask_L", "middle"), ("no_acc", "middle_g"), ("no_acc", "middle")]
BWD_MUTATIONS = [("dg_halo", "middle_g"), ("dg_halo", "last_g"), ("dxn", "middle_g"), ("dxn", "middle"), ("last_drs", "last_g")]
MUT_SHAPE = R.SHAPES[8]          # (4, 50, (50, 48, 47, 3)): four tiles, three of them with both neighbours
_role = lambda roles, name: next(r for r in roles if r[0] == name)


def _differs(got, want, dtype, names):
    """does the bit-for-bit comparator fail on one of the outputs?"""
    failed = []
    for n in names:
        if want[n] is None:
            continue
        try:
            if n == "dg":
                X.assert_exact(got[n].float(), want[n], torch.float32, n, nlc=False)
            else:
                X.assert_exact(got[n].transpose(1, 2).to(dtype), want[n], dtype, n)
        except AssertionError:
            failed.append(n)
    return failed


@pytest.mark.parametrize("shape", [R.SHAPES[2], R.SHAPES[5], R.SHAPES[8]], ids=R.shape_id)
def test_emulation_without_a_mistake_is_the_reference(shape):
    for role in R.FWD_ROLES:
        p = R.exact_fwd_inputs(shape, role)
        assert not _differs(emu_forward(p, shape[2], role[1], BF16), R.layer_forward(p, shape[2], role[1], BF16), BF16,
                            ("x_in", "acts", "x_out", "acc_out"))
        p = R.tol_fwd_inputs(shape, role, BF16)
        out = R.fwd_checks(p, shape[2], role[1], BF16, emu_forward(p, shape[2], role[1], BF16), "exp2")
        assert all(e <= 0 for e, _r in out.values()), out
    for role in R.BWD_ROLES:
        p = R.exact_bwd_inputs(shape, role)
        assert not _differs(emu_backward(p, shape[2], role[1], BF16), R.layer_backward(p, shape[2], role[1], BF16), BF16,
                            ("drs", "dx_in", "dx", "dg"))
        p = R.tol_bwd_inputs(shape, role, BF16)
        out = R.bwd_checks(p, shape[2], role[1], BF16, emu_backward(p, shape[2], role[1], BF16), "exp2")
        assert all(e <= 0 for e, _r in out.values()), out


@pytest.mark.parametrize("mut,role_name", FWD_MUTATIONS, ids=[f"{m}-{r}" for m, r in FWD_MUTATIONS])
def test_forward_mutation_is_caught(mut, role_name):
    role, shape = _role(R.FWD_ROLES, role_name), MUT_SHAPE
    p = R.exact_fwd_inputs(shape, role)
    bad = _differs(emu_forward(p, shape[2], role[1], BF16, mut), R.layer_forward(p, shape[2], role[1], BF16), BF16,
                   ("x_in", "acts", "x_out", "acc_out"))
    assert bad, f"{mut}: the exact comparator saw nothing"
    for dtype in (BF16, torch.float16):
        p = R.tol_fwd_inputs(shape, role, dtype)
        out = R.fwd_checks(p, shape[2], role[1], dtype, emu_forward(p, shape[2], role[1], dtype, mut), "exp2")
        worst = max(r for _e, r in out.values())
        print(f"{mut} {role_name} {dtype}: exact comparator fails on {bad}; {worst:.3g} bounds off")
        assert worst >= MUTATION_FACTOR, out


@pytest.mark.parametrize("mut,role_name", BWD_MUTATIONS, ids=[f"{m}-{r}" for m, r in BWD_MUTATIONS])
def test_backward_mutation_is_caught(mut, role_name):
    role, shape = _role(R.BWD_ROLES, role_name), MUT_SHAPE
    p = R.exact_bwd_inputs(shape, role)
    bad = _differs(emu_backward(p, shape[2], role[1], BF16, mut), R.layer_backward(p, shape[2], role[1], BF16), BF16,
                   ("drs", "dx_in", "dx", "dg"))
    assert bad, f"{mut}: the exact comparator saw nothing"
    for dtype in (BF16, torch.float16):
        p = R.tol_bwd_inputs(shape, role, dtype)
        out = R.bwd_checks(p, shape[2], role[1], dtype, emu_backward(p, shape[2], role[1], dtype, mut), "exp2")
        worst = max(r for _e, r in out.values())
        print(f"{mut} {role_name} {dtype}: exact comparator fails on {bad}; {worst:.3g} bounds off")
        assert worst >= MUTATION_FACTOR, out
