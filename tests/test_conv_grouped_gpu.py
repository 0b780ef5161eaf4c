"""GPU: the grouped k = 41, stride-4 convolutions of DiscriminatorS (csrc/conv_grouped.hip), 16-bit kernels: weights in
registers, register-prefetched tiles, 16 groups per block, 16-position sub-tiles in a partial last tile, the add operand
of backward-data.

Oracle: oracle.ops.conv_block on the CPU, differentiated by autograd; tolerances of tests/test_conv_gpu.py (relative to the
tensor's max-abs: 3e-2 bfloat16, 6e-3 IEEE half, 1e-3 fp32).  The integer-valued variant (operands of tests/exact_inputs.py)
makes every fp32 sum exact, so y, dx and dW have to equal the oracle bit for bit: a position counted twice or not at all
cannot hide.  impl = naive (the direct kernels) is the independent second implementation on the GPU.

Shapes: the four layer geometries at lout = 23 / 64 / 65 / 80 (a lone partial tile, an exact tile, one element into a second
tile, the benchmark's 64 + 16), two sequences of random data (a halo row read across the sequence boundary shows), and one
case per geometry family in which every block walks three or more tiles with a partial one among them -- the only place the
prefetch and the reuse of the LDS stage run.  That case asserts its premise from the launcher's grid rule, restated in
_blocks_x / _wgrad_split below."""
import pytest
import torch

import exact_inputs as X
from oracle import ops as O

pytestmark = pytest.mark.gpu

K, STRIDE, PAD, PT = 41, 4, 20, 64
GEOMS = dict(g4=(16, 64, 4), g16=(64, 256, 16), g64=(256, 1024, 64), g256=(1024, 1024, 256))
LINS = (90, 256, 260, 320)           # lout 23, 64, 65, 80
TOL = {torch.float32: 1e-3, torch.bfloat16: 3e-2, torch.float16: 6e-3}
HALVES = dict(bf16=torch.bfloat16, f16=torch.float16)
NAIVE, AUTO = 1, 0
FUSIONS = [
    dict(name="plain", in_slope=1.0, out_act=0, out_slope=1.0),
    dict(name="slope_in", in_slope=0.1, out_act=0, out_slope=1.0),
    dict(name="lrelu_out", in_slope=1.0, out_act=1, out_slope=0.1),            # y is the derivative operand of both backwards
    dict(name="tanh_out", in_slope=1.0, out_act=2, out_slope=1.0),
]
# A leaky-relu on load TOGETHER with a leaky-relu on the output runs on integer operands only (INT_FUSIONS): the 16-bit
# kernels round lrelu(x) to the storage type before the MFMA, which moves y by 2^-9 of its terms in bfloat16 and flips the
# sign of outputs near zero; act' then differs by 1 - slope on those elements and one flip is a 10 % error of dx -- no
# bound relative to max-abs holds for that, whereas exact integer sums have no such flips.
# integer operands: power-of-two slopes, no tanh; budgets (tx / tdy products per element) as tests/exact_inputs.py::FUSIONS;
# for both slopes (eighth-steps): sigma = 15.8 sqrt(T) steps forward, 11.5 sqrt(T) backward, 256 steps at 6.5 sigma,
# less the bias (up to 16 steps): T = 4 and 8
INT_FUSIONS = [
    dict(name="plain", in_slope=1.0, out_act=0, out_slope=1.0, res=False, step=1.0, tx=160, tdy=160),
    dict(name="slope_in", in_slope=0.5, out_act=0, out_slope=1.0, res=False, step=0.5, tx=64, tdy=40),
    dict(name="lrelu_out", in_slope=1.0, out_act=1, out_slope=0.25, res=False, step=0.25, tx=12, tdy=16),
    dict(name="slope_in_lrelu_out", in_slope=0.5, out_act=1, out_slope=0.25, res=False, step=0.125, tx=4, tdy=8),
]


def _case(geom, lin, nseq):
    cin, cout, groups = GEOMS[geom]
    return (cin, cout, K, STRIDE, PAD, 1, groups, False, False, lin, nseq)


def _lout(lin):
    return (lin + 2 * PAD - (K - 1) - 1) // STRIDE + 1


@pytest.fixture(params=list(HALVES), ids=list(HALVES))
def half(request):
    from easevoice_trainer_amd.hip import lib as L

    dtype = HALVES[request.param]
    L.set_half(dtype)
    yield dtype
    L.set_half(torch.bfloat16)


# ---- references, computed once per (case, fusion, dtype) and shared ------------------------------------------------------
_REF = {}


def _reference(case, fusion, dtype):
    """random operands rounded to `dtype` and the oracle's y, dx, dW, db (fp32, reference layout [nseq, C, L])"""
    key = (case, fusion["name"], dtype)
    if key in _REF:
        return _REF[key]
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    g = X.gen("grouped", case, fusion["name"])
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).float()
    w = (torch.randn(cout, cin // groups, k, generator=g) * 0.2).to(dtype).float()    # (stored values of `dtype`, like x and dy)
    b = rnd(cout)
    x, dy = rnd(nseq, cin, lin), rnd(nseq, cout, _lout(lin))
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y = O.conv_block(leaves[0], leaves[1], leaves[2], None, stride=stride, pad=pad, dil=dil, groups=groups,
                     in_slope=fusion["in_slope"], out_act=fusion["out_act"], out_slope=fusion["out_slope"])
    if fusion["out_act"] == 1:
        # the kernels take act' from the sign of the STORED output: no upstream gradient where the output is within the
        # accumulation noise of zero (tests/test_conv_gpu.py::_run_case)
        dy = dy.masked_fill(y.detach().abs() < 1e-4, 0.0)
    dx, dw, db = torch.autograd.grad(y, leaves, dy)
    _REF[key] = dict(x=x, w=w, bias=b, dy=dy, y=y.detach(), dx=dx, dW=dw, db=db)
    return _REF[key]


def _run(gpu, case, fusion, dtype, impl, ops):
    """forward + backward of one module on the GPU; returns y, dx (channels-last), dW, db and the launch tags"""
    from easevoice_trainer_amd.hip import conv as HC

    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    m = HC.EvtConv1d(cin, cout, k, stride, pad, dil, groups, bias=True, transposed=False, weight_norm=False)
    with torch.no_grad():
        m.weight.copy_(ops["w"])
        m.bias.copy_(ops["bias"])
    m = m.to(gpu)
    bank = HC.WeightBank(m, dtype, gpu, impl=impl)
    bank.build_tables()
    bank.fold()
    nlc = lambda t: t.transpose(1, 2).contiguous().to(gpu, dtype)
    xg = nlc(ops["x"]).requires_grad_(True)
    rec = []
    HC.set_trace(rec)
    try:
        y = m(xg, None, fusion["in_slope"], fusion["out_act"], fusion["out_slope"])
        y.backward(nlc(ops["dy"]))
        bank.grads()
        torch.cuda.synchronize()
    finally:
        HC.set_trace(None)
    tags = {(r[1], r[0]) for r in rec}
    return dict(y=y.detach(), dx=xg.grad, dW=m.weight.grad.detach(), db=m.bias.grad.detach()), tags


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def _ncl(t):
    return t.transpose(1, 2)


def _compare(got, ref, tol, ctx):
    for name in ("y", "dx"):
        err = _rel(_ncl(got[name]), ref[name])
        assert err < tol, f"{name}: rel err {err:.3e} (tol {tol}) {ctx}"
    for name in ("dW", "db"):
        err = _rel(got[name], ref[name])
        assert err < tol, f"{name}: rel err {err:.3e} (tol {tol}) {ctx}"


def _grouped_tags(tags, fusion):
    assert ("fwd", "grouped_fwd") in tags, tags
    assert ("bwd_weight", "grouped_bwd_weight") in tags, tags
    if fusion["in_slope"] == 1.0:      # (with a leaky-relu on load the input gradient needs the gate: generic path)
        assert ("bwd_data", "grouped_bwd_data") in tags, tags


@pytest.mark.parametrize("lin", LINS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_tile_edges_vs_oracle_and_direct_kernels(gpu, half, geom, lin):
    """every fusion at every tile edge, two sequences of random data: the grouped kernels against the CPU oracle, the direct
    kernels (impl = naive) against the same oracle, and the two GPU implementations against each other"""
    case = _case(geom, lin, 2)
    for fusion in FUSIONS:
        ref = _reference(case, fusion, half)
        ctx = f"[{geom} L{lin} {fusion['name']} {half}]"
        got, tags = _run(gpu, case, fusion, half, AUTO, ref)
        _grouped_tags(tags, fusion)
        _compare(got, ref, TOL[half], ctx + " grouped vs oracle")
        direct, dtags = _run(gpu, case, fusion, half, NAIVE, ref)
        assert not any(t.startswith("grouped") for _, t in dtags), dtags
        _compare(direct, ref, TOL[half], ctx + " direct vs oracle")
        for name in ("y", "dx", "dW", "db"):
            err = _rel(got[name], direct[name])
            assert err < TOL[half], f"{name}: grouped vs direct kernels rel err {err:.3e} {ctx}"


def _int_reference(case, fusion):
    key = (case, "int:" + fusion["name"])
    if key in _REF:
        return _REF[key]
    cin, cout, k, stride, pad, dil, groups = case[:7]
    inp = X.conv_inputs(case, fusion)
    # fp32 is as exact as float64 here (integer sums far below 2^24 steps) and several times faster on the long cases
    dt = torch.float32 if X.heavy(case) or case[-1] > 2 else torch.float64
    x, w, b = (inp[n].to(dt).clone().requires_grad_(True) for n in ("x", "w", "bias"))
    y = O.conv_block(x, w, b, None, stride=stride, pad=pad, dil=dil, groups=groups, in_slope=fusion["in_slope"],
                     out_act=fusion["out_act"], out_slope=fusion["out_slope"])
    dx, dw, db = torch.autograd.grad(y, (x, w, b), inp["dy"].to(dt))
    ref = dict(x=inp["x"], w=inp["w"], bias=inp["bias"], dy=inp["dy"], y=y.detach().double(), dx=dx.double(),
               dW=dw.double(), db=db.double())
    X.check_stored(dict(x=ref["x"], dy=ref["dy"], y=ref["y"], dx=ref["dx"]), fusion["step"])
    X.check_f32(dict(dW=ref["dW"], db=ref["db"]))
    _REF[key] = ref
    return ref


INT_CASES = [(g, lin, 2) for g in GEOMS for lin in LINS]


@pytest.mark.parametrize("geom,lin,nseq", INT_CASES, ids=[f"{g}-L{l}" for g, l, _ in INT_CASES])
def test_integer_operands_are_exact(gpu, half, geom, lin, nseq):
    """small-integer operands: y, dx and dW equal the oracle bit for bit"""
    X.assert_lrelu_zero_convention(0.25)
    case = _case(geom, lin, nseq)
    for fusion in INT_FUSIONS:
        ref = _int_reference(case, fusion)
        ctx = f"[{geom} L{lin} {fusion['name']} {half}]"
        got, tags = _run(gpu, case, fusion, half, AUTO, ref)
        _grouped_tags(tags, fusion)
        X.assert_exact(got["y"], ref["y"], half, "y", context=ctx)
        X.assert_exact(got["dx"], ref["dx"], half, "dx", context=ctx)
        X.assert_exact(got["dW"], ref["dW"], torch.float32, "dW", nlc=False, context=ctx)
        X.assert_exact(got["db"], ref["db"], torch.float32, "db", nlc=False, context=ctx)


# ---- the launcher's grid rule (csrc/conv_grouped.hip: groups_per_block, blocks16, evt_grouped_bwd_weight) ----------------
def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _gb(groups):
    return 16 if groups % 16 == 0 else 8 if groups % 8 == 0 else 4


def _blocks_x(gpu, tiles, groups):
    """forward / backward-data: 16 waves per CU over all group sets, in blocks of gb waves"""
    gb = _gb(groups)
    return max(1, min(tiles, _cus(gpu) * 16 // (gb * (groups // gb))))


def _wgrad_split(gpu, tiles, groups):
    """weight gradient: two blocks per CU over the sets of 4 groups, at most one per CU for a single set"""
    sets = groups // 4
    return max(1, min(tiles, _cus(gpu), (2 * _cus(gpu) + sets - 1) // sets))


# (geometry, Lin, nseq): every block of all three kernels walks >= 3 tiles, full and partial ones alternating
MULTI_TILE = [("g256", 260, 25), ("g64", 260, 100)]


@pytest.mark.parametrize("geom,lin,nseq", MULTI_TILE, ids=[c[0] for c in MULTI_TILE])
def test_blocks_walk_several_tiles(gpu, half, geom, lin, nseq):
    """the prefetch pipeline: >= 3 tiles per block with partial ones among them (lout 65 = one full tile + one position),
    integer operands compared bit for bit, and random operands against the direct kernels"""
    case = _case(geom, lin, nseq)
    groups = case[6]
    tiles_f = nseq * -(-_lout(lin) // PT)
    tiles_d = nseq * -(-((lin - 1 + PAD) // 4 + 1) // PT)
    assert tiles_f // _blocks_x(gpu, tiles_f, groups) >= 3, "forward: fewer than 3 tiles per block on this chip"
    assert tiles_d // _blocks_x(gpu, tiles_d, groups) >= 3, "backward-data: fewer than 3 tiles per block on this chip"
    assert tiles_f // _wgrad_split(gpu, tiles_f, groups) >= 3, "weight gradient: fewer than 3 tiles per block on this chip"
    assert _lout(lin) % PT != 0
    fusion = INT_FUSIONS[2]
    ref = _int_reference(case, fusion)
    ctx = f"[{geom} L{lin} n{nseq} {fusion['name']} {half}]"
    got, tags = _run(gpu, case, fusion, half, AUTO, ref)
    _grouped_tags(tags, fusion)
    X.assert_exact(got["y"], ref["y"], half, "y", context=ctx)
    X.assert_exact(got["dx"], ref["dx"], half, "dx", context=ctx)
    X.assert_exact(got["dW"], ref["dW"], torch.float32, "dW", nlc=False, context=ctx)
    fusion = FUSIONS[2]
    ref = _reference(case, fusion, half)
    got, _ = _run(gpu, case, fusion, half, AUTO, ref)
    _compare(got, ref, TOL[half], ctx + " random operands vs oracle")


# ---- operands as the generator step passes them ----------------------------------------------------------------------------
def _slot_of(gpu, case, dtype, ops):
    from easevoice_trainer_amd.hip import conv as HC

    cin, cout, k, stride, pad, dil, groups = case[:7]
    m = HC.EvtConv1d(cin, cout, k, stride, pad, dil, groups, bias=True, transposed=False, weight_norm=False)
    with torch.no_grad():
        m.weight.copy_(ops["w"])
        m.bias.copy_(ops["bias"])
    m = m.to(gpu)
    bank = HC.WeightBank(m, dtype, gpu, impl=AUTO)
    bank.build_tables()
    bank.fold()
    return m, bank


@pytest.mark.parametrize("geom,lin", [("g4", 320), ("g16", 260), ("g64", 90), ("g256", 320)])
def test_half_batch_operands_and_add(gpu, half, geom, lin):
    """backward-data and the weight gradient over the SECOND half of a batch (y[h:], dy of the half: non-zero storage
    offsets) give the bits of the same call on copies; they agree with the oracle's second half; and the fused add operand
    equals backward-data followed by add_, bit for bit"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    h = 2
    case = _case(geom, lin, 2 * h)
    fusion = FUSIONS[2]
    ref = _reference(case, fusion, half)
    m, bank = _slot_of(gpu, case, half, ref)
    slot = m._slot
    nlc = lambda t: t.transpose(1, 2).contiguous().to(gpu, half)
    x, dy = nlc(ref["x"]), nlc(ref["dy"])
    args = (1.0, L.ACT_LRELU, fusion["out_slope"])
    rec = []
    HC.set_trace(rec)
    try:
        y = HC._fwd(slot, x, None, *args)
        dyh = dy[h:]                                   # contiguous view at a storage offset
        assert y[h:].storage_offset() > 0 and dyh.storage_offset() > 0
        dx_view = HC._bwd_data(slot, dyh, y[h:], None, None, h, lin, *args)
        dx_copy = HC._bwd_data(slot, dyh.clone(), y[h:].clone(), None, None, h, lin, *args)
        add = torch.randn(h, lin, case[0], device=gpu).to(half)
        dx_fused = HC._bwd_data(slot, dyh, y[h:], None, add, h, lin, *args)
        dw = []
        for xs, ds, ys in ((x[h:], dyh, y[h:]), (x[h:].clone(), dyh.clone(), y[h:].clone())):
            bank.zero_dw()
            if m.weight.grad is not None:
                m.weight.grad.zero_()
                m.bias.grad.zero_()
            HC._bwd_weight_now(slot, xs, ds, ys, h, lin, *args)
            bank.grads()
            dw.append(m.weight.grad.detach().clone())
        torch.cuda.synchronize()
    finally:
        HC.set_trace(None)
    tags = {(r[1], r[0]) for r in rec}
    assert {("fwd", "grouped_fwd"), ("bwd_data", "grouped_bwd_data"), ("bwd_weight", "grouped_bwd_weight")} <= tags, tags
    assert not any(t.startswith("conv_naive") for _, t in tags), tags
    assert torch.equal(dx_view, dx_copy)
    assert torch.equal(dx_fused, dx_copy.clone().add_(add)), "fused add differs from backward-data + add_"
    tol = TOL[half]
    assert _rel(_ncl(dx_view), ref["dx"][h:]) < tol
    # the oracle's dW of the second half alone
    xo, wo = ref["x"][h:].clone(), ref["w"].clone().requires_grad_(True)
    yo = O.conv_block(xo, wo, ref["bias"], None, stride=STRIDE, pad=PAD, dil=1, groups=case[6], out_act=1,
                      out_slope=fusion["out_slope"])
    (dwo,) = torch.autograd.grad(yo, wo, ref["dy"][h:])
    for d in dw:
        assert _rel(d, dwo) < tol
    assert _rel(dw[0], dw[1]) < 1e-5                   # (fp32 atomics: equal up to the order of the additions)


def test_add_operand_fp32_matches_two_steps(gpu):
    """the fp32 kernel's add epilogue: the same bits as backward-data followed by add_"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    case = _case("g16", 260, 2)
    ref = _reference(case, FUSIONS[0], torch.float32)
    m, bank = _slot_of(gpu, case, torch.float32, ref)
    dy = ref["dy"].transpose(1, 2).contiguous().to(gpu)
    add = torch.randn(2, 260, case[0], device=gpu)
    rec = []
    HC.set_trace(rec)
    try:
        plain = HC._bwd_data(m._slot, dy, None, None, None, 2, 260, 1.0, L.ACT_NONE, 1.0)
        fused = HC._bwd_data(m._slot, dy, None, None, add, 2, 260, 1.0, L.ACT_NONE, 1.0)
        torch.cuda.synchronize()
    finally:
        HC.set_trace(None)
    assert {r[0] for r in rec} == {"grouped_bwd_data"}, rec
    assert torch.equal(fused, plain.clone().add_(add))
    assert _rel(_ncl(plain), ref["dx"]) < TOL[torch.float32]
