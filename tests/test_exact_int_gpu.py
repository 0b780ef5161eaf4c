"""GPU: the convolution, residual-unit and dense-GEMM kernels against float64 references, BIT FOR BIT.

Operands, references, the comparator and the reasoning why equality is owed are in tests/exact_inputs.py; the conditions
on the references are checked without a GPU by tests/test_exact_inputs_cpu.py.  Every comparison here is torch.equal on the
stored type; every run also asserts which kernels it reached: by family where the dispatcher's intent is known (as
tests/test_conv_gpu.py does), and launch kind by launch kind against tests/golden/exact_int_tags.json, the record the static
guard reads.  `python tests/test_exact_int_gpu.py --record` (on the GPU) rewrites that record after a deliberate dispatch
change.

Rounding points the kernels take on purpose, and how the operands stay representable there:
  * hip/conv.py::ConvFn.backward stores dy * act'(y) in 16 bits (evt_dact_mul) for wide layers: dy is a small integer and
    act' a power of two;
  * hip/conv.py::ConvFn.forward stores lrelu(x) in 16 bits for the upsamplers (PLAIN_X): |x| <= 2 and the slope is 0.5;
  * csrc/elementwise.hip:67,106,166 fold a weight-normed row as v * (g / sqrtf(ss)): with g = sqrt(ss) that scale is 1 to
    within 2 ulp of fp32 (measured on the first run of this file: whole output channels off by 2^-23 relative), which a
    16-bit image rounds back to v and an fp32 image keeps.  The fp32 runs therefore take the weight_norm=False module of the
    same geometry (the same kernels: the fold is the only difference); the fp32 weight-norm fold stays with
    tests/test_conv_gpu.py at 1e-3;
  * hip/resunit.py::ResUnitFn / resunit_bwd store xa, the mid activation and dmid in 16 bits: all three are among the tensors
    the CPU file bounds (for the dense +-1 pass dmid only where exact_inputs.resunit_dense_judges_first says so).
"""
import json
import os
import sys
import types

import pytest
import torch

import exact_inputs as X

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TAGS_PATH = os.path.join(HERE, "golden", "exact_int_tags.json")
DT = dict(bf16=torch.bfloat16, f16=torch.float16, f32=torch.float32)
IMPL = dict(auto=0, naive=1)
RECORD = os.environ.get("EXACT_INT_RECORD")          # a path: write the observed tags there instead of asserting them
_observed = {}


def _expect_tags(key, tags):
    """`tags`: set of (kind, kernel tag) of one run; compared by (kind, head) with the committed record"""
    got = sorted({f"{k}:{X.tag_head(t)}" for k, t in tags})
    if RECORD:
        _observed[key] = got
        with open(RECORD, "w") as f:
            json.dump(_observed, f, indent=0, sort_keys=True)
        return
    with open(TAGS_PATH) as f:
        table = json.load(f)
    assert key in table, f"no recorded kernels for {key}: run `python tests/test_exact_int_gpu.py --record` on the GPU"
    assert got == table[key], f"{key}: launched {got}, recorded {table[key]}"


def _traced(HC, fn):
    """run fn() with the launch trace on; returns (result, records)"""
    rec = []
    HC.set_trace(rec)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        HC.set_trace(None)
    return out, rec


def _zero_grads(mods, bank):
    for p in mods.parameters():
        if p.grad is not None:
            p.grad.zero_()           # in place: the bank's tables hold these addresses
    bank.zero_dw()


def _nlc(t, gpu, dtype):
    return t.transpose(1, 2).contiguous().to(gpu, dtype)


# ---- convolutions -----------------------------------------------------------------------------------------------------------
def _conv_module(HC, case, inp, wn):
    cin, cout, k, stride, pad, dil, groups, transposed = case[:8]
    m = HC.EvtConv1d(cin, cout, k, stride, pad, dil, groups, bias=inp["bias"] is not None, transposed=transposed,
                     weight_norm=wn)
    with torch.no_grad():
        if wn:
            m.weight_v.copy_(inp["w"])
            m.weight_g.copy_(X.weight_g_of(inp["w"]))
        else:
            m.weight.copy_(inp["w"])
        if inp["bias"] is not None:
            m.bias.copy_(inp["bias"])
    return m


def _conv_pass(gpu, bank, mods, m, inp, fusion, dtype, dy):
    _zero_grads(mods, bank)
    xg = _nlc(inp["x"], gpu, dtype).requires_grad_(True)
    rg = _nlc(inp["res"], gpu, dtype).requires_grad_(True) if inp["res"] is not None else None
    y = m(xg, rg, fusion["in_slope"], fusion["out_act"], fusion["out_slope"])
    y.backward(_nlc(dy, gpu, dtype))
    bank.grads()
    torch.cuda.synchronize()
    return y.detach(), xg.grad, (rg.grad if rg is not None else None)


def run_conv(gpu, case, fusion, dn, impl, inp, ref, trace=True, weight_grads=True):
    """one convolution, forward and two backward passes, everything compared exactly; returns {(kind, tag)}.
    A weight-normed module cannot show its raw dW (dv and dg are projections of it: the tolerance tests' business), so dW is
    read through a weight_norm=False twin of the same geometry in the same bank, which must reach the same kernel."""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    dtype = DT[dn]
    L.set_half(dtype)
    wn = case[8] and dn != "f32"          # (the fp32 fold of a weight-normed layer: see the module docstring)
    mods = torch.nn.ModuleList([_conv_module(HC, case, inp, wn)] + ([_conv_module(HC, case, inp, False)] if wn else []))
    mods = mods.to(gpu)
    m, twin = mods[0], mods[-1]
    bank = HC.WeightBank(mods, dtype, gpu, impl=IMPL[impl])
    bank.build_tables()
    bank.fold()
    ctx = f"[case={case} fusion={fusion['name']} dtype={dn} impl={impl}]"

    def body():
        y, dx, dres = _conv_pass(gpu, bank, mods, m, inp, fusion, dtype, inp["dy"])
        X.assert_exact(y, ref["y"], dtype, "y", context=ctx)
        X.assert_exact(dx, ref["dx"], dtype, "dx", context=ctx)
        if dres is not None:
            X.assert_exact(dres, ref["dres"], dtype, "dres", context=ctx)
        if not weight_grads:
            return
        if m.bias is not None:
            X.assert_exact(m.bias.grad, ref["db"], torch.float32, "db", nlc=False, context=ctx)
        if not wn:
            X.assert_exact(m.weight.grad, ref["dW"], torch.float32, "dW", nlc=False, context=ctx)
        # the second pass: dense +-1 dy, dW and db alone
        _conv_pass(gpu, bank, mods, twin, inp, fusion, dtype, inp["dy2"])
        X.assert_exact(twin.weight.grad, ref["dW2"], torch.float32, "dW (dense dy)", nlc=False, context=ctx)
        if twin.bias is not None:
            X.assert_exact(twin.bias.grad, ref["db2"], torch.float32, "db (dense dy)", nlc=False, context=ctx)

    if not trace:
        body()
        return set()
    _, rec = _traced(HC, body)
    of = lambda mod: {(r[1], r[0]) for r in rec if r[7] is mod}
    if wn and weight_grads:
        a, b = ({t for k_, t in of(mod) if k_ == "bwd_weight"} for mod in (m, twin))
        assert a == b, f"the weight_norm=False twin reached {b}, the module {a} {ctx}"
    return of(m) | of(twin)


DEEP = ("conv_deep", "conv_deep32")


def _family_check(name, case, fusion, tags, ctx):
    """the kernels each list exists for, as tests/test_conv_gpu.py asserts them (16-bit types, impl auto)"""
    heads = {(k, X.tag_head(t)) for k, t in tags}
    fwd = {h for k, h in heads if k == "fwd"}
    bwd = {h for k, h in heads if k == "bwd_data"}
    wg = {h for k, h in heads if k == "bwd_weight"}
    plain_in = fusion["in_slope"] == 1.0
    cin, cout = case[0], case[1]
    if name in ("deep", "edge_deep", "edge_p7") and plain_in:
        assert fwd & set(DEEP), (fwd, ctx)
        if cin % 128 == 0:
            assert bwd & set(DEEP), (bwd, ctx)
        if cout % 128 == 0 and cin % 64 == 0 and name not in X.LIGHT:
            assert wg & {"wgrad_deep", "wgrad_halo"}, (wg, ctx)
    if name in ("ring", "edge_ring") and plain_in:
        assert "conv_ring" in fwd, (fwd, ctx)
        if cin % 64 == 0 and cout % 64 == 0:
            assert "conv_ring" in bwd, (bwd, ctx)
        assert wg & {"wgrad_ring", "wgrad_halo"}, (wg, ctx)
    if name in ("narrow", "edge_narrow"):
        if plain_in:
            assert "conv_narrow" in fwd, (fwd, ctx)
        assert "conv_narrow" in bwd, (bwd, ctx)
    if name == "ups":
        assert fwd & {"conv_ring", "conv_deep", "conv_deep32"}, (fwd, ctx)
        assert (("elt", "lrelu_kernel") in heads) == (not plain_in), (heads, ctx)      # activated once: hip/conv.py::PLAIN_X
    if (name == "halo" and case[1] in (32, 64) or name == "edge_halo") and plain_in:
        assert "wgrad_halo" in wg, (wg, ctx)
    if name == "edge_rows16" and plain_in and fusion["out_act"] == 0:
        assert "rows16_gemm" in fwd, (fwd, ctx)
    if name == "edge_igemm":
        assert "conv_igemm" in fwd, (fwd, ctx)


@pytest.mark.parametrize("name,ci", X.conv_case_ids(), ids=[f"{n}-{i}" for n, i in X.conv_case_ids()])
def test_conv_exact(gpu, name, ci):
    case = X.conv_case_lists()[name][ci]
    seen = {run: set() for run in X.conv_runs(name)}
    for fusion in X.conv_fusions(case):
        inp = X.conv_inputs(case, fusion)
        ref = X.conv_reference(inp, case, fusion, weight_grads=name not in X.LIGHT)
        for dn, impl in X.conv_runs(name):
            tags = run_conv(gpu, case, fusion, dn, impl, inp, ref, weight_grads=name not in X.LIGHT)
            if dn != "f32" and impl == "auto":
                _family_check(name, case, fusion, tags, f"[{name}-{ci} {fusion['name']} {dn}]")
            seen[(dn, impl)] |= tags
    for (dn, impl), tags in seen.items():
        _expect_tags(f"conv/{name}/{ci}/{dn}/{impl}", tags)


def _slab_cases():
    import test_conv_gpu as TC

    marks = [m for m in TC.test_wgrad_deep_ring_slabs_are_deterministic.pytestmark if m.name == "parametrize"]
    return [TC.HALO_CASES[i] for i in (0, 2, 5, 7, 10)] + [tuple(c) for c in marks[0].args[1]]


@pytest.mark.parametrize("case", _slab_cases(), ids=lambda c: "x".join(map(str, c)))
def test_wgrad_exact_under_every_reduction(gpu, case):
    """the deterministic slabs (EVT_WGRAD_PARTS=1, the default) and the fp32 atomics (=0), each with the weight-gradient
    launches deferred to the side stream (EVT_WGRAD_DEFER, default 48) and in stream order (=0): all four equal the
    reference -- not each other to 1e-4.  The bank reads both switches when it is built (tests/test_conv_gpu.py::
    _wgrad_twice handles them the same way); no trace here, a traced run never defers."""
    from easevoice_trainer_amd.hip import conv as HC

    fusion = X.FUSIONS[0]
    inp = X.conv_inputs(case, fusion)
    ref = X.conv_reference(inp, case, fusion)
    for parts in ("1", "0"):
        for defer in (None, "0"):
            env = {"EVT_WGRAD_PARTS": parts, "EVT_WGRAD_DEFER": defer}
            old = {k: os.environ.get(k) for k in env}
            for k, v in env.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            try:
                made = []
                orig = HC.WeightBank.__init__

                def spy(self, *a, **kw):
                    orig(self, *a, **kw)
                    made.append(self)

                HC.WeightBank.__init__ = spy
                try:
                    run_conv(gpu, case, fusion, "bf16", "auto", inp, ref, trace=False)
                finally:
                    HC.WeightBank.__init__ = orig
                assert made[0].parts_on == (parts == "1") and (made[0].defer_n > 0) == (defer is None), env
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ---- residual units ---------------------------------------------------------------------------------------------------------
def _unit_modules(HC, C, k, d, inp, wn):
    from easevoice_trainer_amd.module.models import get_padding

    c1 = HC.EvtConv1d(C, C, k, dilation=d, padding=get_padding(k, d), weight_norm=wn)
    c2 = HC.EvtConv1d(C, C, k, dilation=1, padding=get_padding(k, 1), weight_norm=wn)
    with torch.no_grad():
        for c, w, b in ((c1, inp["w1"], inp["b1"]), (c2, inp["w2"], inp["b2"])):
            if wn:
                c.weight_v.copy_(w)
                c.weight_g.copy_(X.weight_g_of(w))
            else:
                c.weight.copy_(w)
            c.bias.copy_(b)
    return c1, c2


def _unit_pass(gpu, HC, bank, mods, c1, c2, inp, dtype, dy):
    _zero_grads(mods, bank)
    xg = _nlc(inp["x"], gpu, dtype).requires_grad_(True)
    y = HC.res_unit(xg, c1, c2, 0.5)
    xa, mid_a = y.grad_fn.saved_tensors
    y.backward(_nlc(dy, gpu, dtype))
    bank.grads()
    torch.cuda.synchronize()
    return y.detach(), xa, mid_a, xg.grad


@pytest.mark.parametrize("case", X.RESUNIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resunit_exact(gpu, case):
    """res_unit forward (xa, the mid activation, y) and backward (dx, dW, db of both convolutions): csrc/resunit.hip +
    resunit_bwd.hip for C = 16 / 32, resunit_wide.hip both ways for C = 64 / 128, the three- and four-launch composition
    for C = 256.  slope = 0.5.  bfloat16 where exact_inputs.resunit_dtypes allows it, IEEE half everywhere."""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    C, k, d, Lq = case
    inp = X.resunit_inputs(C, k, d, Lq, X.RESUNIT_NSEQ)
    ref = X.resunit_reference(inp, k, d, 0.5)
    for dn in X.resunit_dtypes(C, k, d):
        dtype = DT[dn]
        L.set_half(dtype)
        mods = torch.nn.ModuleList(_unit_modules(HC, C, k, d, inp, True) + _unit_modules(HC, C, k, d, inp, False)).to(gpu)
        bank = HC.WeightBank(mods, dtype, gpu)
        bank.build_tables()
        bank.fold()
        ctx = f"[unit {case} {dn}]"
        x0 = _nlc(inp["x"], gpu, dtype)
        fused = Lq >= 64                  # shorter sequences: the composition of single launches, exact all the same
        if C <= 32 and fused:
            assert HC._resunit_params(mods[0]._slot, mods[1]._slot, x0, 0.5) is not None, "the fused path must cover this case"
        elif C <= 128 and fused:
            assert HC._resunit_wide_params(mods[0]._slot, mods[1]._slot, x0, 0.5) is not None, "the wide path must cover it"

        def body():
            y, xa, mid_a, dx = _unit_pass(gpu, HC, bank, mods, mods[0], mods[1], inp, dtype, inp["dy"])
            for got, n in ((xa, "xa"), (mid_a, "mid_a"), (y, "y"), (dx, "dx")):
                X.assert_exact(got, ref[n], dtype, n, context=ctx)
            X.assert_exact(mods[0].bias.grad, ref["db1"], torch.float32, "db1", nlc=False, context=ctx)
            X.assert_exact(mods[1].bias.grad, ref["db2"], torch.float32, "db2", nlc=False, context=ctx)
            y, xa, mid_a, dx = _unit_pass(gpu, HC, bank, mods, mods[2], mods[3], inp, dtype, inp["dy"])
            X.assert_exact(y, ref["y"], dtype, "y (twin)", context=ctx)
            X.assert_exact(dx, ref["dx"], dtype, "dx (twin)", context=ctx)
            for mod, n in ((mods[2], "1"), (mods[3], "2")):
                X.assert_exact(mod.weight.grad, ref["dW" + n], torch.float32, "dW" + n, nlc=False, context=ctx)
                X.assert_exact(mod.bias.grad, ref["db" + n], torch.float32, "db" + n + " (twin)", nlc=False, context=ctx)
            _unit_pass(gpu, HC, bank, mods, mods[2], mods[3], inp, dtype, inp["dy2"])
            judged = [(mods[3], "2")] + ([(mods[2], "1")] if X.resunit_dense_judges_first(C, k, dn) else [])
            for mod, n in judged:
                X.assert_exact(mod.weight.grad, ref["dW" + n + "2"], torch.float32, f"dW{n} (dense dy)", nlc=False, context=ctx)
                X.assert_exact(mod.bias.grad, ref["db" + n + "2"], torch.float32, f"db{n} (dense dy)", nlc=False, context=ctx)

        _, rec = _traced(HC, body)
        wn_tags = {(r[1], r[0]) for r in rec if r[7] is mods[0] or r[7] is mods[1]}
        tw_tags = {(r[1], r[0]) for r in rec if r[7] is mods[2] or r[7] is mods[3]}
        assert wn_tags == tw_tags, f"twin {tw_tags} against {wn_tags} {ctx}"
        heads = {(k_, X.tag_head(t)) for k_, t in wn_tags}
        if C <= 32 and fused:
            assert ("fwd", "resunit_fwd") in heads and ("bwd_unit", "resunit_bwd_multi") in heads, heads
        elif C <= 128 and fused:
            assert ("fwd", "resunit_wide_fwd") in heads and ("bwd_unit", "resunit_wide_bwd") in heads, heads
        _expect_tags(f"resunit/{C}x{k}x{d}x{Lq}/{dn}", wn_tags)


@pytest.mark.parametrize("scale", [0.5, 0.25])
@pytest.mark.parametrize("case", X.STAGE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stage_exact(gpu, case, scale):
    """res_stage: three one-unit blocks (k = 3 / 7 / 11, d = 1 / 3 / 5) on one input through the grouped launches
    (resunit_fwd_multi, resunit_bwd_multi), summed with a power-of-two scale that the backward folds into its load of dy"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    C, Lq = case
    units = X.stage_inputs(C, Lq, X.RESUNIT_NSEQ)
    ref = X.stage_reference(units, X.STAGE_KS, X.STAGE_DS, 0.5, scale)
    for dn in X.stage_dtypes(C):
        dtype = DT[dn]
        L.set_half(dtype)
        ctx = f"[stage {case} scale {scale} {dn}]"
        for wn in (True, False):
            pairs = [_unit_modules(HC, C, k, d, u, wn) for u, k, d in zip(units, X.STAGE_KS, X.STAGE_DS)]
            mods = torch.nn.ModuleList([c for p in pairs for c in p]).to(gpu)
            blocks = [types.SimpleNamespace(convs1=[mods[2 * i]], convs2=[mods[2 * i + 1]]) for i in range(3)]
            bank = HC.WeightBank(mods, dtype, gpu)
            bank.build_tables()
            bank.fold()

            def one(dy):
                _zero_grads(mods, bank)
                xg = _nlc(units[0]["x"], gpu, dtype).requires_grad_(True)
                y = HC.res_stage(xg, blocks, 0.5, scale)
                assert y is not None, "the grouped path must cover this stage"
                y.backward(_nlc(dy, gpu, dtype))
                bank.grads()
                torch.cuda.synchronize()
                return y.detach(), xg.grad

            def body():
                y, dx = one(units[0]["dy"])
                X.assert_exact(y, ref["y"], dtype, "y", context=ctx)
                X.assert_exact(dx, ref["dx"], dtype, "dx", context=ctx)
                for i, r in enumerate(ref["units"]):
                    for j, n in ((0, "1"), (1, "2")):
                        mod = mods[2 * i + j]
                        X.assert_exact(mod.bias.grad, r["db" + n], torch.float32, f"unit {i} db{n}", nlc=False, context=ctx)
                        if not wn:
                            X.assert_exact(mod.weight.grad, r["dW" + n], torch.float32, f"unit {i} dW{n}", nlc=False,
                                           context=ctx)
                if not wn:
                    one(units[0]["dy2"])
                    for i, (r, k) in enumerate(zip(ref["units"], X.STAGE_KS)):
                        X.assert_exact(mods[2 * i + 1].weight.grad, r["dW22"], torch.float32, f"unit {i} dW2 (dense dy)",
                                       nlc=False, context=ctx)
                        X.assert_exact(mods[2 * i + 1].bias.grad, r["db22"], torch.float32, f"unit {i} db2 (dense dy)",
                                       nlc=False, context=ctx)

            _, rec = _traced(HC, body)
            tags = {(r[1], r[0]) for r in rec}
            heads = {(k_, X.tag_head(t)) for k_, t in tags}
            assert ("fwd", "resunit_fwd_multi") in heads and ("bwd_unit", "resunit_bwd_multi") in heads, heads
            _expect_tags(f"stage/{C}x{Lq}/{scale}/{dn}/{'wn' if wn else 'plain'}", tags)


# ---- dense GEMMs ------------------------------------------------------------------------------------------------------------
def _last_tag():
    from easevoice_trainer_amd.hip import lib as L

    return L.lib().evt_last_kernel_tag().decode()


def _linear_bank(gpu, inp, N, K, dtype):
    from easevoice_trainer_amd.hip.linear import LinearBank

    Np = (N + 127) // 128 * 128 if N % 8 else N
    store = torch.zeros(Np, K, device=gpu)                     # the padded rows the image reads must exist and be zero
    w = torch.nn.Parameter(store[:N])
    w.data.copy_(inp["w"])
    b = torch.nn.Parameter(inp["bias"].float().to(gpu)) if inp["bias"] is not None else None
    bank = LinearBank([("t", w, b)], dtype, gpu)
    bank.prepare()
    return w, b, Np


def _gemm_cases():
    import test_gemm_gpu as TG

    return TG.CASES


@pytest.mark.parametrize("case", _gemm_cases(), ids=lambda c: "x".join(map(str, c[:3])))
def test_linear_exact(gpu, case):
    """hip/linear.py::linear forward, backward-data and backward-weight at the shapes of tests/test_gemm_gpu.py::CASES; the
    padded 1025 -> 1152 vocabulary columns are exact zeros and their weight-gradient rows never surface"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.linear import gemm_bwd_data, gemm_bwd_weight, linear

    M, N, K, has_bias, relu = case
    inp = X.gemm_inputs(M, N, K, has_bias)
    ref = X.gemm_reference(inp, relu)
    for dn in ("f32", "bf16", "f16"):
        _linear_exact(gpu, case, dn, inp, ref, HC, L, gemm_bwd_data, gemm_bwd_weight, linear)


def _linear_exact(gpu, case, dn, inp, ref, HC, L, gemm_bwd_data, gemm_bwd_weight, linear):
    M, N, K, has_bias, relu = case
    dtype = DT[dn]
    L.set_half(dtype)
    w, b, Np = _linear_bank(gpu, inp, N, K, dtype)
    ctx = f"[linear {case} {dn}]"
    tags = set()
    HC.set_trace([])          # switches the library's kernel tags on
    try:
        for sfx, dy in (("", inp["dy"]), ("2", inp["dy2"])):
            w.grad = None
            if b is not None:
                b.grad = None
            xg = inp["x"].unsqueeze(0).to(gpu, dtype).requires_grad_(True)          # a 3-D input, like [B, L, K]
            y = linear(xg, w, b, relu=relu)
            tags.add(("fwd", _last_tag()))
            assert y.shape == (1, M, Np)
            if Np != N:
                assert not y[..., N:].any(), "padding columns are exact zeros"
            X.assert_exact(y[0, :, :N], ref["y"], dtype, "y", nlc=False, context=ctx)
            y[..., :N].backward(dy.unsqueeze(0).to(gpu, dtype))
            torch.cuda.synchronize()
            if sfx == "":
                X.assert_exact(xg.grad[0], ref["dx"], dtype, "dx", nlc=False, context=ctx)
            X.assert_exact(w.grad, ref["dW" + sfx], torch.float32, "dW" + sfx, nlc=False, context=ctx)
            if b is not None:
                X.assert_exact(b.grad, ref["db" + sfx], torch.float32, "db" + sfx, nlc=False, context=ctx)
        # the same backward launches from this thread, for their tags (autograd's thread keeps its own)
        slot = w._evt_slot
        dyp = torch.zeros(M, Np, device=gpu, dtype=dtype)
        dyp[:, :N] = (inp["dy"] * (ref["y"] > 0) if relu else inp["dy"]).to(gpu, dtype)
        dx = gemm_bwd_data(slot, dyp)
        tags.add(("bwd_data", _last_tag()))
        X.assert_exact(dx, ref["dx"], dtype, "dx (direct)", nlc=False, context=ctx)
        dw, db = gemm_bwd_weight(slot, inp["x"].to(gpu, dtype), dyp)
        tags.add(("bwd_weight", _last_tag()))
        X.assert_exact(dw, ref["dW"], torch.float32, "dW (direct)", nlc=False, context=ctx)
    finally:
        HC.set_trace(None)
    _expect_tags(f"linear/{M}x{N}x{K}/{dn}", tags)


@pytest.mark.parametrize("shape", X.gemm256_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_gemm256_exact(gpu, shape):
    """the 256 x 256 kernels (csrc/gemm256.hip) with every fused epilogue -- relu, relu + dropout (p = 0.5: keep-scale 2, the
    keep mask is the one evt_relu_dropout_fwd draws for the same seed and site), add, and gate + add on backward-data
    (gate_pos = 2) -- and the weight gradient of the same shapes (wgrad_gemm)"""
    import ctypes as C
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import enc as E, lib as L
    from easevoice_trainer_amd.hip.linear import gemm_bwd_data, gemm_bwd_weight, gemm_fwd

    M, N, K = shape
    inp = X.gemm_inputs(M, N, K, True)
    ref = X.gemm_reference(inp, True)
    epi = X.gemm_epilogue_operands(M, N, K)
    want = dict(dx=inp["dy"].float() @ inp["w"].float(), dW=inp["dy2"].t().float() @ inp["x"].float(), db=inp["dy2"].sum(0))
    for dn in ("bf16", "f16"):
        _gemm256_exact(gpu, shape, dn, inp, ref, epi, want, C, HC, E, L, gemm_bwd_data, gemm_bwd_weight, gemm_fwd)


def _gemm256_exact(gpu, shape, dn, inp, ref, epi, want, C, HC, E, L, gemm_bwd_data, gemm_bwd_weight, gemm_fwd):
    M, N, K = shape
    dtype = DT[dn]
    L.set_half(dtype)
    w, b, _ = _linear_bank(gpu, inp, N, K, dtype)
    slot = w._evt_slot
    assert slot.fused(M, False)
    ctx = f"[gemm256 {shape} {dn}]"
    dev = lambda t: t.to(gpu, dtype)
    x = dev(inp["x"])
    z, relu_z = ref["z"], ref["y"]
    tags = set()
    HC.set_trace([])
    try:
        # no gate / add operand: the pipelined kernel, or gemm256_nt for one long-K tile per block (gemm256.hip: pipe_shape);
        # which of the two is in the record
        G256 = ("gemm256_pipe<", "gemm256_nt<")
        X.assert_exact(gemm_fwd(slot, x, relu=True), relu_z, dtype, "relu", nlc=False, context=ctx)
        assert _last_tag().startswith(G256), _last_tag()
        tags.add(("fwd", _last_tag()))
        X.assert_exact(gemm_fwd(slot, x), z, dtype, "bias only", nlc=False, context=ctx)
        assert _last_tag().startswith(G256), _last_tag()
        # relu + dropout: equal to the standalone kernel on the exact relu(z), every element either dropped or doubled
        E.seed_rng(gpu, 123)
        p, site = 0.5, 9
        y = gemm_fwd(slot, x, relu=True, drop=(p, site))
        assert _last_tag().startswith(G256), _last_tag()
        tags.add(("fwd_dropout", _last_tag()))
        zz = dev(relu_z)
        yk = torch.empty_like(zz)
        L.check(L.lib().evt_relu_dropout_fwd(L.dt_code(dtype), L.ptr(zz), C.c_float(p), L.ptr(E.rng_counter(gpu)),
                                             C.c_uint32(site), None, 0, 0, L.ptr(yk), C.c_int64(zz.numel()), L.stream_ptr()),
                "evt_relu_dropout_fwd")
        assert torch.equal(y, yk), f"fused relu + dropout differs from evt_relu_dropout_fwd {ctx}"
        kept = yk != 0
        assert torch.equal(yk, torch.where(kept, 2 * zz, torch.zeros_like(zz))), f"a kept element is not 2 relu(z) {ctx}"
        live = zz > 0
        frac = (kept & live).float().sum() / live.float().sum()
        assert abs(frac.item() - (1 - p)) < 0.01, frac
        # forward add
        X.assert_exact(gemm_fwd(slot, x, add=dev(epi["add_n"])), z + epi["add_n"], dtype, "add", nlc=False, context=ctx)
        assert _last_tag().startswith("gemm256_nt<"), _last_tag()
        tags.add(("fwd_add", _last_tag()))
        # backward-data: plain, then gate (the derivative of relu + dropout off the saved activation) and add
        dy = dev(inp["dy"])
        dxr = want["dx"].double()
        X.assert_exact(gemm_bwd_data(slot, dy), dxr, dtype, "dx", nlc=False, context=ctx)
        tags.add(("bwd_data", _last_tag()))
        got = gemm_bwd_data(slot, dy, gate=dev(epi["gate"]), gate_pos=2.0, add=dev(epi["add_k"]))
        if slot.fused(M, True):
            assert _last_tag().startswith("gemm256_nt<"), _last_tag()
        tags.add(("bwd_data_gate", _last_tag()))
        X.assert_exact(got, dxr * (epi["gate"] > 0) * 2.0 + epi["add_k"], dtype, "dx gate + add", nlc=False, context=ctx)
        # weight gradient: dense +-1 dy
        dw, db = gemm_bwd_weight(slot, x, dev(inp["dy2"]))
        tags.add(("bwd_weight", _last_tag()))
        X.assert_exact(dw, want["dW"], torch.float32, "dW", nlc=False, context=ctx)
        X.assert_exact(db, want["db"], torch.float32, "db", nlc=False, context=ctx)
    finally:
        HC.set_trace(None)
    _expect_tags(f"gemm256/{M}x{N}x{K}/{dn}", tags)


@pytest.mark.parametrize("wdn", ["f32", "bf16"])
@pytest.mark.parametrize("B", X.DEC_ROWS)
def test_dec_linear_exact(gpu, B, wdn):
    """evt_dec_gemv (B <= 4) and evt_dec_gemm_rows (B <= 32) without the LayerNorm prologue: fp32 activations, weights in
    fp32 or bf16, fp32 outputs -- integer operands make every sum exact below 2^24, so y equals the reference in any order;
    N = 1025 (the logits: no bias, not a multiple of 16) and two layer shapes with a bias, with and without relu"""
    import ctypes as C
    from easevoice_trainer_amd.hip import lib as L

    for N, K in X.DEC_SHAPES:
        g = X.gen("dec", B, N, K, wdn)
        W, a = X.dense_pm((N, K), g), X.small_int((B, K), g, 3)
        bias = None if N == 1025 else X.small_int((N,), g, 3)
        Wg, ag = W.to(gpu, DT[wdn]), a.float().to(gpu)
        bg = bias.float().to(gpu) if bias is not None else None
        for relu in (0, 1):
            want = a @ W.t() + (bias if bias is not None else 0.0)
            want = want.clamp(min=0) if relu else want
            assert float(want.abs().max()) < X.F32_EXACT
            for fn in (["evt_dec_gemv"] if B <= 4 else []) + ["evt_dec_gemm_rows"]:
                y = torch.full((B, N), float("nan"), device=gpu)
                L.check(getattr(L.lib(), fn)(L.dt_of(Wg), L.ptr(Wg), L.ptr(bg), L.ptr(ag), None, None, None, C.c_float(1e-5),
                                             None, L.ptr(y), B, N, K, relu, L.stream_ptr()), fn)
                torch.cuda.synchronize()
                X.assert_exact(y, want, torch.float32, fn, nlc=False, context=f"[B={B} N={N} K={K} {wdn} relu={relu}]")


if __name__ == "__main__":
    if "--record" in sys.argv:
        os.environ["EXACT_INT_RECORD"] = TAGS_PATH
        sys.exit(pytest.main([os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider"]))
