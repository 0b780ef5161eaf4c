"""CPU side of the integer-exact tests (tests/exact_inputs.py, tests/test_exact_int_gpu.py): no GPU needed.

1. The conditions under which a kernel must equal the float64 reference bit for bit, checked on the reference alone, for
   EVERY element of EVERY case the GPU file runs: each stored output / intermediate (y, dx, dres, the residual unit's xa,
   mid activation and dmid) is an integer multiple of the case's step (1, 0.5, 0.25) of at most 256 steps -- the bfloat16
   significand, which the 2048 of IEEE half contains --, and |dW|, |db| stay below 2^24.  Nothing is masked: a case that
   violated this would get a lower density in exact_inputs.py.
2. The comparator's sensitivity: four single faults injected into the reference (a tap dropped at the last position of one
   sequence, one input channel dropped, one sequence shifted by one position, one split of the dW sum counted twice) must
   each fail it, on a deep, a ring, a narrow and a GEMM case.
3. The static guard: every evt_set_last_tag("...") head of the conv / resunit / GEMM sources is expected by at least one
   exact case (tests/golden/exact_int_tags.json, which the GPU file asserts launch by launch) or is excluded here, by name,
   with a reason.
"""
import json
import os
import re

import pytest
import torch

import exact_inputs as X

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BF16 = torch.bfloat16
DTYPES = dict(bf16=torch.bfloat16, f16=torch.float16)


@pytest.mark.parametrize("name,ci", X.conv_case_ids(), ids=[f"{n}-{i}" for n, i in X.conv_case_ids()])
def test_conv_conditions(name, ci):
    case = X.conv_case_lists()[name][ci]
    for fusion in X.conv_fusions(case):
        inp = X.conv_inputs(case, fusion)
        assert bool((inp["w"] != 0).all()) and float(inp["w"].abs().max()) == 2.0
        assert bool((inp["x"] != 0).any()) and bool((inp["dy"] != 0).any())
        ref = X.conv_reference(inp, case, fusion, weight_grads=name not in X.LIGHT)
        X.check_stored(dict(y=ref["y"], dx=ref["dx"], dres=ref["dres"], x=inp["x"], dy=inp["dy"], res=inp["res"]),
                       fusion["step"])
        X.check_f32({k: ref[k] for k in ("dW", "db", "dW2", "db2")})
        # the folded weight-normed image is v itself
        g = X.weight_g_of(inp["w"])
        ss = (inp["w"].float() ** 2).reshape(g.size(0), -1).sum(1).reshape(g.shape)
        assert torch.equal(g / torch.sqrt(ss), torch.ones_like(g))


@pytest.mark.parametrize("case", X.RESUNIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resunit_conditions(case):
    C, k, d, L = case
    inp = X.resunit_inputs(C, k, d, L, X.RESUNIT_NSEQ)
    ref = X.resunit_reference(inp, k, d, 0.5)
    for name in X.resunit_dtypes(C, k, d):
        limit = X.LIMIT_STEPS[DTYPES[name]]
        X.check_stored({n: ref[n] for n in ("xa", "mid_a", "y", "dx", "dmid")}, 0.25, limit)
        if X.resunit_dense_judges_first(C, k, name):
            X.check_stored(dict(dmid2=ref["dmid2"]), 0.25, limit)
    X.check_f32({n: ref[n] for n in ("dW1", "dW2", "db1", "db2", "dW12", "dW22", "db12", "db22")})
    # an impulse at the first and at the last position of a sequence: the boundary taps are exercised
    for t in (inp["x"], inp["dy"]):
        assert bool((t[:, :, 0] != 0).any()) and bool((t[:, :, -1] != 0).any())


@pytest.mark.parametrize("case", X.STAGE_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("scale", [0.5, 0.25])
def test_stage_conditions(case, scale):
    C, L = case
    units = X.stage_inputs(C, L, X.RESUNIT_NSEQ)
    ref = X.stage_reference(units, X.STAGE_KS, X.STAGE_DS, 0.5, scale)
    step = 0.25 * scale
    for name in X.stage_dtypes(C):
        limit = X.LIMIT_STEPS[DTYPES[name]]
        X.check_stored(dict(y=ref["y"], dx=ref["dx"]), step, limit)
        for r in ref["units"]:
            X.check_stored({n: r[n] for n in ("xa", "mid_a", "y")}, 0.25, limit)
            X.check_stored({n: r[n] for n in ("dx", "dmid")}, step, limit)
            X.check_f32({n: r[n] for n in ("dW1", "dW2", "db1", "db2")})


def _gemm_shapes():
    import test_gemm_gpu as TG

    shapes = [(M, N, K, b, relu) for (M, N, K, b, relu) in TG.CASES]
    shapes += [(M, N, K, True, True) for (M, N, K) in X.gemm256_shapes()]
    return shapes


@pytest.mark.parametrize("shape", _gemm_shapes(), ids=lambda s: "x".join(map(str, s[:3])))
def test_gemm_conditions(shape):
    M, N, K, has_bias, relu = shape
    inp = X.gemm_inputs(M, N, K, has_bias)
    assert bool((inp["w"] != 0).all())
    ref = X.gemm_reference(inp, relu)
    extra = X.gemm_epilogue_operands(M, N, K)
    X.check_stored(dict(y=ref["y"], z=ref["z"], dx=ref["dx"], y_add=ref["z"] + extra["add_n"], y_drop=2 * ref["y"],
                        dx_epi=2 * ref["dx"] + extra["add_k"]), 1.0)
    X.check_f32({k: ref[k] for k in ("dW", "db", "dW2", "db2")})


# ---- the comparator sees single faults --------------------------------------------------------------------------------------
def _sensitivity_cases():
    import test_conv_gpu as TC

    return dict(deep=TC.DEEP_CASES[2], ring=TC.RING_CASES[2], narrow=TC.NARROW_CASES[2], gemm=X.gemm_as_conv(96, 512, 512))


def _fails(got, want, name):
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got.to(BF16), want, BF16, name, nlc=want.dim() == 3 and name != "dW")
    return str(e.value)


@pytest.mark.parametrize("family", ["deep", "ring", "narrow", "gemm"])
def test_comparator_fails_on_single_faults(family):
    import torch.nn.functional as F

    case = _sensitivity_cases()[family]
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    fusion = X.FUSIONS[0]
    inp = X.conv_inputs(case, fusion)
    ref = X.conv_reference(inp, case, fusion)
    y = ref["y"]
    X.assert_exact(y.transpose(1, 2).to(BF16), y, BF16, "y")                  # the unperturbed reference passes
    lout = y.size(2)

    # 1. one tap dropped at the last position of one sequence
    last = lout - 1
    found = None
    for s in range(nseq):
        for t in range(k):
            p = last * stride - pad + t * dil
            if 0 <= p < lin and bool((inp["x"][s, :, p] != 0).any()):
                found = (s, t, p)
                break
        if found:
            break
    assert found, "no non-zero product at the last position of any sequence: the case cannot see a lost boundary tap"
    s, t, p = found
    bad = y.clone()
    bad[s, :, last] -= inp["w"][:, :, t] @ inp["x"][s, :, p]
    msg = _fails(bad.transpose(1, 2), y, "y")
    assert f"seq {s}, pos {last}" in msg and f"pos%64={last % 64}" in msg, msg

    # 2. one input channel dropped
    c0 = int(torch.nonzero(inp["x"].abs().sum((0, 2)))[0])
    bad = y - F.conv1d(inp["x"][:, c0:c0 + 1], inp["w"][:, c0:c0 + 1], None, stride=stride, padding=pad, dilation=dil)
    _fails(bad.transpose(1, 2), y, "y")

    # 3. one sequence shifted by one position
    bad = y.clone()
    bad[nseq - 1] = torch.roll(y[nseq - 1], 1, dims=1)
    msg = _fails(bad.transpose(1, 2), y, "y")
    assert f"seq {nseq - 1}" in msg, msg

    # 4. one split of the dW sum counted twice (the positions of the first 64-position K stage of sequence 0)
    part = torch.zeros_like(inp["dy2"])
    part[0, :, :64] = inp["dy2"][0, :, :64]
    w = inp["w"].clone().requires_grad_(True)
    c = dict(inp, w=w)
    (extra,) = torch.autograd.grad(X.conv_forward(c, case, fusion), w, part)
    assert bool((extra != 0).any())
    with pytest.raises(AssertionError) as e:
        X.assert_exact((ref["dW2"] + extra).float(), ref["dW2"], torch.float32, "dW", nlc=False)
    assert "differ" in str(e.value)


def test_comparator_reports_dtype_shape_and_nan():
    a = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    X.assert_exact(a.transpose(1, 2).to(BF16), a, BF16, "a")
    with pytest.raises(AssertionError):
        X.assert_exact(a.transpose(1, 2).float(), a, BF16, "a")              # stored in another type
    with pytest.raises(AssertionError):
        X.assert_exact(a.to(BF16), a, BF16, "a")                             # not channels-last
    b = a.transpose(1, 2).to(BF16).clone()
    b[1, 2, 0] = float("nan")
    with pytest.raises(AssertionError) as e:
        X.assert_exact(b, a, BF16, "a")
    assert "1 of 24" in str(e.value) and "seq 1, pos 2, ch 0" in str(e.value)


# ---- static guard --------------------------------------------------------------------------------------------------------
GUARDED_SOURCES = ["conv1d.hip", "conv_deep.hip", "conv_small.hip", "conv_narrow.hip", "wgrad_halo.hip", "rows_gemm.hip",
                   "gemm256.hip", "resunit.hip", "resunit_wide.hip", "resunit_bwd.hip"]
# sources whose kernels are NOT multiply-accumulate alone, so that integer operands do not make them exact
EXCLUDED_SOURCES = {
    "wn_layer.hip": "tanh * sigmoid gate between its two GEMMs: transcendental, rests on the tolerance tests",
    "mha.hip": "softmax (exp, a division by the row sum): transcendental, rests on the tolerance tests",
    "frontend.hip": "layout transposes, codebook norms / argmin and the mel filterbank: no convolution or GEMM kernel",
}
# heads of the guarded sources that no exact case can expect
EXCLUDED_HEADS = {}      # (none at present)


def source_tag_heads(fname):
    src = open(os.path.join(ROOT, "easevoice_trainer_amd", "csrc", fname)).read()
    heads = set()
    for fmt in re.findall(r'evt_set_last_tag\(\s*"([^"]*)"', src):
        head = X.tag_head(fmt)
        if "%s" in head:        # resunit_wide_%s: "fwd" / "bwd"
            heads.update(head.replace("%s", v) for v in ("fwd", "bwd"))
        else:
            heads.add(head)
    return heads


def expected_heads():
    with open(os.path.join(HERE, "golden", "exact_int_tags.json")) as f:
        table = json.load(f)
    return {kh.split(":", 1)[1] for tags in table.values() for kh in tags}


def test_every_tagged_kernel_has_an_exact_case():
    want = set()
    for f in GUARDED_SOURCES:
        heads = source_tag_heads(f)
        assert heads, f"{f}: no evt_set_last_tag found (the guard's pattern no longer matches the source)"
        want |= heads
    have = expected_heads()
    missing = sorted(h for h in want - have if h not in EXCLUDED_HEADS)
    assert not missing, (f"kernels without an integer-exact case: {missing} -- add a case to tests/exact_inputs.py that reaches "
                         "each (and record its tags), or exclude it in EXCLUDED_HEADS with a reason")
    stale = sorted(h for h in EXCLUDED_HEADS if h in have)
    assert not stale, f"excluded although an exact case expects them: {stale}"


def test_every_source_with_tags_is_guarded_or_excluded():
    csrc = os.path.join(ROOT, "easevoice_trainer_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip") or f == "elementwise.hip":          # elementwise.hip defines evt_set_last_tag itself
            continue
        if 'evt_set_last_tag("' in open(os.path.join(csrc, f)).read():
            assert f in GUARDED_SOURCES or f in EXCLUDED_SOURCES, f"{f} tags kernels: guard it or exclude it with a reason"
