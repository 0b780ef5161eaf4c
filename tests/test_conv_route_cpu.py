"""Dispatch of the Conv1d family without a GPU: evt_conv1d_route (the host arithmetic evt_conv1d_fwd / _bwd_data /
_bwd_weight run before they launch) against tests/golden/exact_int_tags.json, the record of which kernel every pass of
every run of tests/test_exact_int_gpu.py::test_conv_exact launched on the GPU.  A change that moves a shape to another
kernel fails here, before the tree travels to a GPU."""
import ctypes as C
import json
import os

import pytest

import exact_inputs as X
from easevoice_trainer_amd.hip import conv as HC
from easevoice_trainer_amd.hip import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "exact_int_tags.json")) as f:
    TAGS = {k: v for k, v in json.load(f).items() if k.startswith("conv/")}      # resunit/, stage/, linear/, gemm256/: other dispatchers

# family -> the tag heads its launchers set (csrc/conv1d.hip, conv_deep.hip, conv_narrow.hip, conv_small.hip, ...)
HEADS = {
    "fwd": dict(ROWS16={"rows16_gemm"}, GROUPED={"grouped_fwd"}, COUT1={"cout1_fwd"}, CIN1={"cin1_fwd"},
                NAIVE={"conv_naive_fwd"}, DEEP={"conv_deep", "conv_deep32", "conv_ring"}, NARROW={"conv_narrow"},
                IGEMM={"conv_igemm"}),
    "bwd_data": dict(ROWS16={"rows16_gemm"}, GROUPED={"grouped_bwd_data"}, COUT1={"cout1_bwd_data"}, CIN1={"cin1_bwd_data"},
                     NAIVE={"conv_naive_bwd_data"}, DEEP={"conv_deep", "conv_deep32", "conv_ring"}, NARROW={"conv_narrow"},
                     IGEMM={"conv_igemm"}),
    "bwd_weight": dict(GROUPED={"grouped_bwd_weight"}, COUT1={"cout1_bwd_weight", "cout1_bwd_weight_xs"},
                       CIN1={"cin1_bwd_weight"}, NAIVE={"conv_naive_bwd_weight"}, GEMM={"wgrad_gemm"}, HALO={"wgrad_halo"},
                       DEEP={"wgrad_deep"}, RING={"wgrad_ring"}, TILE={"conv_wgrad_tr", "conv_wgrad"}),
}
PASSES = dict(fwd=L.PASS_FWD, bwd_data=L.PASS_BWD_DATA, bwd_weight=L.PASS_BWD_WEIGHT)


def route(p, kind, fused=0):
    r = L.ConvRoute()
    assert L.lib().evt_conv1d_route(C.byref(p), PASSES[kind], fused, C.byref(r)) == 0, (kind, fused)
    return (L.WG_FAMILIES if kind == "bwd_weight" else L.CONV_FAMILIES)[r.family]


def conv_fn_routes(case, fusion, dn, impl):
    """the library calls of one hip/conv.py::ConvFn forward + backward (tests/test_exact_int_gpu.py::_conv_pass: x needs a
    gradient, the bank wants weight gradients, no dx_add), as routes: ({kind: family}, activated input?, plain dy?)"""
    lib = L.lib()
    in_slope, out_act, out_slope = fusion["in_slope"], fusion["out_act"], fusion["out_slope"]
    params = lambda s, a, o: X.conv_params(case, dn, impl, s, a, o)
    has_res = fusion["res"] and not case[7]                                    # exact_inputs.conv_inputs
    # ConvFn.forward
    pre = bool(in_slope != 1.0 and HC.PLAIN_X and lib.evt_conv1d_wants_plain_x(C.byref(params(in_slope, out_act, out_slope))))
    fam = dict(fwd=route(params(1.0 if pre else in_slope, out_act, out_slope), "fwd", L.FUSED_RES if has_res else 0))
    # ConvFn.backward
    plain_dy = bool(out_act != L.ACT_NONE and lib.evt_conv1d_wants_plain_dy(C.byref(params(in_slope, out_act, out_slope))))
    if plain_dy:
        out_act, out_slope = L.ACT_NONE, 1.0
    fam["bwd_weight"] = route(params(1.0 if pre else in_slope, out_act, out_slope), "bwd_weight")
    fam["bwd_data"] = route(params(in_slope, out_act, out_slope), "bwd_data")
    return fam, pre, plain_dy


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
def test_routes_match_the_recorded_launches(dn):
    """every conv/ key of the record, none skipped: for each pass the recorded heads are exactly covered by the families the
    routes of the key's three fusions name, and the two element-wise pre-passes are recorded exactly when the predicates ask
    for them"""
    assert HC.PLAIN_X, "EVT_CONV_PLAIN_X=0 is a measurement switch: the record was taken with the default"
    L.set_half(X.DT[dn])
    try:
        lists = X.conv_case_lists()
        keys = [k for k in TAGS if k.split("/")[3] == dn]
        assert len(TAGS) == 488 and keys
        for key in keys:
            _, name, ci, _, impl = key.split("/")
            case = lists[name][int(ci)]
            assert (dn, impl) in X.conv_runs(name), key
            recorded = {kind: {t.split(":")[1] for t in TAGS[key] if t.startswith(kind + ":")}
                        for kind in ("fwd", "bwd_data", "bwd_weight", "elt")}
            allowed = {kind: set() for kind in PASSES}
            lrelu = dact = False
            for fusion in X.conv_fusions(case):
                fam, pre, plain_dy = conv_fn_routes(case, fusion, dn, impl)
                lrelu, dact = lrelu or pre, dact or plain_dy
                for kind, f in fam.items():
                    heads = HEADS[kind][f]
                    assert heads & recorded[kind], f"{key} {fusion['name']}: {kind} routes to {f}, recorded {recorded[kind]}"
                    allowed[kind] |= heads
            for kind in PASSES:
                assert recorded[kind] <= allowed[kind], f"{key}: {kind} recorded {recorded[kind]}, the routes allow {allowed[kind]}"
            assert ("lrelu_kernel" in recorded["elt"]) == lrelu, key
            assert ("dact_mul_kernel" in recorded["elt"]) == dact, key
            assert recorded["elt"] <= {"lrelu_kernel", "dact_mul_kernel"}, key
    finally:
        L.set_half(X.DT["bf16"])


def test_every_recorded_run_is_routed():
    """the three dtype passes above cover the record: every conv/ key belongs to one of them"""
    assert {k.split("/")[3] for k in TAGS} == {"bf16", "f16", "f32"}
    assert sorted(TAGS) == sorted(f"conv/{n}/{i}/{d}/{m}" for n, i in X.conv_case_ids() for d, m in X.conv_runs(n))


def test_family_names_follow_the_header():
    """hip/lib.py names the families, passes, images and fused bits by value: the values are include/evt.h's #defines"""
    import re

    with open(os.path.join(HERE, "..", "include", "evt.h")) as f:
        defs = {n: int(v) for n, v in re.findall(r"^#define (EVT_[A-Z0-9_]+) (\d+)\b", f.read(), flags=re.M)}
    assert {f"EVT_CONV_{n}": i for i, n in enumerate(L.CONV_FAMILIES)} == {k: v for k, v in defs.items() if k.startswith("EVT_CONV_")}
    assert {f"EVT_WG_{n}": i for i, n in enumerate(L.WG_FAMILIES)} == {k: v for k, v in defs.items() if k.startswith("EVT_WG_")}
    for name in ("PASS_FWD", "PASS_BWD_DATA", "PASS_BWD_WEIGHT", "FUSED_RES", "FUSED_ADD", "IMG_REG", "IMG_ALT"):
        assert getattr(L, name) == defs["EVT_" + name], name


def test_route_query_refusals():
    """evt_conv1d_route validates like the entry points and launches nothing"""
    lib = L.lib()
    r = L.ConvRoute()
    good = L.ConvParams(L.DT_F32, 2, 64, 32, 32, 3, 1, 1, 1, 1, 0, 1.0, 0, 1.0, L.IMPL_AUTO)
    assert lib.evt_conv1d_route(C.byref(good), L.PASS_FWD, 0, C.byref(r)) == 0 and L.CONV_FAMILIES[r.family] == "IGEMM"
    assert lib.evt_conv1d_route(C.byref(good), 3, 0, C.byref(r)) == L.EVT_EINVAL
    assert lib.evt_conv1d_route(C.byref(good), L.PASS_FWD, 0, None) == L.EVT_EINVAL
    odd = L.ConvParams(L.DT_F32, 2, 64, 30, 32, 3, 1, 1, 1, 1, 0, 1.0, 0, 1.0, L.IMPL_IGEMM)
    for kind in PASSES.values():      # EVT_IMPL_IGEMM on a shape the MFMA kernels do not take
        assert lib.evt_conv1d_route(C.byref(odd), kind, 0, C.byref(r)) == L.EVT_ENOTSUP
    bad = L.ConvParams(L.DT_F32, 2, 64, 30, 32, 3, 1, 1, 1, 4, 0, 1.0, 0, 1.0, L.IMPL_AUTO)       # cin % groups != 0
    assert lib.evt_conv1d_route(C.byref(bad), L.PASS_FWD, 0, C.byref(r)) == L.EVT_EINVAL
