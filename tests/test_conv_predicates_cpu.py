"""evt_conv1d_wants_plain_x / evt_conv1d_wants_plain_dy / evt_conv1d_layout against tests/golden/conv_predicates.json, the
answers of the commit before the predicates were rebuilt on the dispatcher's routes (tests/golden/
make_golden_conv_predicates.py has the grid: every convolution of the s2 models and three dilations beyond theirs).
hip/conv.py and hip/disc.py act on the predicates: an answer that moves quietly moves a layer to another kernel."""
import ctypes as C
import importlib.util
import json
import os

import torch

from easevoice_trainer_amd.hip import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_conv_predicates",
                                               os.path.join(HERE, "golden", "make_golden_conv_predicates.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
with open(os.path.join(HERE, "golden", "conv_predicates.json")) as f:
    REC = json.load(f)
CONVS = [tuple(g) for g in REC["convs"]]


def test_the_grid_is_the_s2_models():
    """the recorded convolutions are the ones the models of configs/s2.json hold today, then EXTRA"""
    assert CONVS == G.s2_convs() + G.EXTRA
    assert len(CONVS) > 60 and all(len(REC["answers"][dn]["plain"]) == len(G.rows(CONVS)) for dn in G.DTYPES)


def test_predicates_and_layouts_answer_as_recorded():
    assert G.answers(CONVS) == REC["answers"]


def test_rows_that_left_the_parents_answer():
    """The parent's wants_plain_dy asked narrow_eligible with a descriptor whose dilation was still 0, so it promised the
    narrow kernel where the dispatcher's own descriptor fails the kernel's register bound (conv_narrow.hip:170-171: C = 32
    k = 7 from dil 11, C = 16 k = 11 from dil 18) and the caller paid evt_dact_mul for the generic kernel.  Those rows, at
    EXTRA alone, carry the new answer beside the parent's; the new answer is what evt_conv1d_route says of the backward
    calls with plain operands."""
    first_extra = len(CONVS) - len(G.EXTRA)
    assert REC["parent"], "the three EXTRA layers are where the parent's predicate and its dispatcher disagreed"
    for e in REC["parent"]:
        ci, nseq, lin, act, oslope, slope = e["row"]
        assert ci >= first_extra and act != 0 and slope == 1.0 and nseq * lin >= 4096, e
        assert (e["parent"], e["plain"]) == ("2", "0"), e                       # wants_plain_dy 1 -> 0, wants_plain_x untouched
        L.set_half(dict(bf16=torch.bfloat16, f16=torch.float16)[e["dtype"]])
        try:
            p = L.ConvParams(L.dt_code(L.half()), nseq, lin, *CONVS[ci], 1.0, 0, 1.0, 0)      # dy * act' as a plain operand
            r = L.ConvRoute()
            assert L.lib().evt_conv1d_route(C.byref(p), L.PASS_BWD_DATA, 0, C.byref(r)) == 0
            assert L.CONV_FAMILIES[r.family] == "IGEMM", e                      # neither DEEP nor NARROW ...
            assert L.lib().evt_conv1d_route(C.byref(p), L.PASS_BWD_WEIGHT, 0, C.byref(r)) == 0
            assert L.WG_FAMILIES[r.family] not in ("DEEP", "HALO"), e           # ... and no weight gradient that wants it
        finally:
            L.set_half(torch.bfloat16)
