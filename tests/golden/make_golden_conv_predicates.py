"""Recorder of tests/golden/conv_predicates.json: what evt_conv1d_wants_plain_x, evt_conv1d_wants_plain_dy and
evt_conv1d_layout answer over a grid, taken from the library of the tree this file is run in (host arithmetic: no GPU).

    python tests/golden/make_golden_conv_predicates.py [--parent OLD.json]

The grid: every distinct convolution of the s2 models of configs/s2.json (generator, enc_q, flow, the text encoder and both
discriminator kinds; the shapes come from the modules' own slots, ConvSlot.params) and EXTRA, each at nseq x lin x out_act x
in_slope x dtype.  hip/conv.py and hip/disc.py act on these predicates, so a refactor of the dispatcher must leave them
alone: tests/test_conv_predicates_cpu.py compares the library of its tree with this record.  --parent names a record
taken from an earlier commit: rows whose answer differs from it are listed under "parent" with the earlier answer (the
test admits them only at EXTRA and only where the new answer is what evt_conv1d_route says).  Data only."""
import ctypes as C
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NSEQ, LIN = (1, 4, 32), (5, 64, 400, 3200)
ACTS = ((0, 1.0), (1, 0.1), (2, 1.0))          # (out_act, out_slope): none, lrelu, tanh
SLOPES = (1.0, 0.1)                            # in_slope
DTYPES = ("f32", "bf16", "f16")
# (cin, cout, k, stride, pad, dil, groups, transposed): stride-1 layers of the narrow kernel's widths at dilations beyond the
# models' (1, 3, 5), where the register bound of conv_narrow.hip::narrow_eligible depends on the dilation
EXTRA = [(32, 32, 7, 1, 33, 11, 1, 0), (32, 32, 7, 1, 36, 12, 1, 0), (16, 16, 11, 1, 90, 18, 1, 0)]


def s2_convs():
    """the distinct geometries of the s2 models, in module order, read from slots as hip/bank.py makes them"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.module import models

    hps = json.load(open(os.path.join(ROOT, "configs", "s2.json")))
    nets = [models.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"]), models.MultiPeriodDiscriminator(False)]
    bank = types.SimpleNamespace(dt=L.DT_F32, impl=L.IMPL_AUTO)
    seen = []
    for net in nets:
        for m in net.modules():
            if isinstance(m, HC.EvtConv1d):
                lay = HC.conv_layout(L.DT_F32, m.cin, m.cout, m.k, m.stride, m.pad, m.dil, m.groups, m.transposed)
                p = HC.ConvSlot(m, lay, bank).params(1, 64, 1.0, 0, 1.0)
                geo = (p.cin, p.cout, p.k, p.stride, p.pad, p.dil, p.groups, p.transposed)
                if geo not in seen:
                    seen.append(geo)
    return seen


def answers(convs):
    """{dtype: {"layout": [13 numbers per conv], "plain": one character per grid row, '0' + wants_plain_x + 2 wants_plain_dy}};
    rows in the order conv, nseq, lin, (out_act, out_slope), in_slope"""
    import torch
    from easevoice_trainer_amd.hip import lib as L

    out = {}
    for dn in DTYPES:
        dtype = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[dn]
        L.set_half(dtype)
        lib, dt = L.lib(), L.dt_code(dtype)
        layouts, plain = [], []
        for geo in convs:
            lay = L.WLayout()
            assert lib.evt_conv1d_layout(C.byref(L.ConvParams(dt, 1, 64, *geo, 1.0, 0, 1.0, 0)), C.byref(lay)) == 0
            layouts.append([getattr(lay, f) for f, _ in L.WLayout._fields_])
            for nseq in NSEQ:
                for lin in LIN:
                    for act, oslope in ACTS:
                        for slope in SLOPES:
                            p = L.ConvParams(dt, nseq, lin, *geo, slope, act, oslope, 0)
                            plain.append(str(lib.evt_conv1d_wants_plain_x(C.byref(p))
                                             + 2 * lib.evt_conv1d_wants_plain_dy(C.byref(p))))
        out[dn] = dict(layout=layouts, plain="".join(plain))
    L.set_half(torch.bfloat16)
    return out


def rows(convs):
    """the grid row of every character of "plain", as [conv, nseq, lin, out_act, out_slope, in_slope]"""
    return [[i, nseq, lin, act, oslope, slope] for i in range(len(convs)) for nseq in NSEQ for lin in LIN
            for act, oslope in ACTS for slope in SLOPES]


def main():
    sys.path.insert(0, ROOT)
    convs = s2_convs() + [g for g in EXTRA]
    rec = dict(convs=[list(g) for g in convs], answers=answers(convs), parent=[])
    if "--parent" in sys.argv:
        old = json.load(open(sys.argv[sys.argv.index("--parent") + 1]))
        assert old["convs"] == rec["convs"], "the earlier record was taken over another grid"
        grid = rows(convs)
        for dn in DTYPES:
            assert old["answers"][dn]["layout"] == rec["answers"][dn]["layout"], "evt_conv1d_layout differs"
            for row, a, b in zip(grid, old["answers"][dn]["plain"], rec["answers"][dn]["plain"]):
                if a != b:
                    rec["parent"].append(dict(dtype=dn, row=row, plain=b, parent=a))
    path = os.path.join(HERE, "conv_predicates.json")
    with open(path, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print(len(convs), "convolutions,", len(rec["answers"]["bf16"]["plain"]), "rows per dtype,", len(rec["parent"]),
          "rows differ from the earlier record,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
