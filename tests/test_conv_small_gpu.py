"""GPU tests of the degenerate convolutions of csrc/conv_small.hip: one output channel (C -> 1: the discriminators' and the
vocoder's conv_post) and one input channel (1 -> C: the discriminators' first layers), forward, backward-data and weight
gradient with the fused bias gradient.

Oracle parity goes through tests/test_conv_gpu.py::_run_case (y, dx, dres, dweight_v, dweight_g / dweight, dbias against
the CPU oracle, that file's tolerances) with its four fusions in fp32 and bf16.  The shapes are edges of the kernels'
geometry, which csrc/conv_small.hip names:
  C -> 1   G <= 64 lanes per output in the forward, a thread per 16-byte piece of dx in backward-data, both striding from
           capped grids; the weight gradient is x-stationary (cout1_bwd_weight_xs) at stride 1, dilation 1 with 3 or 7 taps
           and generic otherwise; sequences far shorter than a block's share put several sequence ends -- all of them
           padding -- into one block.
  1 -> C   C1_TP = 512 outputs per forward tile, C1_TQ = 256 outputs per weight-gradient tile, and 512 (k5 s3) or 256
           (k15) INPUTS per backward-data tile.
"""
import re

import pytest
import torch

import exact_inputs as X
import test_conv_gpu as TC

pytestmark = pytest.mark.gpu

# (cin, cout, k, stride, pad, dil, groups, transposed, wn, L, nseq)
_P = (1024, 1, 3, 1, 1, 1, 1, False, True)        # discriminator conv_post
_V = (16, 1, 7, 1, 3, 1, 1, False, False)         # vocoder conv_post: no bias, no weight norm
# The grids stride over their work: evt_cout1_fwd caps its grid at 4096 blocks (`cap`) of four outputs each (1024 channels:
# 64 lanes per output), evt_cout1_bwd_data at 2048 blocks of 256 16-byte pieces.  127 x 48 = 6096 positions fit one round of
# the forward; 127 x 130 = 16510 take two with a ragged second one, and five ragged trips of backward-data.
COUT1_CASES = [
    _P + (23, 11), _P + (37, 7), _P + (1, 5), _P + (2, 5),
    _P + (127, 130),
    _V + (3000, 3), _V + (5, 4),
    (64, 1, 3, 1, 1, 1, 1, False, True, 40, 3),
    # rows whose 16-byte piece count is no power of two (the weight gradient's `pc < ppr` guard, lane groups that do not
    # divide the pieces): 384 channels are 48 pieces in 16 bits and 96 in fp32; 24 channels with 7 taps are 3 and 6 pieces
    (384, 1, 3, 1, 1, 1, 1, False, True, 29, 5),
    (24, 1, 7, 1, 3, 1, 1, False, True, 70, 3),
    # other tap counts / strides: the generic kernels (cout1_bwd_weight, not the x-stationary form)
    (32, 1, 5, 1, 2, 1, 1, False, True, 90, 3),
    (64, 1, 3, 2, 1, 1, 1, False, True, 81, 3),
]

_A = (1, 32, 5, 3, 2, 1, 1, False, True)          # DiscriminatorP first layer: lout = (L - 1) // 3 + 1
_B = (1, 16, 15, 1, 7, 1, 1, False, True)         # DiscriminatorS first layer: lout = L


def _cin1_cases():
    cases = []
    # k5 s3: lout at T - 1, T, T + 1, 2T + 1 for T = 256 (weight gradient) and 512 (forward); L at the same marks of the
    # 512-input backward-data tile; L = 1; L = 3 (below the 5-tap receptive field)
    for lout in (255, 256, 257, 513, 511, 512, 1025):
        cases.append(_A + (3 * (lout - 1) + 1, 3))
    for L in (511, 512, 513, 1025, 1, 3):
        cases.append(_A + (L, 3))
    # k15 s1: T = 256 (weight gradient, backward-data) and 512 (forward); L = 1; L = 10 (below 15 taps)
    for L in (255, 256, 257, 513, 511, 512, 1025, 1, 10):
        cases.append(_B + (L, 3))
    # more than 16 taps (8 channels): two tap passes in backward-data and in the weight gradient
    cases.append((1, 8, 20, 2, 9, 1, 1, False, True, 601, 3))
    return cases


CIN1_CASES = _cin1_cases()

# determinism and the integer-exact runs: one case of either kind (several tiles, sequences that end inside a tile)
INT_CASES = [_P + (37, 19), _A + (1537, 3)]


def _id(case):
    return "x".join(str(int(v)) for v in case)


def _parity(gpu, case):
    for dtype in (torch.float32, torch.bfloat16):
        for fusion in TC.FUSIONS:
            TC._run_case(gpu, case, fusion, dtype, 0)


@pytest.mark.parametrize("case", COUT1_CASES, ids=_id)
def test_cout1_parity(gpu, case):
    _parity(gpu, case)


@pytest.mark.parametrize("case", CIN1_CASES, ids=_id)
def test_cin1_parity(gpu, case):
    _parity(gpu, case)


def _step(gpu, HC, case, dtype, fusion, seed=11):
    """forward and backward of one module from seeded inputs; returns the stored y, dx and the parameter gradients"""
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    torch.manual_seed(seed)
    m = HC.EvtConv1d(cin, cout, k, stride, pad, dil, groups, bias=True, transposed=transposed, weight_norm=wn).to(gpu)
    x = torch.randn(nseq, lin, cin).to(gpu, dtype).requires_grad_(True)
    dy = torch.randn(nseq, m.lout(lin), cout).to(gpu, dtype)
    bank = HC.WeightBank(m, dtype, gpu, impl=0)
    bank.build_tables()
    bank.fold()
    y = m(x, None, fusion["in_slope"], fusion["out_act"], fusion["out_slope"])
    y.backward(dy)
    bank.grads()
    torch.cuda.synchronize()
    out = dict(y=y.detach().clone(), dx=x.grad.clone())
    for n_, p in m.named_parameters():
        out["d" + n_] = p.grad.clone()
    return out


@pytest.mark.parametrize("case", INT_CASES, ids=_id)
def test_bit_identical_from_run_to_run(gpu, case):
    from easevoice_trainer_amd.hip import conv as HC

    fusion = TC.FUSIONS[2]
    a = _step(gpu, HC, case, torch.bfloat16, fusion)
    b = _step(gpu, HC, case, torch.bfloat16, fusion)
    assert {"y", "dx", "dbias"} <= set(a) and any(n.startswith("dweight") for n in a), sorted(a)
    for name in a:
        assert torch.equal(a[name], b[name]), f"{name} differs between two runs of {case}"


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", INT_CASES, ids=_id)
def test_integer_exact(gpu, case, dn):
    """bit for bit against the float64 reference on integer operands (tests/exact_inputs.py; the conditions that make this
    a fair demand are checked element by element in tests/test_conv_small_cpu.py).  These cases are not in the recorded tag
    table, so the launches are not traced."""
    import test_exact_int_gpu as TE
    from easevoice_trainer_amd.hip import lib as L

    try:
        for fusion in X.conv_fusions(case):
            inp = X.conv_inputs(case, fusion)
            ref = X.conv_reference(inp, case, fusion)
            TE.run_conv(gpu, case, fusion, dn, "auto", inp, ref, trace=False)
    finally:
        L.set_half(torch.bfloat16)


def test_biased_cout1_weight_gradient_is_one_kernel_and_one_fold(gpu):
    """the bias gradient of a C -> 1 layer comes out of the weight-gradient kernel and its fold: no column-sum launch, one
    fold launch for dW and dbias together"""
    from torch.profiler import ProfilerActivity, profile

    from easevoice_trainer_amd.hip import conv as HC

    case, fusion, dtype = _P + (37, 19), TC.FUSIONS[2], torch.bfloat16
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    torch.manual_seed(3)
    m = HC.EvtConv1d(cin, cout, k, stride, pad, dil, groups, bias=True, transposed=transposed, weight_norm=False).to(gpu)
    x = torch.randn(nseq, lin, cin).to(gpu, dtype).requires_grad_(True)
    dy = torch.randn(nseq, m.lout(lin), cout).to(gpu, dtype)
    bank = HC.WeightBank(m, dtype, gpu, impl=0)
    bank.build_tables()
    bank.fold()
    y = m(x, None, fusion["in_slope"], fusion["out_act"], fusion["out_slope"])
    torch.cuda.synchronize()
    rec = []
    HC.set_trace(rec)
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            y.backward(dy)
            bank.grads()         # (a bank may queue its weight-gradient launches until here)
            torch.cuda.synchronize()
    finally:
        HC.set_trace(None)
    wg = [r[0] for r in rec if r[1] == "bwd_weight"]
    assert wg == ["cout1_bwd_weight_xs<k3>"], rec
    dev = torch.autograd.DeviceType.CUDA
    kernels = [e.name for e in prof.events() if e.device_type == dev and not e.name.startswith(("Memcpy", "Memset"))]
    assert any("cout1_bwd_weight_xs" in n for n in kernels), kernels
    assert not [n for n in kernels if "colsum_act" in n], kernels
    assert len([n for n in kernels if re.search(r"fold_partials(?!_)", n)]) == 1, kernels
    # and the fused bias gradient is the sum of dy * act'(y)
    want = (dy.float() * torch.where(y.detach().float() > 0, 1.0, fusion["out_slope"])).sum()
    assert abs(float(m.bias.grad) - float(want)) <= 1e-3 * max(1.0, abs(float(want))), (float(m.bias.grad), float(want))
