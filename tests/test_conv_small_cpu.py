"""CPU side of the integer-exact cases of tests/test_conv_small_gpu.py (no GPU needed): the conditions under which the
kernels of csrc/conv_small.hip must equal the float64 reference bit for bit, checked on the reference alone for EVERY
element, as tests/test_exact_inputs_cpu.py does for its own cases.  Every stored value (x, dy, res, y, dx, dres) is an
integer multiple of the fusion's step of at most 256 steps -- the bfloat16 significand -- and of at most 2048 steps for
IEEE half (which the first implies; both are asserted, by the limits of tests/exact_inputs.py); |dW| and |db| stay below
2^24, where fp32 sums of integers are exact in any order."""
import pytest
import torch

import exact_inputs as X
import test_conv_small_gpu as TS


@pytest.mark.parametrize("case", TS.INT_CASES, ids=TS._id)
def test_conv_small_exact_conditions(case):
    for fusion in X.conv_fusions(case):
        inp = X.conv_inputs(case, fusion)
        assert bool((inp["w"] != 0).all()) and float(inp["w"].abs().max()) == 2.0
        assert bool((inp["x"] != 0).any()) and bool((inp["dy"] != 0).any())
        ref = X.conv_reference(inp, case, fusion)
        stored = dict(y=ref["y"], dx=ref["dx"], dres=ref["dres"], x=inp["x"], dy=inp["dy"], res=inp["res"])
        for dtype in (torch.bfloat16, torch.float16):
            X.check_stored(stored, fusion["step"], X.LIMIT_STEPS[dtype])
        X.check_f32({k: ref[k] for k in ("dW", "db", "dW2", "db2")})
        # the folded weight-normed image is v itself
        g = X.weight_g_of(inp["w"])
        ss = (inp["w"].float() ** 2).reshape(g.size(0), -1).sum(1).reshape(g.shape)
        assert torch.equal(g / torch.sqrt(ss), torch.ones_like(g))
