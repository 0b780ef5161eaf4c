"""hip/enc.py::attn_rows_route: which self-attention calls that ask for it run their core on evt_mha_rows_f32."""
import itertools

import torch

from easevoice_trainer_amd.hip.enc import attn_rows_route


def test_only_fp32_windowless_dropout_free_served_widths_without_autograd_take_the_route():
    for dtype, window, p, D, grad in itertools.product((torch.float32, torch.bfloat16, torch.float16), (None, 0, 4),
                                                       (0.0, 0.1), (32, 48, 64, 96, 128), (False, True)):
        want = dtype == torch.float32 and window is None and p == 0.0 and D in (32, 64) and not grad
        assert attn_rows_route(dtype, window, p, D, grad) is want, (dtype, window, p, D, grad)
