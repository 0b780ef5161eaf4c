"""hip/enc.py::gemm_rows_route: which layers of the feature extractors run on evt_gemm_rows_f32; and the argument errors of its
binding hip/feat.py::gemm_rows_f32, which are raised before anything touches a device."""
import itertools

import pytest
import torch

from easevoice_trainer_amd.hip import lib as L
from easevoice_trainer_amd.hip.enc import gemm_rows_route
from easevoice_trainer_amd.hip.feat import (GEMM_ROWS_ACT_GELU, GEMM_ROWS_ACT_NONE, GEMM_ROWS_TILE_K, GEMM_ROWS_TILE_M,
                                            GEMM_ROWS_TILE_N, conv_rows_weight, gemm_rows_f32)


def test_only_fp32_whole_tiles_aligned_rows_without_autograd_take_the_route():
    for dtype, N, K, lda, grad in itertools.product((torch.float32, torch.bfloat16, torch.float16), (16, 768, 24, 0),
                                                    (16, 1536, 3072, 8, 40), (1024, 16, 4, 6, 0), (False, True)):
        want = dtype == torch.float32 and N > 0 and N % 16 == 0 and K % 16 == 0 and lda > 0 and lda % 4 == 0 and not grad
        assert gemm_rows_route(dtype, N, K, lda, grad) is want, (dtype, N, K, lda, grad)
    assert (GEMM_ROWS_TILE_M, GEMM_ROWS_TILE_N, GEMM_ROWS_TILE_K) == (128, 128, 32)          # include/evt.h


def test_conv_rows_weight_is_tap_major():
    w = torch.arange(2 * 3 * 2, dtype=torch.float32).view(2, 3, 2)                           # [cout, cin, k]
    assert conv_rows_weight(w).tolist() == [[0, 2, 4, 1, 3, 5], [6, 8, 10, 7, 9, 11]]


@pytest.mark.parametrize("bad,why", [
    (dict(x=torch.zeros(2, 5, 32)[:, :, 1:17]), "contiguous float32 items"),                 # a strided view
    (dict(x=torch.zeros(2, 5, 16, dtype=torch.bfloat16)), "contiguous float32 items"),
    (dict(x=torch.zeros(2 * 5 * 16 + 1)[1:].view(2, 5, 16)), "16-byte aligned"),             # 4 bytes off
    (dict(w=torch.zeros(32, 16, dtype=torch.float64)), "float32 matrix"),
    (dict(x=torch.zeros(2, 5, 24), w=torch.zeros(32, 24)), "not served"),                    # K % 16
    (dict(w=torch.zeros(24, 16)), "not served"),                                             # N % 16
    (dict(lda=6), "not served"),
    (dict(rows=6), "do not fit"),
    (dict(bias=torch.zeros(16)), "bias must be"),
    (dict(act=2), "act 2"),
    (dict(lens=torch.zeros(2, dtype=torch.int64)), "lens must be"),
    (dict(out=torch.zeros(2, 5, 16)), "out must be"),
    (dict(x=torch.zeros(2, 5, 16, requires_grad=True)), "inference only"),
    (dict(w=torch.zeros(32, 16, requires_grad=True)), "inference only"),
    (dict(), "must be on the GPU"),                                                          # all else in order: no CPU path
])
def test_binding_refuses(bad, why):
    args = dict(x=torch.zeros(2, 5, 16), lens=torch.tensor([5, 2], dtype=torch.int32), w=torch.zeros(32, 16),
                bias=torch.zeros(32), act=GEMM_ROWS_ACT_GELU)
    args.update(bad)
    with pytest.raises(L.EvtError, match=why):
        gemm_rows_f32(**args)
    with torch.no_grad(), pytest.raises(L.EvtError, match="must be on the GPU" if "inference" in why else why):
        gemm_rows_f32(**dict(args, act=GEMM_ROWS_ACT_NONE if "act" not in bad else bad["act"]))
