"""evt_gemm_rows_f32 (csrc/gemm_rows.hip): the fp32 MFMA GEMM of the feature extractors on rows that may overlap, bias and GELU
fused, against float64 F.linear / F.conv1d of each item alone.  Row counts sit around the large tile; everything behind an
item's live run in x is NaN (or 1e30) and y is NaN before the launch."""
import pytest
import torch
import torch.nn.functional as F

from easevoice_trainer_amd.hip.feat import GEMM_ROWS_ACT_GELU as GELU
from easevoice_trainer_amd.hip.feat import GEMM_ROWS_ACT_NONE as NONE
from easevoice_trainer_amd.hip.feat import GEMM_ROWS_TILE_M as TM

pytestmark = pytest.mark.gpu
LENS = (1, TM - 1, TM, TM + 1, 2 * TM + 5, 0)
NAN, CIN = float("nan"), 16
# (N, K, lda): the smallest; a dense layer with a column tail and a K tail; cin 16 k 3 stride 2 (rows overlap); cin 16 k 2 stride 2
SHAPES = pytest.mark.parametrize("N,K,lda,fill", [(16, 16, 16, NAN), (144, 80, 80, 1e30), (48, 48, 32, NAN), (32, 32, 32, 1e30)])
_DATA = {}


def _live(n, K, lda):
    return (n - 1) * lda + K if n else 0


def _data(N, K, lda, exact):
    """seeded items (the live floats of each of LENS), w [N, K], bias and the float64 result of each item alone, built once.
    exact: ternary x and w, small-integer bias -- every partial sum is an integer far below 2^24"""
    key = (N, K, lda, exact)
    if key not in _DATA:
        g = torch.Generator().manual_seed(N + K + lda + exact)
        rnd = (lambda *s: torch.randint(-1, 2, s, generator=g).float()) if exact else (lambda *s: torch.randn(*s, generator=g))
        items = [rnd(_live(n, K, lda)) for n in LENS]
        w, bias = rnd(N, K), torch.randint(-3, 4, (N,), generator=g).float() if exact else torch.randn(N, generator=g)
        refs = []
        for n, it in zip(LENS, items):
            if lda == K or n == 0:
                refs.append(F.linear(it.double().view(n, K), w.double(), bias.double()))
            else:    # the rows are the im2col rows of a convolution without padding over channels-last [T, CIN] frames
                w3 = w.double().view(N, K // CIN, CIN).permute(0, 2, 1)
                refs.append(F.conv1d(it.double().view(-1, CIN).t()[None], w3, bias.double(), stride=lda // CIN)[0].t())
        _DATA[key] = (items, w, bias, refs)
    return _DATA[key]


def _run(gpu, N, K, lda, fill, exact, act=NONE, use_bias=True, order=None, pad=2):
    """the batch (items in `order`, `fill` behind every live run, `pad` more rows of it) through gemm_rows_f32 into NaN"""
    from easevoice_trainer_amd.hip.feat import gemm_rows_f32

    items, w, bias, _ = _data(N, K, lda, exact)
    order = list(range(len(LENS))) if order is None else order
    rows = max(LENS) + pad
    x = torch.full((len(order), _live(rows, K, lda)), fill)
    for i, b in enumerate(order):
        x[i, :items[b].numel()] = items[b]
    lens = torch.tensor([LENS[b] for b in order], dtype=torch.int32).to(gpu)
    y = torch.full((len(order), rows, N), NAN, device=gpu)
    with torch.no_grad():
        got = gemm_rows_f32(x.to(gpu), lens, w.to(gpu), bias.to(gpu) if use_bias else None, act, rows=rows, lda=lda, out=y)
    assert got is y
    return y


def _tag():
    from easevoice_trainer_amd.hip import lib as L

    return L.lib().evt_last_kernel_tag().decode()


@SHAPES
def test_exact(gpu, N, K, lda, fill):
    from easevoice_trainer_amd.hip.feat import gemm_rows_f32

    items, w, bias, refs = _data(N, K, lda, True)
    y = _run(gpu, N, K, lda, fill, True)
    assert torch.isfinite(y).all()
    for b, n in enumerate(LENS):
        assert torch.equal(y[b, :n].double().cpu(), refs[b]), (b, n)
        assert not y[b, n:].any(), (b, n)
    # lens = None: every row of every item is live
    full = [b for b, n in enumerate(LENS) if n == max(LENS)] * 3
    x = torch.stack([items[b] for b in full]).to(gpu)
    with torch.no_grad():
        y = gemm_rows_f32(x, None, w.to(gpu), bias.to(gpu), NONE, lda=lda)
    assert y.shape == (3, max(LENS), N)
    for i, b in enumerate(full):
        assert torch.equal(y[i].double().cpu(), refs[b])


@SHAPES
def test_fused_gelu_is_gelu_rows_of_the_plain_output(gpu, N, K, lda, fill):
    from easevoice_trainer_amd.hip.feat import gelu_rows

    bias = _data(N, K, lda, False)[2].to(gpu)
    plain = _run(gpu, N, K, lda, fill, False, NONE, use_bias=False)
    fused = _run(gpu, N, K, lda, fill, False, GELU)
    want = gelu_rows(plain, bias)
    for b, n in enumerate(LENS):
        assert torch.equal(fused[b, :n], want[b, :n]), (b, n)
        assert not fused[b, n:].any()


def test_rounding_against_float64_and_the_old_fp32_route(gpu):
    """max-abs error over max|ref| at K = 4096, N = 144, 130 rows: at most 4 x that of evt_gemm_bf16_fwd in EVT_DT_F32 (another
    fp32 MFMA summation order; test_mha_rows_gpu.py's margin), both under the fp32 stage tolerance 1e-3"""
    from easevoice_trainer_amd.hip.feat import gemm_rows_f32
    from easevoice_trainer_amd.hip.linear import LinearBank, gemm_fwd

    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(130, 4096, generator=g), torch.randn(144, 4096, generator=g)
    ref = x.double() @ w.double().t()
    wp = torch.nn.Parameter(w.to(gpu))
    bank = LinearBank([("w", wp, None)], torch.float32, gpu)
    bank.prepare()
    with torch.no_grad():
        new = gemm_rows_f32(x.to(gpu)[None], None, wp.data, None, NONE)[0]
        old = gemm_fwd(bank.slots[0], x.to(gpu))
    new_err, old_err = (float((t.double().cpu() - ref).abs().max() / ref.abs().max()) for t in (new, old))
    print(f"max-abs error / max|ref|  gemm_rows_f32 {new_err:.3e}  evt_gemm_bf16_fwd fp32 {old_err:.3e}")
    assert new_err <= 4 * old_err and new_err < 1e-3 and old_err < 1e-3


@SHAPES
def test_a_row_is_the_row_alone(gpu, N, K, lda, fill):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.feat import gemm_rows_f32

    items, w, bias, _ = _data(N, K, lda, False)
    L.lib().evt_debug_kernel_tags(1)
    try:
        base = _run(gpu, N, K, lda, fill, False, GELU)
        assert _tag().startswith("gemm_rows_f32<64,")                                 # 3 x 1..2 x 6 blocks of 128 x 128
        order = list(reversed(range(len(LENS)))) * 16                                 # 96 items: the large tile
        other = _run(gpu, N, K, lda, 1e30 if fill != fill else NAN, False, GELU, order=order, pad=9)
        assert _tag().startswith("gemm_rows_f32<128,")
    finally:
        L.lib().evt_debug_kernel_tags(0)
    for b, n in enumerate(LENS):
        for i in (order.index(b), len(order) - 1 - b):                                # its first and its last occurrence
            assert order[i] == b and torch.equal(other[i, :n], base[b, :n]), (b, n, i)
        if n:
            with torch.no_grad():
                alone = gemm_rows_f32(items[b].to(gpu)[None], None, w.to(gpu), bias.to(gpu), GELU, lda=lda)
            assert alone.shape == (1, n, N) and torch.equal(alone[0], base[b, :n]), (b, n)


def test_the_extractors_take_the_route(gpu):
    """tiny fp32 models: HubertModel.forward_rows (convolutions 2 - 7 with GELU, the dense layers) and a BertEncoderStack pass
    launch evt_gemm_rows_f32 and neither evt_conv1d_fwd's kernels for those layers nor evt_gelu_rows_fwd"""
    from easevoice_trainer_amd.feature_extractor import BertFeatures
    from easevoice_trainer_amd.feature_extractor.cnhubert import HubertModel
    from easevoice_trainer_amd.hip.trace import set_trace
    from easevoice_trainer_amd.runtime import ModelRuntime

    torch.manual_seed(0)
    net = HubertModel(hidden=64, heads=2, inner=128, layers=1, pos_k=128, pos_groups=4).eval()
    net._rt = ModelRuntime(net, dtype=torch.float32, device=gpu)
    net._rt.bank.weight_grads = False
    net._rt.prepare(force=True)
    bert = BertFeatures(None, gpu, torch.float32, vocab=64, hidden=64, heads=2, inner=128, num_layers=1, read_layer=1)
    for run, n_gelu, n_plain in ((lambda: net.forward_rows(torch.randn(2, 4000), [4000, 1700]), 7, 6),
                                 (lambda: bert.hidden_rows([[1, 5, 9, 2], [1, 7, 2]]), 1, 5)):
        rec = []
        set_trace(rec)
        try:
            with torch.no_grad():
                run()
            torch.cuda.synchronize()
        finally:
            set_trace(None)
        tags = [r[0] for r in rec]
        assert sum(t.startswith("gemm_rows_f32<") and t.endswith("gelu>") for t in tags) == n_gelu, tags
        assert sum(t.startswith("gemm_rows_f32<") and t.endswith("none>") for t in tags) == n_plain, tags
        assert all(r[1] == "elt" for r in rec if not r[0].startswith("gemm_rows_f32<")), tags    # no convolution launch is left
