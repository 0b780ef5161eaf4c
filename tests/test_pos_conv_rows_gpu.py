"""evt_pos_conv_rows (csrc/pos_conv.hip): HuBERT's grouped k = 128 positional convolution on ragged rows, bias + GELU fused.
Inputs are exact by construction (ternary x and w, 75 % zeros; integer or eighth bias): every product and partial sum is an
integer exact in fp32 and the operands are exact in all three types, so the linear part is compared with torch.equal against
float64 torch.nn.functional.conv1d of each row alone."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
SHAPES = pytest.mark.parametrize("shape", [(768, 16, 128), (128, 4, 15)], ids=["hubert", "cg32k15"])
TILE = 256                                                          # EVT_POS_CONV_TILE
LENS = (1, 63, TILE - 1, TILE, TILE + 1, 2 * TILE + 37)
TMAX = max(LENS) + 5
_CASES = {}


def _case(shape):
    """rows, weight, the two biases and the float64 convolution of each row alone ([n_b, C], no bias), built once"""
    if shape not in _CASES:
        ch, groups, k = shape
        g = torch.Generator().manual_seed(5)
        tern = lambda *s: (torch.randint(-1, 2, s, generator=g) * (torch.rand(s, generator=g) < 0.25)).float()  # noqa: E731
        x, w = tern(len(LENS), TMAX, ch), tern(ch, ch // groups, k)
        bias_int = torch.randint(-2, 3, (ch,), generator=g).float()
        bias_8th = torch.randint(-8, 9, (ch,), generator=g).float() / 8
        refs = []
        for b, n in enumerate(LENS):
            y = torch.nn.functional.conv1d(x[b, :n].double().T[None], w.double(), padding=k // 2, groups=groups)[0]
            refs.append((y[:, :-1] if k % 2 == 0 else y).T.contiguous())
            assert (refs[-1] + bias_int).abs().max() <= 256           # exact integers in bfloat16
        _CASES[shape] = dict(x=x, w=w, bias_int=bias_int, bias_8th=bias_8th, refs=refs)
    return _CASES[shape]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _ops(gpu, dtype, shape, fill=0.0):
    """x (with `fill` at and behind each row's length), lens and the packed image on the GPU"""
    from easevoice_trainer_amd.hip import feat
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    case = _case(shape)
    x = case["x"].clone()
    for b, n in enumerate(LENS):
        x[b, n:] = fill
    return (x.to(gpu, dtype), torch.tensor(LENS, dtype=torch.int32).to(gpu),
            feat.pos_conv_image(case["w"].to(gpu), shape[1], dtype))


def _raw(dtype_code, x, lens, shape, image, bias, act, out, nseq=None, T=None):
    from easevoice_trainer_amd.hip import lib as L

    p = lambda t: C.c_void_p(t if isinstance(t, int) else (t.data_ptr() if t is not None else 0))  # noqa: E731
    ch, groups, k = shape
    return L.lib().evt_pos_conv_rows(dtype_code, p(x), p(lens), x.size(0) if nseq is None else nseq,
                                     x.size(1) if T is None else T, ch, groups, k, p(image), p(bias), act, p(out),
                                     L.stream_ptr())


@SHAPES
@DTYPES
def test_linear_part_is_exact_and_every_element_is_written(gpu, dtype, shape):
    from easevoice_trainer_amd.hip import lib as L

    case = _case(shape)
    x, lens, image = _ops(gpu, dtype, shape)
    out = torch.full_like(x, 1024.0)                                 # the sentinel: no live value reaches it
    assert _raw(L.dt_code(dtype), x, lens, shape, image, case["bias_int"].to(gpu), 0, out) == 0
    for b, n in enumerate(LENS):
        assert torch.equal(out[b, :n].double().cpu(), case["refs"][b] + case["bias_int"]), (b, n)
        assert not out[b, n:].any(), f"row {b}: tail not exactly zero"


@SHAPES
@DTYPES
def test_fused_bias_and_gelu(gpu, dtype, shape):
    from easevoice_trainer_amd.hip import feat

    case = _case(shape)
    x, lens, image = _ops(gpu, dtype, shape)
    bias = case["bias_8th"].to(gpu)
    got = feat.pos_conv_rows(x, lens, image, bias, shape[1], shape[2], gelu=True)
    if dtype == torch.float32:    # fp32 accumulators stored exactly + the shared GELU function: nothing may differ
        want = feat.gelu_rows(feat.pos_conv_rows(x, lens, image, None, shape[1], shape[2], gelu=False), bias)
    u = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}[dtype]
    for b, n in enumerate(LENS):
        if dtype == torch.float32:
            assert torch.equal(_bits(got[b, :n]), _bits(want[b, :n])), (b, n)
            continue
        pre = case["refs"][b] + case["bias_8th"]
        ref = 0.5 * pre * (1 + torch.erf(pre / 2.0 ** 0.5))
        err = (got[b, :n].double().cpu() - ref).abs()
        bound = u * ref.abs() + 1e-6 * pre.abs().clamp(min=1)       # one rounding of the output type + fp32 erff
        print(f"{dtype} row {b}: max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (b, n)


@SHAPES
@DTYPES
def test_padding_and_neighbours_do_not_enter(gpu, dtype, shape):
    from easevoice_trainer_amd.hip import feat

    bias = _case(shape)["bias_8th"].to(gpu)
    x, lens, image = _ops(gpu, dtype, shape)
    base = feat.pos_conv_rows(x, lens, image, bias, shape[1], shape[2])
    assert torch.isfinite(base.float()).all()
    for fill in (float("nan"), 1e30):
        xf = _ops(gpu, dtype, shape, fill)[0]
        assert torch.equal(_bits(feat.pos_conv_rows(xf, lens, image, bias, shape[1], shape[2])), _bits(base)), fill
    for b, n in enumerate(LENS):
        alone = feat.pos_conv_rows(x[b:b + 1, :n].contiguous(), lens[b:b + 1], image, bias, shape[1], shape[2])
        assert torch.equal(_bits(alone[0]), _bits(base[b, :n])), (b, n)


def test_refusals(gpu):
    from easevoice_trainer_amd.hip import feat
    from easevoice_trainer_amd.hip import lib as L

    shape = (128, 4, 15)
    x, lens, image = _ops(gpu, torch.bfloat16, shape)
    out, bias = torch.empty_like(x), _case(shape)["bias_int"].to(gpu)
    assert _raw(1, x, lens, shape, image, bias, 1, out) == 0
    for kw in (dict(x=None), dict(image=None), dict(out=None), dict(nseq=0), dict(nseq=65536), dict(T=0), dict(shape=(128, 0, 15)),
               dict(x=x.data_ptr() + 2), dict(out=out.data_ptr() + 8), dict(image=image.data_ptr() + 4),
               dict(bias=bias.data_ptr() + 4)):
        args = dict(x=x, lens=lens, shape=shape, image=image, bias=bias, act=1, out=out, nseq=x.size(0), T=x.size(1))
        args.update(kw)
        assert _raw(1, **args) == 22, kw
    for code, shp in ((1, (96, 4, 16)), (1, (128, 4, 129)), (1, (128, 4, 1)), (1, (64, 4, 15)), (2, shape), (7, shape)):
        assert _raw(code, x, lens, shp, image, bias, 1, out, T=1) == 95, (code, shp)      # cg = 24, k = 129, ..., the f16 code
    assert L.lib().evt_pos_conv_pack(1, _case(shape)["w"].to(gpu).data_ptr(), 96, 4, 16, image.data_ptr(), L.stream_ptr()) == 95
    for bad in (dict(lens=lens.long()), dict(lens=lens.cpu()), dict(lens=lens[:-1]), dict(x=x.transpose(0, 1)),
                dict(image=image.float()), dict(bias=bias.double())):
        args = dict(x=x, lens=lens, image=image, bias=bias, groups=4, k=15)
        args.update(bad)
        with pytest.raises(L.EvtError):
            feat.pos_conv_rows(**args)


def _hf_hubert(seed=0):
    """the random-initialised base model of test_hubert_rows_gpu.py::_hf_hubert, restated"""
    from transformers import HubertConfig
    from transformers import HubertModel as HF

    torch.manual_seed(seed)
    hf = HF(HubertConfig()).eval()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if n.endswith("layer_norm.weight") or n.endswith("LayerNorm.weight"):
                p.add_(0.1 * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.add_(0.05 * torch.randn_like(p))
    return hf


def test_model_takes_the_kernel(gpu):
    from easevoice_trainer_amd.feature_extractor import CNHubert
    from easevoice_trainer_amd.hip import conv as HC

    hf = _hf_hubert()
    hub = CNHubert(hf.state_dict(), gpu, torch.float32)
    frames = (1, 28, 300)
    p = torch.randn(3, 303, 768, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        got = hub.model.encoder.pos_conv_embed(p.to(gpu), torch.tensor(frames, dtype=torch.int32).to(gpu)).cpu()
        for b, n in enumerate(frames):
            ref = hf.encoder.pos_conv_embed(p[b:b + 1, :n])[0]
            assert float((got[b, :n] - ref).abs().max() / ref.abs().max()) < 1e-3, (b, n)
            assert not got[b, n:].any()
    rec = []
    HC.set_trace(rec)
    try:
        clips = [0.1 * torch.randn(n, generator=torch.Generator().manual_seed(n)) for n in (400, 9000)]
        hub.last_hidden_state_batch(clips)
        torch.cuda.synchronize()
    finally:
        HC.set_trace(None)
    assert rec and not any(r[0].startswith("conv_naive") for r in rec), sorted({r[0] for r in rec})
