"""GPU: one WN layer -- the one-launch kernels of csrc/wn_layer.hip (evt_wn_layer_fwd, evt_wn_layer_bwd_data) AND the four
launches each replaces (HC._fwd + evt_gated_act_fwd + HC._fwd + evt_wn_residual_fwd; evt_wn_residual_bwd + HC._bwd_data +
evt_gated_act_bwd + HC._bwd_data) -- against the float64 references of tests/wn_refs.py, which shares no code with the
library.  Operands, the exact-gate table, the bounds and the reasoning are there; their conditions and the comparators'
teeth are checked without a GPU by tests/test_wn_refs_cpu.py.

  exact regime      every output bit for bit (torch.equal on the stored type, dg as fp32), no element exempted, bf16 and f16,
                    ten shapes around the 16-position tile and the receptive field of 5, five layer roles each way;
  tolerance regime  randn operands, staged references, S.elementwise_excess <= 0 per output, no element exempted; the fp32
                    instantiations of the four launches too (a zero rounding bound), and evt_gated_act_bwd both with a dg
                    buffer (gated_bwd_dg_kernel) and without (gated_bwd_kernel);
  gate sweep        every finite 16-bit argument up to 2^7 through tanh and through sigmoid, both gate implementations.

Outputs are pre-filled with NaN, so an element a kernel does not write fails the comparison; every fused run asserts from
evt_last_kernel_tag that wn_layer_fwd< / wn_layer_bwd< was the kernel reached.
"""
import ctypes as C
import functools

import pytest
import torch

import exact_inputs as X
import s1_refs as S
import wn_refs as R

pytestmark = pytest.mark.gpu
H, K = R.H, R.K
F64 = torch.float64
DT = dict(bf16=torch.bfloat16, f16=torch.float16, f32=torch.float32)
NAN = float("nan")


class _Layer(torch.nn.Module):
    """one in_layer (k = 5, H -> 2H) and one res_skip layer (1 x 1, H -> 2H or H), weight-normed like the product's in the
    16-bit types (weight_g = X.weight_g_of(v): the 16-bit fold returns v); plain in fp32, where the fold's scale is 1 only to
    within 2 ulp (tests/test_exact_int_gpu.py, module docstring)"""

    def __init__(self, HC, p, last, wn):
        super().__init__()
        self.conv_in = HC.EvtConv1d(H, 2 * H, K, padding=(K - 1) // 2, weight_norm=wn)
        self.conv_rs = HC.EvtConv1d(H, H if last else 2 * H, 1, weight_norm=wn)
        with torch.no_grad():
            for m, w, b in ((self.conv_in, p["w_in"], p.get("b_in")), (self.conv_rs, p["w_rs"], p.get("b_rs"))):
                if wn:
                    m.weight_v.copy_(w)
                    m.weight_g.copy_(X.weight_g_of(w))
                else:
                    m.weight.copy_(w)
                m.bias.zero_() if b is None else m.bias.copy_(b)


def _setup(gpu, dtype, p, last):
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    m = _Layer(HC, p, last, wn=dtype != torch.float32).to(gpu)
    bank = HC.WeightBank(m, dtype, gpu)
    bank.build_tables()
    bank.fold()
    return HC, L, m, bank


def _nlc(t, gpu, dtype):
    return None if t is None else t.transpose(1, 2).contiguous().to(gpu, dtype)


def _ncl64(t):
    """what a kernel stored, as the references' layout and type"""
    return None if t is None else t.detach().cpu().to(F64).transpose(1, 2)


def _full(gpu, dtype, *shape):
    return torch.full(shape, NAN, dtype=dtype, device=gpu)


class _tagged:
    """the library's kernel-name record switched on around one launch (include/evt.h: off by default); .tag afterwards"""

    def __init__(self, L):
        self.lib, self.tag = L.lib(), None

    def __enter__(self):
        self.lib.evt_debug_kernel_tags(1)
        return self

    def __exit__(self, *exc):
        self.tag = self.lib.evt_last_kernel_tag().decode()
        self.lib.evt_debug_kernel_tags(0)


def _forward(gpu, dtype, p, lens, last, path):
    """x_in, acts, x_out, acc_out (and rs from the four launches) as stored, [B, T, C]"""
    HC, L, m, bank = _setup(gpu, dtype, p, last)
    si, sr = m.conv_in._slot, m.conv_rs._slot
    dt = L.dt_code(dtype)
    B, _, T = p["x"].shape
    x, acc = _nlc(p["x"], gpu, dtype), _nlc(p["acc"], gpu, dtype)
    g = None if p["g"] is None else p["g"].to(gpu, dtype).contiguous()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
    acts, acc_out = _full(gpu, dtype, B, T, H), _full(gpu, dtype, B, T, H)
    x_out = None if last else _full(gpu, dtype, B, T, H)
    if path == "fused":
        assert L.lib().evt_wn_layer_supported(dt, H, K, 1) == 1
        x_in = _full(gpu, dtype, B, T, 2 * H)
        frag_in, frag_rs = bank.frag(si, "reg"), bank.frag(sr, "reg")
        with _tagged(L) as t:
            L.check(L.lib().evt_wn_layer_fwd(dt, L.ptr(x), L.ptr(frag_in), L.ptr(m.conv_in.bias.data), L.ptr(frag_rs),
                                             L.ptr(m.conv_rs.bias.data), L.ptr(g), L.ptr(acc), L.ptr(lens_d), L.ptr(x_in),
                                             L.ptr(acts), L.ptr(x_out), L.ptr(acc_out), B, T, H, K, int(last), L.stream_ptr()),
                    "evt_wn_layer_fwd")
        assert t.tag.startswith("wn_layer_fwd<"), t.tag
        rs = None
    else:
        x_in = HC._fwd(si, x, None, 1.0, L.ACT_NONE, 1.0)
        L.check(L.lib().evt_gated_act_fwd(dt, L.ptr(x_in), L.ptr(g), L.ptr(acts), B, T, H, L.stream_ptr()), "gate")
        rs = HC._fwd(sr, acts, None, 1.0, L.ACT_NONE, 1.0)
        L.check(L.lib().evt_wn_residual_fwd(dt, L.ptr(None if last else x), L.ptr(rs), L.ptr(acc), L.ptr(lens_d), T,
                                            L.ptr(x_out), L.ptr(acc_out), C.c_int64(B * T), H, int(last), L.stream_ptr()),
                "residual")
    torch.cuda.synchronize()
    return dict(x_in=x_in, acts=acts, rs=rs, x_out=x_out, acc_out=acc_out)


def _backward(gpu, dtype, p, lens, last, path, want_dg=True):
    """drs, dx_in, dx, dg (and dacts from the four launches) as stored"""
    HC, L, m, bank = _setup(gpu, dtype, p, last)
    si, sr = m.conv_in._slot, m.conv_rs._slot
    dt = L.dt_code(dtype)
    B, _, T = p["dacc"].shape
    rs_w = H if last else 2 * H
    x_in, dacc, dx_next = _nlc(p["x_in"], gpu, dtype), _nlc(p["dacc"], gpu, dtype), _nlc(p["dx_next"], gpu, dtype)
    g = None if p["g"] is None else p["g"].to(gpu, dtype).contiguous()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
    drs, dx_in = _full(gpu, dtype, B, T, rs_w), _full(gpu, dtype, B, T, 2 * H)
    dg = torch.zeros(B, 2 * H, dtype=torch.float32, device=gpu) if (g is not None and want_dg) else None
    if path == "fused":
        dx = _full(gpu, dtype, B, T, H)
        alt_rs, alt_in = bank.frag(sr, "alt"), bank.frag(si, "alt")
        with _tagged(L) as t:
            L.check(L.lib().evt_wn_layer_bwd_data(dt, L.ptr(dx_next), L.ptr(dacc), L.ptr(x_in), L.ptr(g), L.ptr(alt_rs),
                                                  L.ptr(alt_in), L.ptr(lens_d), L.ptr(drs), L.ptr(dx_in), L.ptr(dx), L.ptr(dg),
                                                  B, T, H, K, int(last), L.stream_ptr()), "evt_wn_layer_bwd_data")
        assert t.tag.startswith("wn_layer_bwd<"), t.tag
        dacts = None
    else:
        dx_res = None if last else _full(gpu, dtype, B, T, H)
        L.check(L.lib().evt_wn_residual_bwd(dt, L.ptr(dx_next), L.ptr(dacc), L.ptr(lens_d), T, L.ptr(dx_res), L.ptr(drs),
                                            C.c_int64(B * T), H, int(last), L.stream_ptr()), "residual bwd")
        dacts = HC._bwd_data(sr, drs, None, None, None, B, T, 1.0, L.ACT_NONE, 1.0)
        L.check(L.lib().evt_gated_act_bwd(dt, L.ptr(x_in), L.ptr(g), L.ptr(dacts), L.ptr(dx_in), L.ptr(dg), B, T, H,
                                          L.stream_ptr()), "gate bwd")
        dx = HC._bwd_data(si, dx_in, None, None, dx_res, B, T, 1.0, L.ACT_NONE, 1.0)
    torch.cuda.synchronize()
    return dict(drs=drs, dacts=dacts, dx_in=dx_in, dx=dx, dg=dg)


# ---- exact regime -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_fwd(si, ri):
    """operands and reference of one case: the same for both types and both paths (nothing rounds)"""
    shape, role = R.SHAPES[si], R.FWD_ROLES[ri]
    p = R.exact_fwd_inputs(shape, role)
    return p, R.layer_forward(p, shape[2], role[1], torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _exact_bwd(si, ri):
    shape, role = R.SHAPES[si], R.BWD_ROLES[ri]
    p = R.exact_bwd_inputs(shape, role)
    return p, R.layer_backward(p, shape[2], role[1], torch.bfloat16)


_SHAPE_IDS = [R.shape_id(s) for s in R.SHAPES]


@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("si", range(len(R.SHAPES)), ids=_SHAPE_IDS)
def test_forward_exact(gpu, dn, si):
    dtype, shape = DT[dn], R.SHAPES[si]
    for ri, role in enumerate(R.FWD_ROLES):
        p, ref = _exact_fwd(si, ri)
        for path in ("fused", "four"):
            got = _forward(gpu, dtype, p, shape[2], role[1], path)
            ctx = f"[{R.shape_id(shape)} lens={shape[2]} {role[0]} {dn} {path}]"
            for name in ("x_in", "acts", "rs", "x_out", "acc_out"):
                if got[name] is not None:
                    X.assert_exact(got[name], ref[name], dtype, name, context=ctx)


@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("si", range(len(R.SHAPES)), ids=_SHAPE_IDS)
def test_backward_data_exact(gpu, dn, si):
    dtype, shape = DT[dn], R.SHAPES[si]
    for ri, role in enumerate(R.BWD_ROLES):
        p, ref = _exact_bwd(si, ri)
        for path in ("fused", "four"):
            got = _backward(gpu, dtype, p, shape[2], role[1], path)
            ctx = f"[{R.shape_id(shape)} lens={shape[2]} {role[0]} {dn} {path}]"
            for name in ("drs", "dacts", "dx_in", "dx"):
                if got[name] is not None:
                    X.assert_exact(got[name], ref[name], dtype, name, context=ctx)
            if ref["dg"] is not None:
                X.assert_exact(got["dg"], ref["dg"], torch.float32, "dg", nlc=False, context=ctx)


# ---- tolerance regime ---------------------------------------------------------------------------------------------------------
def _runs(dn):
    """(path, formula of the gate it states): fp32 exists as four launches only"""
    return [("four", "libm")] if dn == "f32" else [("fused", "exp2"), ("four", "libm")]


def _assert_within(out, ctx):
    for name, (exc, ratio) in out.items():
        print(f"{ctx} {name}: excess {exc:.3g}, {ratio:.3f} of the bound")
    bad = {n: v for n, v in out.items() if not v[0] <= 0}           # (a NaN -- an unwritten element -- is not <= 0)
    assert not bad, f"{ctx} beyond the bound: {bad}"


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", R.TOL_SHAPES, ids=R.shape_id)
def test_forward_within_bounds(gpu, dn, shape):
    dtype = DT[dn]
    for role in R.FWD_ROLES:
        p = R.tol_fwd_inputs(shape, role, torch.bfloat16 if dn == "f32" else dtype)
        for path, form in _runs(dn):
            got = {k: _ncl64(v) for k, v in _forward(gpu, dtype, p, shape[2], role[1], path).items()}
            out = R.fwd_checks(p, shape[2], role[1], dtype, got, form)
            _assert_within(out, f"[{R.shape_id(shape)} {role[0]} {dn} {path}]")
            masked = 1 - R.live(shape[2], shape[1])
            zero = got["acc_out"] if role[1] else got["x_out"]
            assert float((zero * masked).abs().max()) == 0.0                   # masked rows are exact zeros


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", R.TOL_SHAPES, ids=R.shape_id)
def test_backward_data_within_bounds(gpu, dn, shape):
    dtype = DT[dn]
    for role in R.BWD_ROLES:
        p = R.tol_bwd_inputs(shape, role, torch.bfloat16 if dn == "f32" else dtype)
        for path, form in _runs(dn):
            ctx = f"[{R.shape_id(shape)} {role[0]} {dn} {path}]"
            raw = _backward(gpu, dtype, p, shape[2], role[1], path)
            got = {k: (_ncl64(v) if k != "dg" else (None if v is None else v.cpu().to(F64))) for k, v in raw.items()}
            _assert_within(R.bwd_checks(p, shape[2], role[1], dtype, got, form, add_after_rounding=path == "four"), ctx)
            if path == "four" and p["g"] is not None:
                # the same launches without a dg buffer: gated_bwd_kernel instead of gated_bwd_dg_kernel
                raw = _backward(gpu, dtype, p, shape[2], role[1], path, want_dg=False)
                assert raw["dg"] is None
                got = {k: _ncl64(v) for k, v in raw.items()}
                _assert_within(R.bwd_checks(p, shape[2], role[1], dtype, got, form, add_after_rounding=True),
                               ctx + " no dg buffer")


# ---- gate sweep ---------------------------------------------------------------------------------------------------------------
def _sweep(gpu, dtype, path, ga, gb):
    """acts[s, 0, h] = tanh(ga[s, h]) sigmoid(gb[s, h]) through the forward with x = 0, zero biases and T = 1"""
    B = ga.size(0)
    p = dict(w_in=X.dense_pm((2 * H, H, K), X.gen("sweep")), w_rs=X.dense_pm((2 * H, H, 1), X.gen("sweep", 2)), b_in=None,
             b_rs=None, x=torch.zeros(B, H, 1, dtype=F64), g=torch.cat([ga, gb], 1), acc=None)
    got = _forward(gpu, dtype, p, (1,) * B, False, path)
    assert float(got["x_in"].float().abs().max()) == 0.0
    return got["acts"].cpu().to(F64).view(B, H)


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_gate_sweep(gpu, dn):
    """tanh (with sigmoid held at +512 -> 1) and sigmoid (with tanh held at +512 -> 1) at every finite 16-bit argument of both
    signs from 2^-20 (bf16: 6917 values) / the smallest subnormal (f16: 45059 values) to 2^7, and at 0 and +-512, through the
    fused forward (rcp / exp2: wn_layer.hip sigmoid_f, tanh_f) and through evt_gated_act_fwd (tanhf, 1 / (1 + __expf)).
    Asserted: |stored - float64| <= round_bound (1 + 2^-10) + slack, slack = 4 x the largest deviation of the stated
    formula evaluated in float32 on the CPU; exact values at the points the exact regime of tests/wn_refs.py rests on:
    tanh(0) = 0, tanh(+-512) = +-1, sigmoid(+512) = 1, sigmoid(-512) = 0, sigmoid(0) = 1/2.
    The exact points hold on an MI355X for both implementations, so no row of the exact-gate table had to be dropped.
    Measured there (printed under `-s`; the figures stand at csrc/wn_layer.hip's sigmoid_f too).  `ulp` = spacing of the
    stored type at the float64 value, so 0.5 is a correctly rounded result; `beyond` = the largest |error| minus half that
    spacing, what the final rounding cannot account for:
                          slack     beyond                        largest error in ulp
      bf16 fused tanh     6.8e-7    8.5e-8 at -1.04e-6            12 at -1.04e-6 (-9.54e-7 stored for -1.043e-6)
      bf16 fused sigmoid  3.4e-7    9.9e-39 at -87.5              109 at -87.5 (0 stored for 1.0e-38: an fp32 subnormal, flushed)
      bf16 four  tanh     1.2e-7    none                          0.498 at 0.0903
      bf16 four  sigmoid  3.4e-7    2.2e-39 at -89                24 at -89 (0 stored for 2.2e-39: flushed likewise)
      f16  fused tanh     7.1e-7    9.4e-8 at -2.96e-4            1.0 at 4.08e-4 (4.0865e-4 stored for 4.0841e-4)
      f16  fused sigmoid  3.5e-7    none                          0.5
      f16  four  tanh     1.2e-7    none                          0.5
      f16  four  sigmoid  3.5e-7    none                          0.5
    The absolute bound holds everywhere with a factor of 7 to spare; the relative excess of the fused tanh near 0 is the
    cancellation in 2 s - 1 and is left alone (a gradient that small is nothing training sees).
    """
    dtype = DT[dn]
    v = R.sweep_values(dtype)
    hold = torch.full_like(v, R.SAT)
    exact = {0.0: (0.0, 0.5), R.SAT: (1.0, 1.0), -R.SAT: (-1.0, 0.0)}
    for path, form in (("fused", "exp2"), ("four", "libm")):
        for fn, ga, gb in (("tanh", v, hold), ("sigmoid", hold, v)):
            got = _sweep(gpu, dtype, path, ga, gb)
            ref = torch.tanh(v) if fn == "tanh" else torch.sigmoid(v)
            v32 = v.float()
            run32 = R.tanh_form(v32, form) if fn == "tanh" else R.sigmoid_form(v32, form)
            slack = S.slack_of(run32, ref)
            err = (got - ref).abs()
            ulps = err / R.spacing(ref, dtype)
            beyond = err - S.round_bound(ref, dtype)          # what the final rounding cannot account for: the gate's own
            i, j = int(beyond.argmax()), int(ulps.argmax())
            print(f"gate sweep {dn} {path} {fn}: slack {slack:.3g}; largest |error| beyond the final rounding "
                  f"{float(beyond.flatten()[i]):.3g} at {float(v.flatten()[i])!r}; largest error {float(ulps.flatten()[j]):.3g} ulp at {float(v.flatten()[j])!r} "
                  f"(got {float(got.flatten()[j])!r}, float64 {float(ref.flatten()[j])!r})")
            for arg, (t_want, s_want) in exact.items():
                at = got[v == arg]
                want = t_want if fn == "tanh" else s_want
                assert at.numel() and bool((at == want).all()), (dn, path, fn, arg, at)
            exc = S.elementwise_excess(got, ref, dtype, slack)
            assert exc <= 0, (dn, path, fn, exc)
