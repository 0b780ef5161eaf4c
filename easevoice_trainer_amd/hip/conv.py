"""Host side of the fused Conv1d / ConvTranspose1d family: the parameter module with the reference's state_dict keys and
the autograd Functions that call the C ABI; re-exports hip/bank.py (prepared-weight banks), hip/wgrad.py (weight
gradients, their queue), hip/launch.py (single launches), hip/resunit.py (ResBlock units), hip/trace.py (tracing).

Layout contract: activations are channels-last [nseq, L, C] (contiguous); the reference's [B, C, L]
tensors are transposed once at the model boundary.  Reference modules mirrored:
torch.nn.Conv1d / ConvTranspose1d / Conv2d((k,1)) with optional old-style weight_norm
(`weight_g` / `weight_v` keys), src/easevoice/module/models.py:419-446,486-536,563-574,
modules.py:154-185,226-296.
"""
import ctypes as C
import os
import math

import torch
from torch import nn

from . import lib as L
from . import trace as T
# reached through this module by the package, tests and tools (not the mutable state: trace.TRACE, wgrad.GROUP_FLUSH)
from .bank import ConvSlot, FrozenBank, FrozenConv, PackedConv, WeightBank, conv_layout, slab_count  # noqa: F401
from .launch import _add3, _bias, _bwd_data, _fwd, _lrelu, mask_tail, resample_rows  # noqa: F401
from .resunit import (ResStageFn, ResUnitFn, _resunit_params, _resunit_wide_params, res_stage, res_unit,  # noqa: F401
                      resunit_bwd)
from .trace import set_trace, t0 as _t0  # noqa: F401
from .wgrad import WgGroup, WgJob, _bwd_weight, _bwd_weight_group, _bwd_weight_now  # noqa: F401


def __getattr__(name):
    if name in ("TRACE", "TRACE_RANGES"):      # the trace state, read where it lives: never a copy that could go stale
        return getattr(T, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class EvtConv1d(nn.Module):
    """Conv1d / ConvTranspose1d parameter holder.  Keys: `weight` (+`bias`) or `weight_g`/`weight_v`
    (+`bias`) exactly as torch's (old-style weight-normed) modules expose them; `kdims=2` appends the
    trailing size-1 kernel dim of DiscriminatorP's Conv2d((k,1)) weights; `kdims=0` (k = 1 only) drops the kernel dim:
    the `weight` [cout, cin] / `bias` of an nn.Linear, run as a 1x1 convolution over the rows."""

    def __init__(self, cin, cout, k, stride=1, padding=0, dilation=1, groups=1, bias=True, transposed=False,
                 weight_norm=False, kdims=1):
        super().__init__()
        self.cin, self.cout, self.k, self.stride, self.pad, self.dil = cin, cout, k, stride, padding, dilation
        self.groups, self.transposed, self.weight_norm, self.kdims = groups, transposed, weight_norm, kdims
        d0 = cin if transposed else cout
        d1 = cout if transposed else cin // groups
        if kdims == 0 and (k != 1 or transposed or groups != 1):
            raise L.EvtError("kdims=0 is the nn.Linear layout: k = 1, dense, not transposed")
        wshape = (d0, d1) if kdims == 0 else (d0, d1, k) + ((1,) if kdims == 2 else ())
        w = torch.empty(wshape)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        fan_in = d1 * k if not transposed else d0 * k  # torch: fan_in is computed from weight.size(1)*k
        fan_in = w.size(1) * k
        bias_p = None
        if bias:
            bound = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
            bias_p = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        # registration order = the reference's parameters() order, which numbers the optimiser state of a checkpoint:
        # plain conv (weight, bias); torch.nn.utils.weight_norm removes `weight` and appends weight_g, weight_v, so a
        # weight-normed conv enumerates as (bias, weight_g, weight_v)
        if weight_norm:
            self.register_parameter("bias", bias_p)
            self.weight_g = nn.Parameter(w.reshape(d0, -1).norm(dim=1).reshape((d0,) + (1,) * (w.dim() - 1)))
            self.weight_v = nn.Parameter(w)
        else:
            self.weight = nn.Parameter(w)
            self.register_parameter("bias", bias_p)
        self._slot = None            # the WeightBank finds its convolutions by this attribute

    @property
    def v(self):
        return self.weight_v if self.weight_norm else self.weight

    def lout(self, lin):
        if not self.transposed:
            return (lin + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        return (lin - 1) * self.stride - 2 * self.pad + self.dil * (self.k - 1) + 1

    def forward(self, x, res=None, in_slope=1.0, out_act=L.ACT_NONE, out_slope=1.0):
        if self._slot is None:
            raise L.EvtError("EvtConv1d used before WeightBank.attach(); there is no eager fallback")
        return ConvFn.apply(x, self._slot.bank.anchor, res, self._slot, float(in_slope), int(out_act),
                            float(out_slope))


PLAIN_X = os.environ.get("EVT_CONV_PLAIN_X", "1") != "0"   # A/B switch: pre-activated input for GEMM-sized layers with a load-side leaky-relu


class ConvFn(torch.autograd.Function):
    """y = act_out(conv(lrelu(x, in_slope)) + bias) + res, one HIP launch each way."""

    @staticmethod
    def forward(ctx, x, anchor, res, slot, in_slope, out_act, out_slope):
        ctx.pre = False
        if in_slope != 1.0 and x.is_cuda and x.dim() == 3 and PLAIN_X and L.lib().evt_conv1d_wants_plain_x(
                C.byref(slot.params(x.size(0), x.size(1), in_slope, out_act, out_slope))):
            # GEMM-sized layer with a leaky-relu on load (the vocoder's upsamplers): activate once, the forward and the
            # weight gradient then take plain operands (LDS-DMA kernels); backward-data keeps its fused derivative,
            # read from the sign of the activated tensor
            xa = _lrelu(x, in_slope, slot.module)
            y = _fwd(slot, xa, res, 1.0, out_act, out_slope)
            x, ctx.pre = xa, True
        else:
            y = _fwd(slot, x, res, in_slope, out_act, out_slope)
        ctx.slot, ctx.cfg = slot, (in_slope, out_act, out_slope)
        ctx.has_res = res is not None
        ctx.save_for_backward(x, y if out_act != L.ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        slot = ctx.slot
        in_slope, out_act, out_slope = ctx.cfg
        dy = dy.contiguous()
        nseq, lin = x.size(0), x.size(1)
        if out_act != L.ACT_NONE and L.lib().evt_conv1d_wants_plain_dy(
                C.byref(slot.params(nseq, lin, in_slope, out_act, out_slope))):
            # wide layers: apply the activation derivative once, both backward GEMMs then take plain operands
            dy_eff = torch.empty_like(dy)
            e0 = T.t0()
            L.check(L.lib().evt_dact_mul(L.dt_of(dy), L.ptr(dy), L.ptr(y), int(out_act), float(out_slope),
                                         L.ptr(dy_eff), dy.numel(), L.stream_ptr()), "evt_dact_mul")
            if e0 is not None:
                T.t1_elt(e0, "dact_mul_kernel", 3 * dy.numel() * dy.element_size(), slot.module)
            dy, y, out_act, out_slope = dy_eff, None, L.ACT_NONE, 1.0
        if slot.bank.weight_grads:
            # (ctx.pre: x is the activated input -- plain operand for the weight gradient)
            _bwd_weight(slot, x, dy, y, nseq, lin, 1.0 if ctx.pre else in_slope, out_act, out_slope)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _bwd_data(slot, dy, y, x, None, nseq, lin, in_slope, out_act, out_slope)
        dres = dy if (ctx.has_res and ctx.needs_input_grad[2]) else None
        if dres is not None and out_act != L.ACT_NONE:
            raise L.EvtError("residual + output activation: residual is added after the activation, "
                             "its gradient is dy (supported), but was not expected here")
        return dx, None, dres, None, None, None, None


class Add3ScaleFn(torch.autograd.Function):
    """(a + b + c) * scale — HiFi-GAN stage mean (models.py:457-466)."""

    @staticmethod
    def forward(ctx, a, b, c, scale, owner=None):
        out = _add3(a, b, c, scale, torch.empty_like(a), owner)
        ctx.scale, ctx.owner = scale, owner
        return out

    @staticmethod
    def backward(ctx, d):
        d = d.contiguous()
        g = _add3(d, None, None, ctx.scale, torch.empty_like(d), ctx.owner)
        return g, g, g, None, None


class GatedActFn(torch.autograd.Function):
    """tanh(a+ga) * sigmoid(b+gb) on channels-last [n, t, 2H] (+ g [n, 2H]) — commons.py:94-101."""

    @staticmethod
    def forward(ctx, xin, g):
        n, t, h2 = xin.shape
        acts = torch.empty((n, t, h2 // 2), dtype=xin.dtype, device=xin.device)
        L.check(L.lib().evt_gated_act_fwd(L.dt_of(xin), L.ptr(xin), L.ptr(g), L.ptr(acts), n, t, h2 // 2,
                                          L.stream_ptr()), "evt_gated_act_fwd")
        ctx.save_for_backward(xin, g)
        return acts

    @staticmethod
    def backward(ctx, dacts):
        xin, g = ctx.saved_tensors
        n, t, h2 = xin.shape
        dacts = dacts.contiguous()
        dxin = torch.empty_like(xin)
        dg32 = None
        if g is not None and ctx.needs_input_grad[1]:
            dg32 = torch.zeros((n, h2), dtype=torch.float32, device=xin.device)
        L.check(L.lib().evt_gated_act_bwd(L.dt_of(xin), L.ptr(xin), L.ptr(g), L.ptr(dacts), L.ptr(dxin), L.ptr(dg32),
                                          n, t, h2 // 2, L.stream_ptr()), "evt_gated_act_bwd")
        return dxin, (dg32.to(g.dtype) if dg32 is not None else None)
