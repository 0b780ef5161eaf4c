"""Operands, float64 references and bounds of tests/test_wn_layer_exact_gpu.py (and of their CPU-side conditions,
tests/test_wn_refs_cpu.py) for one layer of the gated WN stack: the one-launch kernels of csrc/wn_layer.hip
(evt_wn_layer_fwd, evt_wn_layer_bwd_data) and the four launches each of them replaces, csrc/elementwise.hip's gate kernels
among them.  Nothing here touches a GPU, the library or oracle/: the convolutions are torch.nn.functional.conv1d /
conv_transpose1d in float64 (tests/test_wn_refs_cpu.py checks the backward formulas against autograd of the forward), the
helpers are those of tests/exact_inputs.py (X) and tests/s1_refs.py (S).  H = 192 and k = 5 throughout
(evt_wn_layer_supported serves nothing else).  Reference layout: activations [B, C, T], g [B, 2H].

    x_in = in_layer(x) + b_in                 k = 5, 'same' padding               stored, 16 bits
    acts = tanh(x_in[:H] + g[:H]) * sigmoid(x_in[H:] + g[H:])                     stored, 16 bits
    rs   = res_skip(acts) + b_rs              1 x 1                               rounded to 16 bits (wn_layer.hip, header)
    x_out = (x + rs[:H]) * mask, acc_out = acc + rs[H:]        last layer: acc_out = (acc + rs) * mask
  backward-data, from (dx_next, dacc, x_in, g, lens):
    drs   = [dx_next * mask | dacc]           last layer: dacc * mask
    dacts = res_skip^T drs                                                         rounded to 16 bits (wn_layer_bwd: `d`) 
    da = dacts s (1 - t^2), db = dacts t s (1 - s);  dx_in = [da | db] stored;  dg[seq] = sum over ALL T positions of the
         unrounded [da | db] (the gate kernels know no lengths; behind a last layer dacc arrives masked)
    dx    = in_layer^T dx_in + dx_next * mask

EXACT REGIME.  Small-integer operands make both convolutions exact in any summation order (tests/exact_inputs.py); the gate
is driven only to points where every implementation owes an exact value (a = tanh argument, b = sigmoid argument):

    a            b             t, s       acts     da, db
    +-512 + x_in +512 + x_in   +-1, 1     +-1      0, 0
    anything     -512 + x_in   . , 0      0        0, 0
    0            +512          0, 1       0        d, 0
    0            0             0, 1/2     0        d/2, 0
    +-512        0             +-1, 1/2   +-1/2    0, +-d/4

which rests on exp2 / exp / rcp / division being exact at 2^(+-inf) -> 0 / inf, 2^0 = 1, 1 / 1, 1 / 2 and 1 / inf
(tests/test_wn_layer_exact_gpu.py::test_gate_sweep contains these points and asserts them).
Forward with g: x sparse over {+-1, +-2} at the project's plain budget of 160 non-zero products per x_in element
(exact_inputs.FUSIONS[0]), weights dense over {+-1, +-2}, biases and acc small integers, g per (sequence, channel) from
{+512, -512}: rows one and two of the table, acts in {0, +-1}.  Forward without g: the saturation offset sits in b_in
(+-512 per channel), and the stored x_in = sum + bias has to stay a 16-bit number: bfloat16 spaces the values between 512
and 1024 by 4, so x is drawn from {+-4, +-8} and every stored x_in is a multiple of 4.  The gate has to stay saturated as
well: a fp32 sigmoid is exactly 0 only from exp(88.7) = inf on, and the 16-bit product only below the smallest bfloat16
subnormal, sigmoid(-93); with a margin, |x_in| >= 128, that is |sum| <= 384 (and |x_in| <= 896 < 256 steps of 4).
TX_NOG = 44 non-zero products per element (a density of 44 / 960 = 4.6 %) is the largest multiple of 4 at which EVERY
element of every case below holds that (the largest |sum| is then 364; at 48 one element reaches 408).
Backward: x_in is an input, set per element to the table's points (minus g, which is drawn from {0, +-512}); a fraction
BWD_TERMS / (2H min(k, T)) of the elements goes to the last three rows, the rest to the zero-gradient rows; dx_next and
dacc are sparse over {+-1, +-2} with BWD_T1 non-zero products per dacts element.  dx_in is then a multiple of 1/4 and dx,
dg exact sums of such.  Conditions (tests/test_wn_refs_cpu.py, on all elements): every stored tensor an integer multiple of
its step of at most 256 steps (the bfloat16 limit, used for IEEE half as well), dg below 2^24 steps.

TOLERANCE REGIME.  randn operands rounded to the stored type; staged references -- stage n reads what the kernel stored
for stage n - 1 (itself checked), so each stage sees one rounding.  Per element
    bound = round_bound(ref, dtype) (1 + 2^-10) + sum_bound(sum |terms|, number of addends) + slack
where the gate's slack is 4 x the largest deviation of a float32 CPU evaluation of the formula the kernel states from the
float64 one (S.slack_of), never the kernel's own numbers.  rs (forward) and dacts (backward) are rounded to 16 bits INSIDE
the one-launch kernels without being stored: a value within sum_bound of a rounding boundary may land on either side, so
the next stage takes both ends, round(ref - sum_bound) and round(ref + sum_bound) -- equal on most elements, neighbours
on some, further apart only where the value is so small that sum_bound exceeds its spacing; the next stage is monotone in
them (a sum, a product) -- and every element has to meet the bound against the nearest point of that range (`judge`).
The four-launch path stores rs and dacts: there the next stage reads the stored tensor.  That path also adds dx_next to
the k = 5 backward-data result in an epilogue that may round the result first (`bwd_checks`, add_after_rounding).
"""
import torch
import torch.nn.functional as F

import exact_inputs as X
import s1_refs as S

H, K, PAD, TILE = 192, 5, 2, 16
F64 = torch.float64
SAT = 512.0
LOG2E_F32 = 1.4426950408889634

TX_G = X.FUSIONS[0]["tx"]      # 160 non-zero products per x_in element, steps of 1
TX_NOG = 44                    # without g: steps of 4, see above
BWD_T1 = 2                     # non-zero products per dacts element
BWD_TERMS = 8                  # non-zero products per dx element (dx_in in quarter steps)

_PRODUCT_LENS = (200, 1, 16, 17, 199, 33, 64, 100, 150, 5, 48, 47, 128, 177, 80, 2)
SHAPES = [
    (1, 1, (1,)), (2, 2, (2, 1)), (2, 4, (4, 3)),                     # T below the receptive field
    (3, 15, (15, 1, 8)), (3, 16, (16, 15, 1)), (3, 17, (17, 16, 2)),  # the 16-position tile - 1 / + 0 / + 1
    (2, 31, (31, 17)), (2, 33, (33, 32)), (4, 50, (50, 48, 47, 3)),
    (16, 200, _PRODUCT_LENS),                                         # the product's shape
]
TOL_SHAPES = [SHAPES[5], SHAPES[8], SHAPES[9]]
# (name, last, with_g, with_acc): the roles of tests/test_wn_layer_gpu.py
FWD_ROLES = [("first_g", False, True, False), ("middle_g", False, True, True), ("middle", False, False, True),
             ("last_g_acc", True, True, True), ("last", True, False, False)]
# (name, last, with_g, with_dx_next)
BWD_ROLES = [("last_g", True, True, False), ("middle_g", False, True, True), ("middle", False, False, True),
             ("first_g", False, True, True), ("first_nodx", False, False, False)]


def shape_id(shape):
    return f"{shape[0]}x{shape[1]}"


def live(lens, T):
    """[B, 1, T] float64: 1 where position < len"""
    return (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).to(F64).unsqueeze(1)


def q(t, dtype):
    """rounded to the stored type, as float64"""
    return t.to(dtype).to(F64)


def _sign(shape, g):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


# ---- the layer, float64 -----------------------------------------------------------------------------------------------------
def gate(x_in, g):
    a, b = x_in[:, :H], x_in[:, H:]
    if g is not None:
        a, b = a + g[:, :H, None], b + g[:, H:, None]
    return a, b


def layer_forward(p, lens, last, dtype):
    """x_in, acts, rs, x_out (None when last), acc_out: float64 with the kernels' rounding points; `raw`: the sums before
    their rounding (what the conditions of the exact regime are checked on)"""
    x = p["x"]
    raw = dict(x_in=F.conv1d(x, p["w_in"], p["b_in"], padding=PAD))
    x_in = q(raw["x_in"], dtype)
    a, b = gate(x_in, p["g"])
    acts = q(torch.tanh(a) * torch.sigmoid(b), dtype)
    raw["rs"] = F.conv1d(acts, p["w_rs"], p["b_rs"])
    rs = q(raw["rs"], dtype)
    raw["x_out"], raw["acc_out"] = tail(x, p["acc"], rs, lens, last)
    return dict(x_in=x_in, acts=acts, rs=rs, x_out=None if last else q(raw["x_out"], dtype),
                acc_out=q(raw["acc_out"], dtype), raw=raw)


def tail(x, acc, rs, lens, last):
    m = live(lens, x.size(2))
    acc = torch.zeros_like(x) if acc is None else acc
    if last:
        return None, (acc + rs) * m
    return (x + rs[:, :H]) * m, acc + rs[:, H:]


def drs_of(dx_next, dacc, lens, last):
    m = live(lens, dacc.size(2))
    if last:
        return dacc * m
    return torch.cat([(torch.zeros_like(dacc) if dx_next is None else dx_next * m), dacc], 1)


def gate_grads(x_in, g, d):
    """(da, db) of acts = tanh(a) sigmoid(b) at upstream gradient d, float64"""
    a, b = gate(x_in, g)
    t, s = torch.tanh(a), torch.sigmoid(b)
    return d * s * (1 - t * t), d * t * s * (1 - s)


def layer_backward(p, lens, last, dtype):
    """drs, dacts, dx_in, dx (rounded where the kernels round) and dg (fp32 sum of the unrounded gate gradients)"""
    drs = drs_of(p["dx_next"], p["dacc"], lens, last)
    raw = dict(dacts=F.conv_transpose1d(drs, p["w_rs"]))
    dacts = q(raw["dacts"], dtype)
    v = torch.cat(gate_grads(p["x_in"], p["g"], dacts), 1)
    # (sigmoid(-512) is 1e-223 in float64 and 0 in fp32, the type the kernels hold these in and sum into dg)
    raw["dx_in"] = torch.where(v.abs() < 2.0 ** -126, torch.zeros_like(v), v)
    dx_in = q(raw["dx_in"], dtype)
    dx = F.conv_transpose1d(dx_in, p["w_in"], padding=PAD)
    if not last:
        dx = dx + drs[:, :H]
    raw["dx"] = dx
    dg = raw["dx_in"].sum(2) if p["g"] is not None else None
    return dict(drs=drs, dacts=dacts, dx_in=dx_in, dx=q(dx, dtype), dg=dg, raw=raw)


# ---- exact operands -----------------------------------------------------------------------------------------------------------
def exact_fwd_inputs(shape, role):
    B, T, _lens = shape
    name, last, with_g, with_acc = role
    g_ = X.gen("wn_fwd", B, T, name)
    rs_c = H if last else 2 * H
    p = dict(w_in=X.dense_pm((2 * H, H, K), g_), w_rs=X.dense_pm((rs_c, H, 1), g_), b_rs=X.small_int((rs_c,), g_))
    if with_g:
        p["x"] = X.sparse_pm((B, H, T), g_, TX_G / (H * K))
        p["b_in"] = X.small_int((2 * H,), g_)
        p["g"] = SAT * _sign((B, 2 * H), g_)
    else:
        p["x"] = 4.0 * X.sparse_pm((B, H, T), g_, TX_NOG / (H * K))
        p["b_in"] = SAT * _sign((2 * H,), g_)
        p["g"] = None
    p["acc"] = X.small_int((B, H, T), g_) if with_acc else None
    return p


def fwd_steps(role):
    """the step every stored tensor of a forward case is a multiple of"""
    return dict(x=1.0 if role[2] else 4.0, x_in=1.0 if role[2] else 4.0, acts=1.0, rs=1.0, x_out=1.0, acc_out=1.0, acc=1.0)


def exact_bwd_inputs(shape, role):
    B, T, _lens = shape
    name, last, with_g, with_dx = role
    g_ = X.gen("wn_bwd", B, T, name)
    rs_c = H if last else 2 * H
    p = dict(w_in=X.dense_pm((2 * H, H, K), g_), w_rs=X.dense_pm((rs_c, H, 1), g_))
    p["g"] = SAT * torch.randint(-1, 2, (B, 2 * H), generator=g_).double() if with_g else None
    n = (B, H, T)
    sparse = torch.rand(n, generator=g_, dtype=F64) < BWD_TERMS / (2 * H * min(K, T))
    kind = torch.where(sparse, torch.randint(2, 5, n, generator=g_), torch.randint(0, 2, n, generator=g_))
    sat = SAT * _sign(n, g_)
    anything = torch.tensor([0.0, 4.0, -4.0, SAT, -SAT], dtype=F64)[torch.randint(0, 5, n, generator=g_)]
    zero = torch.zeros(n, dtype=F64)
    ta = torch.where(kind == 0, sat, torch.where(kind == 1, anything, torch.where(kind == 4, sat, zero)))
    tb = torch.where(kind == 0, SAT + zero, torch.where(kind == 1, zero - SAT, torch.where(kind == 2, SAT + zero, zero)))
    x_in = torch.cat([ta, tb], 1)
    if with_g:
        x_in = x_in - p["g"][:, :, None]
    p["x_in"] = x_in
    p["kind"] = kind
    cin_live = H * (2 if (with_dx and not last) else 1)
    p["dacc"] = X.sparse_pm(n, g_, min(1.0, BWD_T1 / cin_live))
    p["dx_next"] = X.sparse_pm(n, g_, min(1.0, BWD_T1 / cin_live)) if (with_dx and not last) else None
    return p


BWD_STEPS = dict(x_in=4.0, dacc=1.0, dx_next=1.0, drs=1.0, dacts=1.0, dx_in=0.25, dx=0.25)


# ---- the fp32 yardsticks: the formulas the kernels state, evaluated in float32 on the CPU -------------------------------------
def sigmoid_form(x, form):
    """wn_layer.hip sigmoid_f ("exp2": rcp(1 + exp2(-x log2 e))) / elementwise.hip sigmoid_f ("libm": 1 / (1 + exp(-x))),
    in x's type"""
    if form == "exp2":
        return 1.0 / (1.0 + torch.exp2(x * torch.tensor(-LOG2E_F32, dtype=x.dtype)))
    return 1.0 / (1.0 + torch.exp(-x))


def tanh_form(x, form):
    """wn_layer.hip tanh_f (2 sigmoid(2x) - 1: 2 s is exact, so the fma rounds once, as this does) / tanhf"""
    if form == "exp2":
        return 2.0 * sigmoid_form(2.0 * x, form) - 1.0
    return torch.tanh(x)


def gate_form(x_in, g, form, dt):
    a, b = gate(x_in.to(dt), None if g is None else g.to(dt))
    return tanh_form(a, form) * sigmoid_form(b, form)


def gate_grads_form(x_in, g, d, form, dt):
    a, b = gate(x_in.to(dt), None if g is None else g.to(dt))
    t, s, d = tanh_form(a, form), sigmoid_form(b, form), d.to(dt)
    return d * s * (1 - t * t), d * t * s * (1 - s)


# ---- staged references and bounds ------------------------------------------------------------------------------------------------
def conv_stage(x, w, b, transposed=False, pad=0):
    """(float64 result, sum_bound of it): the number of addends is the reduction length (+ 1 for the bias)"""
    f = F.conv_transpose1d if transposed else F.conv1d
    ref = f(x, w, b, padding=pad)
    mag = f(x.abs(), w.abs(), None if b is None else b.abs(), padding=pad)
    n = (w.size(0) if transposed else w.size(1)) * w.size(2) + (b is not None)
    return ref, S.sum_bound(mag, n)


def candidates(ref, sb, dtype):
    """what a correct kernel may hold after rounding ref (known to within sb) to the stored type"""
    if dtype == torch.float32:
        return [ref]
    lo, hi = q(ref - sb, dtype), q(ref + sb, dtype)
    return [lo] if torch.equal(lo, hi) else [lo, hi]


def acts_stage(x_in_stored, g, form):
    """(reference, slack) of the stored gate output from the stored x_in"""
    a, b = gate(x_in_stored, g)
    ref = torch.tanh(a) * torch.sigmoid(b)
    return ref, S.slack_of(gate_form(x_in_stored, g, form, torch.float32), ref)


def dxin_stage(x_in, g, dacts_cands, form, with_dg=True):
    """from the candidates of the 16-bit dacts: candidate references of dx_in with their slack, and the two ends of dg with
    its bound: sum_bound over the T positions + the float32 yardstick of the whole sum"""
    refs, slack = [], 0.0
    for d in dacts_cands:
        da, db = gate_grads(x_in, g, d)
        da32, db32 = gate_grads_form(x_in, g, d, form, torch.float32)
        refs.append(torch.cat([da, db], 1))
        slack = max(slack, S.slack_of(torch.cat([da32, db32], 1), refs[-1]))
    dg = dg_bound = None
    if with_dg and g is not None:
        T = x_in.size(2)
        lo, hi = torch.minimum(refs[0], refs[-1]), torch.maximum(refs[0], refs[-1])
        dg = [lo.sum(2), hi.sum(2)]            # every position rounds its dacts on its own: the sums of the ends
        dg32 = torch.cat(gate_grads_form(x_in, g, dacts_cands[0], form, torch.float32), 1).sum(2)
        dg_bound = S.sum_bound(torch.maximum(lo.abs(), hi.abs()).sum(2), T) + S.slack_of(dg32, refs[0].sum(2))
    return refs, slack, dg, dg_bound


def judge(got, refs, dtype, slack):
    """(excess, ratio) of one output: S.elementwise_excess against, per element, the admissible reference nearest to what
    the kernel stored (`refs`: one reference, or the two ends of `candidates`; passes when <= 0), and the largest
    |error| / bound (what the mutation checks state their factor in)"""
    got = got.to(F64)
    if got.numel() == 0:
        return 0.0, 0.0
    lo, hi = refs[0], refs[0]
    for r in refs[1:]:
        lo, hi = torch.minimum(lo, r), torch.maximum(hi, r)
    ref = torch.minimum(torch.maximum(got, lo), hi)         # one reference: itself; two: the nearest point of their range
    err = (got - ref).abs()
    bound = S.round_bound(ref, dtype) * (1 + 2.0 ** -10) + slack
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return S.elementwise_excess(got, ref, dtype, slack), float(ratio.max())


def fwd_checks(p, lens, last, dtype, got, form):
    """every forward output of one path against its staged reference.  got: x_in, acts, x_out, acc_out as float64
    [B, C, T], and rs where the path stores it (the four launches).  name -> (excess, ratio)"""
    out = {}
    ref, sb = conv_stage(p["x"], p["w_in"], p["b_in"], pad=PAD)
    out["x_in"] = judge(got["x_in"], [ref], dtype, sb)
    ref, slack = acts_stage(got["x_in"], p["g"], form)
    out["acts"] = judge(got["acts"], [ref], dtype, slack)
    ref, sb = conv_stage(got["acts"], p["w_rs"], p["b_rs"])
    if got.get("rs") is not None:
        out["rs"] = judge(got["rs"], [ref], dtype, sb)
        cands = [got["rs"]]
    else:
        cands = candidates(ref, sb, dtype)
    tails = [tail(p["x"], p["acc"], c, lens, last) for c in cands]
    mag = cands[0].abs().amax() + p["x"].abs().amax() + (0.0 if p["acc"] is None else p["acc"].abs().amax())
    sb = S.sum_bound(float(mag), 2)            # one fp32 addition of two stored numbers
    if not last:
        out["x_out"] = judge(got["x_out"], [t[0] for t in tails], dtype, sb)
    out["acc_out"] = judge(got["acc_out"], [t[1] for t in tails], dtype, sb)
    return out


def bwd_checks(p, lens, last, dtype, got, form, add_after_rounding=False):
    """the same for the data half of the backward.  got: drs, dx_in, dx, dg (None without g), and dacts where stored.
    add_after_rounding: the path adds dx_next * mask as an epilogue of its backward-data launch, which some of the
    convolution kernels do in fp32 before the one rounding (as wn_layer_bwd does) and the tiled ones after rounding the
    convolution's result to the stored type (conv_grouped.hip: dx = T(float(T(conv)) + float(dx_add))); both are the
    arithmetic of "a convolution, then an addition", so dx is judged against the range the two span"""
    out = {}
    drs = drs_of(p["dx_next"], p["dacc"], lens, last)
    d = float((got["drs"].to(F64) - drs).abs().max()) if drs.numel() else 0.0
    out["drs"] = (d, float("inf") if d > 0 else 0.0)             # a masked copy: equal
    ref, sb = conv_stage(got["drs"], p["w_rs"], None, transposed=True)
    if got.get("dacts") is not None:
        out["dacts"] = judge(got["dacts"], [ref], dtype, sb)
        cands = [got["dacts"]]
    else:
        cands = candidates(ref, sb, dtype)
    refs, slack, dg, dg_bound = dxin_stage(p["x_in"], p["g"], cands, form, with_dg=got.get("dg") is not None)
    out["dx_in"] = judge(got["dx_in"], refs, dtype, slack)
    if got.get("dg") is not None:
        out["dg"] = judge(got["dg"], dg, torch.float32, dg_bound)
    ref, sb = conv_stage(got["dx_in"], p["w_in"], None, transposed=True, pad=PAD)
    refs = [ref]
    if not last:
        if add_after_rounding and dtype != torch.float32:
            refs += [q(c, dtype) for c in candidates(ref, sb, dtype)]
        sb = sb + S.sum_bound(drs[:, :H].abs() + ref.abs(), 1)
        refs = [r + drs[:, :H] for r in refs]
    out["dx"] = judge(got["dx"], refs, dtype, sb)
    return out


# ---- tolerance-regime operands -------------------------------------------------------------------------------------------------
def _rn(shape, g, scale, dtype):
    return q(torch.randn(shape, generator=g, dtype=F64) * scale, dtype)


def tol_fwd_inputs(shape, role, dtype):
    """randn operands rounded to `dtype` (the fp32 runs take the bfloat16 operands: every product is then exact in fp32)"""
    B, T, _lens = shape
    name, last, with_g, with_acc = role
    g_ = X.gen("wn_tol_fwd", B, T, name, str(dtype))
    rs_c = H if last else 2 * H
    return dict(w_in=_rn((2 * H, H, K), g_, (H * K) ** -0.5, dtype), w_rs=_rn((rs_c, H, 1), g_, 2.0 * H ** -0.5, dtype),
                b_in=torch.randn(2 * H, generator=g_).double() * 0.05, b_rs=torch.randn(rs_c, generator=g_).double() * 0.05,
                x=_rn((B, H, T), g_, 1.0, dtype), g=_rn((B, 2 * H), g_, 0.5, dtype) if with_g else None,
                acc=_rn((B, H, T), g_, 1.0, dtype) if with_acc else None)


def tol_bwd_inputs(shape, role, dtype):
    B, T, _lens = shape
    name, last, with_g, with_dx = role
    g_ = X.gen("wn_tol_bwd", B, T, name, str(dtype))
    rs_c = H if last else 2 * H
    return dict(w_in=_rn((2 * H, H, K), g_, (H * K) ** -0.5, dtype), w_rs=_rn((rs_c, H, 1), g_, 2.0 * H ** -0.5, dtype),
                x_in=_rn((B, 2 * H, T), g_, 1.0, dtype), g=_rn((B, 2 * H), g_, 0.5, dtype) if with_g else None,
                dacc=_rn((B, H, T), g_, 1.0, dtype),
                dx_next=_rn((B, H, T), g_, 1.0, dtype) if (with_dx and not last) else None)


# ---- gate sweep ------------------------------------------------------------------------------------------------------------------
def sweep_values(dtype):
    """every finite value of the 16-bit type with 2^-20 (bfloat16) / the smallest subnormal (IEEE half) <= |v| <= 2^7, both
    signs, and 0, +-512; padded with zeros to whole rows of H"""
    if dtype == torch.bfloat16:
        lo, hi = 0x3580, 0x4300          # 2^-20 .. 2^7
    else:
        lo, hi = 0x0001, 0x5800          # 2^-24 .. 2^7
    bits = torch.arange(lo, hi + 1, dtype=torch.int32)
    pos = bits.to(torch.int16).view(dtype).to(F64)
    v = torch.cat([torch.tensor([0.0, SAT, -SAT], dtype=F64), pos, -pos])
    pad = (-v.numel()) % H
    return torch.cat([v, torch.zeros(pad, dtype=F64)]).view(-1, H)


def spacing(ref, dtype):
    """distance between neighbouring values of the stored type at ref (2 x S.round_bound)"""
    ref = ref.to(F64).abs()
    if dtype == torch.float16:
        e = torch.floor(torch.log2(torch.clamp(ref, min=2.0 ** -14)))
        return torch.exp2(e - 10)
    e = torch.floor(torch.log2(torch.clamp(ref, min=2.0 ** -126)))
    return torch.exp2(e - 7)
