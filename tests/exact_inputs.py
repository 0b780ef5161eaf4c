"""Integer-exact operands, float64 references and the bit-for-bit comparator of tests/test_exact_int_gpu.py (and of its
CPU-side conditions, tests/test_exact_inputs_cpu.py).

The convolution, residual-unit and GEMM kernels are multiply-accumulate with fp32 accumulators.  With small-integer
operands every product and every partial sum is an integer multiple of one fixed step (1, 0.5 or 0.25) far below 2^24
steps, so fp32 accumulation is exact in ANY order -- split-K, slabs, atomics and stream placement drop out -- and where
every stored value also fits the storage type (at most 256 steps for bfloat16, 2048 for IEEE half) the kernel has to
reproduce a float64 reference bit for bit.  This module has no code in common with the library or with oracle/ops.py: the
references are torch.nn.functional.conv1d / conv_transpose1d / linear differentiated by autograd on the CPU.

Values (one generator per operand role, seeded per case):
  weights      dense, never zero, from {+-1, +-2}: a dropped product cannot hide behind a zero weight
  weight_g     sqrt(sum v^2) per output row, so that g / sqrtf(ss) is exactly 1 and the folded image is v itself
  x, dy        from {+-1, +-2} (zero elsewhere), with a density of `budget / reduction length`: the variance of a sum of T
               products is known, and T is chosen so that 256 steps are 6.5 to 8 standard deviations (the budgets below)
  bias, res    small integers
  slopes       powers of two (0.5, 0.25): multiplying by them only moves the exponent
  dy2          dense +-1 for the second backward pass that judges dW / db alone (fp32, exact below 2^24)
"""
import torch
import torch.nn.functional as F

LIMIT_STEPS = {torch.bfloat16: 256, torch.float16: 2048}    # integers a 16-bit significand holds without rounding
F32_EXACT = float(1 << 24)

# conv fusions: (in_slope, out_act, out_slope, res) as tests/test_conv_gpu.py::FUSIONS, with power-of-two slopes and without tanh
#   step   the smallest step a stored value of the case is a multiple of
#   tx/tdy non-zero products per output element of the forward / of backward-data.  In steps, one product w * x has the
#          second moment  2.5 * 6.25 (plain: w, x from {1, 2}),  2.5 * 6.25 on x in {2, 4, -1, -2} half-steps (in_slope),
#          2.5 * 2.5 * 16 quarter-steps (out_slope 0.25), so sigma = 2.5 sqrt(T), 3.95 sqrt(T), 10 sqrt(T); backward-data sees
#          dy * act' instead of x: 2.5 sqrt(T), 5 sqrt(T), 7.3 sqrt(T).  The budgets put 256 steps at 6.5 sigma or more;
#          tests/test_exact_inputs_cpu.py then checks the condition itself on every element of every case.
FUSIONS = [
    dict(name="plain", in_slope=1.0, out_act=0, out_slope=1.0, res=False, step=1.0, tx=160, tdy=160),
    dict(name="slope_res", in_slope=0.5, out_act=0, out_slope=1.0, res=True, step=0.5, tx=64, tdy=40),
    dict(name="lrelu_out", in_slope=1.0, out_act=1, out_slope=0.25, res=False, step=0.25, tx=12, tdy=16),
]


def gen(*key):
    """a torch.Generator seeded from the case (hash() of a tuple of numbers / strings is not stable across processes)"""
    s = 0
    for part in key:
        for ch in repr(part):
            s = (s * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(s)


def dense_pm(shape, g, mags=(1, 2)):
    """dense, never zero: uniform over {+-m for m in mags}"""
    m = torch.tensor(mags, dtype=torch.float64)[torch.randint(0, len(mags), shape, generator=g)]
    return m * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def sparse_pm(shape, g, density, mags=(1, 2)):
    """{+-m} with probability `density`, zero elsewhere"""
    keep = torch.rand(shape, generator=g, dtype=torch.float64) < density
    return dense_pm(shape, g, mags) * keep


def small_int(shape, g, hi=2):
    return torch.randint(-hi, hi + 1, shape, generator=g).double()


def weight_g_of(v):
    """weight_g that folds to w = v: the fp32 square root of the (exact) fp32 sum of squares of each row"""
    ss = (v.float() ** 2).reshape(v.size(0), -1).sum(1)
    return torch.sqrt(ss).reshape((v.size(0),) + (1,) * (v.dim() - 1))


def assert_lrelu_zero_convention(slope=0.5):
    """the kernels take act' = (stored activation > 0 ? 1 : slope); torch's leaky_relu_backward does the same AT zero, which
    is what lets the sparse operands (mostly zeros) go unmasked"""
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.leaky_relu(z, slope).sum(), z)
    assert torch.equal(g, torch.full_like(g, slope)), g


def _reductions(case):
    cin, cout, k, stride, pad, dil, groups, transposed = case[:8]
    taps = -(-k // stride)
    if transposed:
        return cin * taps, cout * k
    return cin // groups * k, cout // groups * taps


def conv_inputs(case, fusion):
    """operands of one convolution case (reference layout [nseq, C, L], float64).  `case` as in tests/test_conv_gpu.py:
    (cin, cout, k, stride, pad, dil, groups, transposed, wn, L, nseq)"""
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    g = gen("conv", case, fusion["name"])
    red_f, red_b = _reductions(case)
    wshape = (cin, cout // groups, k) if transposed else (cout, cin // groups, k)
    lout = conv_lout(case)
    has_bias = cout != 1 or wn
    has_res = fusion["res"] and not transposed
    return dict(
        w=dense_pm(wshape, g),
        bias=small_int((cout,), g) if has_bias else None,
        x=sparse_pm((nseq, cin, lin), g, min(1.0, fusion["tx"] / red_f)),
        res=small_int((nseq, cout, lout), g) if has_res else None,
        dy=sparse_pm((nseq, cout, lout), g, min(1.0, fusion["tdy"] / red_b)),
        dy2=dense_pm((nseq, cout, lout), g, (1,)),
    )


def conv_lout(case):
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    if transposed:
        return (lin - 1) * stride - 2 * pad + dil * (k - 1) + 1
    return (lin + 2 * pad - dil * (k - 1) - 1) // stride + 1


def heavy(case):
    """the 1024-channel layers and the large GEMMs: their CPU reference runs in fp32, which is as exact as float64 for
    these operands (every partial sum is an integer multiple of the step below 2^24 steps) and several times faster"""
    cin, cout, k, stride, pad, dil, groups, transposed, wn, lin, nseq = case
    return cin * cout * k // groups * nseq * lin >= 1 << 31


def conv_forward(inp, case, fusion, w=None, x=None):
    cin, cout, k, stride, pad, dil, groups, transposed = case[:8]
    w = inp["w"] if w is None else w
    x = inp["x"] if x is None else x
    xa = F.leaky_relu(x, fusion["in_slope"]) if fusion["in_slope"] != 1.0 else x
    if transposed:
        z = F.conv_transpose1d(xa, w, inp["bias"], stride=stride, padding=pad, dilation=dil, groups=groups)
    else:
        z = F.conv1d(xa, w, inp["bias"], stride=stride, padding=pad, dilation=dil, groups=groups)
    y = F.leaky_relu(z, fusion["out_slope"]) if fusion["out_act"] == 1 else z
    return y + inp["res"] if inp["res"] is not None else y


def conv_reference(inp, case, fusion, weight_grads=True):
    """y, and from the pass with the sparse dy: dx, dres, dW, db; from the pass with the dense +-1 dy2: dW2, db2 (the
    second pass differentiates with respect to the parameters only).  weight_grads=False: y, dx and dres alone."""
    assert_lrelu_zero_convention(fusion["in_slope"] if fusion["in_slope"] != 1.0 else fusion["out_slope"])
    dt = torch.float32 if heavy(case) else torch.float64
    c = {k_: (v.to(dt) if v is not None else None) for k_, v in inp.items()}
    leaves = {k_: c[k_].clone().requires_grad_(True) for k_ in ("x", "w", "bias", "res") if c[k_] is not None}
    c.update(leaves)
    y = conv_forward(c, case, fusion)
    names = list(leaves)
    if not weight_grads:
        names = [n for n in names if n in ("x", "res")]
    g1 = dict(zip(names, torch.autograd.grad(y, [leaves[n] for n in names], c["dy"], retain_graph=weight_grads)))
    g2 = {}
    if weight_grads:
        pn = [n for n in names if n in ("w", "bias")]
        g2 = dict(zip(pn, torch.autograd.grad(y, [leaves[n] for n in pn], c["dy2"])))
    out = dict(y=y.detach(), dx=g1["x"], dW=g1.get("w"), dW2=g2.get("w"), db=g1.get("bias"), db2=g2.get("bias"),
               dres=g1.get("res"))
    return {k_: (v.double() if v is not None else None) for k_, v in out.items()}


# ---- residual unit  y = x + c2(lrelu(c1(lrelu(x)))) --------------------------------------------------------------------
#
# Two dense convolutions in a row: ONE non-zero x makes the mid activation non-zero on all C channels at k positions d
# apart, and y a sum of C * ceil(k / d) products, none of them zero (the weights are dense).  In quarter-steps (slope 0.5
# twice) a product of +-1 operands is one of {4, -2, 2, -1}, so that sum has sigma = 2.5 sqrt(C ceil(k / d)) steps whatever
# the density -- and sqrt(2.5) = 1.6 times that per {+-1, +-2} operand.  Hence:
#   * the operands are impulses on a lattice: one channel per position, positions one two-convolution receptive field
#     d (k - 1) + k apart (two impulses that share a receptive field double the variance), the first and the last
#     position of every sequence among them (the sequence boundary is where taps get lost);
#   * weights, x and dy are from {+-1}, the subset of the value sets a chain of two dense layers leaves room for;
#   * b1 has ONE non-zero channel, -1 (a dense b1 makes the mid activation dense); b2 is dense;
#   * bfloat16 (256 steps = 6.4 sigma) holds the result where C ceil(k / d) <= 256; the wider / denser units run in the
#     IEEE-half build alone (2048 steps: 6.4 sigma up to C ceil(k / d) = 16384), which compiles the same kernel sources.
#     The rule is fixed here, from the formats; tests/test_exact_inputs_cpu.py checks every element against it.
def resunit_dtypes(C, k, d):
    """names of the 16-bit builds a residual-unit case is exact in"""
    return ("f16", "bf16") if C * -(-k // d) <= 256 else ("f16",)


def stage_dtypes(C, ks=(3, 7, 11), ds=(1, 3, 5)):
    """a stage output is the sum of its three units: the variances add"""
    return ("f16", "bf16") if C * sum(-(-k // d) for k, d in zip(ks, ds)) <= 256 else ("f16",)


def resunit_dense_judges_first(C, k, dtype_name):
    """does the dense +-1 pass judge the FIRST convolution's dW / db as well?  They are sums over dmid, which the backward
    stores in 16 bits: under a dense dy it is a sum of C k half-steps (sigma = 2 sqrt(C k) quarter-steps)"""
    return dtype_name == "f16" or C * k <= 256


def resunit_mags(C):
    """(magnitudes of w1, of w2, of x and dy): see above"""
    return (1,), (1,), (1,)


def _lattice(shape, g, spacing, mags):
    nseq, C, L = shape
    t = torch.zeros(shape, dtype=torch.float64)
    for s in range(nseq):
        # even sequences start their lattice at position 0, odd ones at a random offset; every sequence ends with L - 1
        off = int(torch.randint(1, spacing, (1,), generator=g)) if s % 2 else 0
        pos = [p for p in range(off, L, spacing) if p + spacing <= L - 1] + [L - 1]
        for p in pos:
            t[s, int(torch.randint(0, C, (1,), generator=g)), p] = dense_pm((1,), g, mags)[0]
    return t


def resunit_inputs(C, k, d, L, nseq, tag="unit", spacing=None):
    g = gen("resunit", tag, C, k, d, L, nseq)
    w1m, w2m, xm = resunit_mags(C)
    spacing = d * (k - 1) + (k - 1) + 1 if spacing is None else spacing
    b1 = torch.zeros(C, dtype=torch.float64)
    b1[int(torch.randint(0, C, (1,), generator=g))] = -1.0      # negative: the second leaky-relu halves it (a background of 2 k quarter-steps)
    return dict(w1=dense_pm((C, C, k), g, w1m), w2=dense_pm((C, C, k), g, w2m), b1=b1, b2=small_int((C,), g, 1),
                x=_lattice((nseq, C, L), g, spacing, xm), dy=_lattice((nseq, C, L), g, spacing, xm),
                dy2=dense_pm((nseq, C, L), g, (1,)))


def resunit_forward(c, k, d, slope, x=None):
    x = c["x"] if x is None else x
    xa = F.leaky_relu(x, slope)
    mid_a = F.leaky_relu(F.conv1d(xa, c["w1"], c["b1"], padding=(k * d - d) // 2, dilation=d), slope)
    return xa, mid_a, F.conv1d(mid_a, c["w2"], c["b2"], padding=(k - 1) // 2) + x


def resunit_reference(inp, k, d, slope=0.5, dy_scale=1.0):
    """xa, mid_a, y; sparse pass: dx, dmid (the gradient at c1's output, before its activation: a stored 16-bit
    intermediate of the backward), dW1, dW2, db1, db2; dense pass: the same with a trailing 2"""
    assert_lrelu_zero_convention(slope)
    c = {k_: v.clone() for k_, v in inp.items()}
    names = ("x", "w1", "w2", "b1", "b2")
    for n in names:
        c[n].requires_grad_(True)
    xa = F.leaky_relu(c["x"], slope)
    pre = F.conv1d(xa, c["w1"], c["b1"], padding=(k * d - d) // 2, dilation=d)
    mid_a = F.leaky_relu(pre, slope)
    y = F.conv1d(mid_a, c["w2"], c["b2"], padding=(k - 1) // 2) + c["x"]
    out = dict(xa=xa.detach(), mid_a=mid_a.detach(), y=y.detach())
    for sfx, dy in (("", c["dy"]), ("2", c["dy2"])):
        gs = torch.autograd.grad(y, [c[n] for n in names] + [pre], dy * dy_scale, retain_graph=True)
        for n, g_ in zip(("dx", "dW1", "dW2", "db1", "db2", "dmid"), gs):
            out[n + sfx] = g_
    return out


def stage_inputs(C, L, nseq, ks=(3, 7, 11), ds=(1, 3, 5)):
    """one vocoder stage of three one-unit blocks (kernel sizes 3 / 7 / 11) on ONE input: the grouped launches.  A chain of
    units multiplies the step by four per unit (two leaky-relus), so three chained units leave the 16-bit significand
    whatever the operands; the chaining itself stays with the tolerance tests."""
    spacing = max(d * (k - 1) + k for k, d in zip(ks, ds))       # the widest unit's receptive field
    units = [resunit_inputs(C, k, d, L, nseq, tag="stage", spacing=spacing) for k, d in zip(ks, ds)]
    for u in units[1:]:
        u["x"], u["dy"], u["dy2"] = units[0]["x"], units[0]["dy"], units[0]["dy2"]
    return units


def stage_reference(units, ks, ds, slope, scale):
    """out = scale * sum_j unit_j(x); dx of the stage; per unit its resunit_reference with dy_scale = scale"""
    refs = [resunit_reference(u, k, d, slope, scale) for u, k, d in zip(units, ks, ds)]
    out = dict(y=scale * sum(r["y"] for r in refs), dx=sum(r["dx"] for r in refs), units=refs)
    return out


# ---- dense GEMM  y = x W^T + b  (a 1 x 1 convolution over the rows) ------------------------------------------------------
def gemm_as_conv(M, N, K):
    return (K, N, 1, 1, 0, 1, 1, False, False, M, 1)


GEMM_T = 40      # products per output element: sigma = 2.5 sqrt(40) = 16 steps; the dropout keep-scale of 2 and the gate's
#                  gate_pos of 2 double a stored value, which leaves 256 steps at 8 sigma


def gemm_inputs(M, N, K, has_bias, tag="gemm"):
    """x [M, K], w [N, K], bias [N], dy [M, N] (sparse, for backward-data) and dy2 (dense +-1, for dW / db)"""
    g = gen(tag, M, N, K, has_bias)
    return dict(w=dense_pm((N, K), g), bias=small_int((N,), g) if has_bias else None,
                x=sparse_pm((M, K), g, min(1.0, GEMM_T / K)), dy=sparse_pm((M, N), g, min(1.0, GEMM_T / N)),
                dy2=dense_pm((M, N), g, (1,)))


def gemm_epilogue_operands(M, N, K):
    """the fused epilogues' operands: `add_n` [M, N] for the forward add, `add_k` [M, K] and `gate` [M, K] (a saved relu +
    dropout activation: zero or positive) for backward-data"""
    g = gen("gemm_epi", M, N, K)
    return dict(add_n=small_int((M, N), g), add_k=small_int((M, K), g), gate=small_int((M, K), g).clamp(min=0))


def gemm256_shapes():
    """the shapes of tests/test_gemm_gpu.py::test_gemm256_fused_epilogues, read off its parametrisation"""
    import test_gemm_gpu as TG

    marks = [m for m in TG.test_gemm256_fused_epilogues.pytestmark if m.name == "parametrize"]
    return [tuple(s_) for s_ in marks[0].args[1]]


def gemm_reference(inp, relu=False):
    dt = torch.float32 if inp["x"].size(0) * inp["w"].numel() >= 1 << 31 else torch.float64
    x = inp["x"].to(dt).clone().requires_grad_(True)
    w = inp["w"].to(dt).clone().requires_grad_(True)
    b = inp["bias"].to(dt).clone().requires_grad_(True) if inp["bias"] is not None else None
    z = F.linear(x, w, b)
    y = F.relu(z) if relu else z
    leaves = [x, w] + ([b] if b is not None else [])
    g1 = torch.autograd.grad(y, leaves, inp["dy"].to(dt), retain_graph=True)
    g2 = torch.autograd.grad(y, leaves, inp["dy2"].to(dt))
    out = dict(z=z.detach(), y=y.detach(), dx=g1[0], dW=g1[1], dW2=g2[1], db=g1[2] if b is not None else None,
               db2=g2[2] if b is not None else None)
    return {k_: (v.double() if v is not None else None) for k_, v in out.items()}


# ---- conditions -----------------------------------------------------------------------------------------------------------
def steps_of(t, step):
    """(every element an integer multiple of `step`?, the largest magnitude in steps)"""
    q = t.double() / step
    return bool(torch.equal(q, q.round())), float(q.abs().max()) if q.numel() else 0.0


def check_stored(named, step, limit=LIMIT_STEPS[torch.bfloat16]):
    """every stored tensor: integer multiples of `step`, at most `limit` steps -- a condition on ALL elements.  Returns the
    largest magnitude in steps."""
    worst = 0.0
    for name, t in named.items():
        if t is None:
            continue
        ok, m = steps_of(t, step)
        assert ok, f"{name}: not a multiple of {step}"
        assert m <= limit, f"{name}: {m} steps of {step} (limit {limit}): lower this case's density"
        worst = max(worst, m)
    return worst


def check_f32(named):
    worst = 0.0
    for name, t in named.items():
        if t is None:
            continue
        m = float(t.abs().max())
        assert m < F32_EXACT, f"{name}: |sum| {m} is not below 2^24"
        worst = max(worst, m)
    return worst


# ---- comparator -----------------------------------------------------------------------------------------------------------
def assert_exact(got, want, dtype, name, nlc=True, context=""):
    """torch.equal(got, want cast to the storage type).  `got`: what the kernel stored (activations channels-last
    [nseq, L, C] when nlc, else any layout equal to the reference's); `want`: the reference ([nseq, C, L] for activations).
    A failure names the edge: how many elements differ, the first few as (sequence, position, channel) and the tile
    coordinates they imply."""
    want = want.detach()
    if nlc and want.dim() == 3:
        want = want.transpose(1, 2)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f"{name}: shape {tuple(got.shape)} against {tuple(want.shape)} {context}"
    want = want.contiguous().to(dtype)
    got = got.contiguous()
    assert got.dtype == dtype, f"{name}: stored as {got.dtype}, expected {dtype} {context}"
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))
    lines = []
    for idx in bad[:8].tolist():
        t = tuple(idx)
        where = f"{t}"
        if nlc and len(t) == 3:
            s, p, c = t
            where = f"(seq {s}, pos {p}, ch {c}) [pos%64={p % 64} pos%128={p % 128} ch%32={c % 32}]"
        lines.append(f"  {where}: got {float(got[t])!r} want {float(want[t])!r}")
    raise AssertionError(f"{name}: {bad.size(0)} of {got.numel()} elements differ {context}\n" + "\n".join(lines))


# ---- case lists -----------------------------------------------------------------------------------------------------------
# the edge sweep of every fast path: L at tile - 1 / tile / tile + 1 of the path's position tile, L shorter than the
# receptive field dil (k - 1) + 1, one sequence, a position count that is not a multiple of 16, stride 3 with lout on a tile
# boundary; sized so that the dispatcher keeps each case on its path (conv_deep.hip::deep_kind: 192 tiles of 128 x 128, else
# 32 tiles of 64 x 64; conv_narrow.hip::narrow_eligible: 4096 positions; rows_gemm.hip: at most 16 rows)
_D = (256, 256, 3, 1, 1, 1, 1, False, True)          # conv_deep both ways: 2 channel tiles x 96+ position tiles of 128
_R = (192, 384, 5, 1, 2, 1, 1, False, True)          # conv_ring: 6 channel tiles x 16 position tiles of 64
_N = (16, 16, 7, 1, 9, 3, 1, False, True)            # conv_narrow: 64-position regions
_I = (64, 64, 5, 1, 2, 1, 1, False, True)            # conv_igemm: too few tiles for the ring
EDGE_CASES = {
    "edge_deep": [
        _D + (127, 98), _D + (128, 96), _D + (129, 96),
        _D + (2, 6200),                                      # L < receptive field (3)
        _D + (12400, 1),                                     # one sequence
        _D + (127, 99),                                      # 12573 positions: not a multiple of 16
        (256, 256, 5, 3, 2, 1, 1, False, True, 384, 96),     # stride 3, lout = 128
    ],
    # DiscriminatorP at period 7: 224 sequences of 37 -- forward and backward-data (the geometry, with 90 sequences and its
    # weight gradients, is DEEP_CASES[1])
    "edge_p7": [(1024, 1024, 5, 1, 2, 1, 1, False, True, 37, 224)],
    "edge_ring": [
        _R + (63, 16), _R + (64, 16), _R + (65, 16),
        _R + (3, 400),                                       # L < receptive field (5)
        _R + (1000, 1),
        _R + (63, 15),                                       # 945 positions
        (128, 64, 5, 3, 2, 1, 1, False, True, 192, 40),      # stride 3, lout = 64
    ],
    "edge_narrow": [
        _N + (63, 66), _N + (64, 66), _N + (65, 66),
        _N + (10, 420),                                      # L < receptive field (19)
        _N + (4100, 1),
        _N + (63, 67),                                       # 4221 positions
        (32, 32, 3, 1, 1, 1, 1, False, True, 65, 64),        # (the narrow kernel has no strided form)
    ],
    "edge_halo": [       # (wgrad_halo.hip::wgrad_halo_eligible: sequence-local 64-position stages, at most 30 % of them padding)
        (64, 64, 7, 1, 3, 1, 1, False, True, 255, 6), (64, 64, 7, 1, 3, 1, 1, False, True, 256, 6),
        (64, 64, 7, 1, 3, 1, 1, False, True, 257, 6), (64, 64, 7, 1, 3, 1, 1, False, True, 1153, 1),
        (64, 64, 7, 1, 3, 1, 1, False, True, 191, 6),
    ],
    "edge_rows16": [
        (512, 512, 1, 1, 0, 1, 1, False, False, 1, 1), (512, 1536, 1, 1, 0, 1, 1, False, True, 15, 1),
        (512, 512, 1, 1, 0, 1, 1, False, False, 16, 1),
    ],
    # one output channel with 5 taps / dilated / strided: the generic cout1_bwd_weight (tests/test_conv_gpu.py::CASES has
    # k = 3 and 7 at stride 1 only, which all take the x-stationary form)
    "edge_small": [
        (32, 1, 5, 1, 2, 1, 1, False, True, 90, 3), (16, 1, 7, 1, 9, 3, 1, False, True, 130, 2),
        (64, 1, 3, 2, 1, 1, 1, False, True, 81, 3),
    ],
    "edge_igemm": [
        _I + (63, 3), _I + (64, 3), _I + (65, 3),
        _I + (3, 5),                                         # L < receptive field (5)
        _I + (100, 1),
        _I + (61, 3),                                        # 183 positions
        (128, 64, 5, 3, 2, 1, 1, False, True, 192, 2),       # stride 3, lout = 64
    ],
}
FULL_CROSS = ("cases", "edge_igemm", "edge_rows16", "edge_small")     # every dtype x both impl; the large lists: conv_runs()
LIGHT = ("edge_p7",)                                                  # y, dx and dres alone: no weight-gradient pass


def conv_case_lists():
    """name -> list of case tuples: the six lists of tests/test_conv_gpu.py (imported, not copied) and the edge sweep"""
    import test_conv_gpu as TC

    lists = dict(cases=TC.CASES, deep=TC.DEEP_CASES, ring=TC.RING_CASES, narrow=TC.NARROW_CASES, ups=TC.UPS_CASES,
                 halo=TC.HALO_CASES)
    lists.update(EDGE_CASES)
    return lists


def conv_case_ids():
    return [(name, i) for name, cs in conv_case_lists().items() for i in range(len(cs))]


def conv_runs(name):
    """(dtype name, impl) combinations a list runs with: the small lists take all six; the large ones (sized to fill the
    chip for one fast path) run that path in the three types -- the naive kernels have no tiles for a size to matter to"""
    if name in FULL_CROSS:
        return [(d, i) for d in ("bf16", "f16", "f32") for i in ("auto", "naive")]
    if name in LIGHT:
        return [("bf16", "auto"), ("f16", "auto")]
    return [("bf16", "auto"), ("f16", "auto"), ("f32", "auto")]


def conv_fusions(case):
    """the three fusions; a transposed convolution takes no residual (as in tests/test_conv_gpu.py)"""
    return FUSIONS


# residual units: (C, k, d, L) -- the existing tests' ragged lengths plus tile +- 1 (64-position tiles).  The fused kernels
# take L >= 64 (resunit.hip::job_ok, resunit_wide.hip::wide_ok): L = 63 is res_unit's composition of single launches.
RESUNIT_CASES = sorted({(C, k, d, L) for C in (16, 32, 64, 128, 256) for (k, d, L) in
                        [(3, 1, 200), (3, 5, 1000), (7, 3, 64), (7, 5, 129), (11, 1, 130), (11, 5, 777), (3, 3, 63),
                         (7, 1, 65), (11, 3, 127), (7, 1, 333)]})
RESUNIT_NSEQ = 4
STAGE_CASES = [(16, 333), (32, 200), (16, 64), (32, 129), (16, 127), (32, 65)]     # (C, L)
STAGE_KS, STAGE_DS = (3, 7, 11), (1, 3, 5)

# dense GEMMs: tests/test_gemm_gpu.py::CASES and the shapes of test_gemm256_fused_epilogues are imported there
DEC_SHAPES = [(1025, 512), (1536, 512), (512, 2048)]      # (N, K) of evt_dec_gemv / evt_dec_gemm_rows; logits first
DEC_ROWS = (1, 4, 5, 32)


def tag_head(tag):
    """"conv_ring<bf16, 64, 64, 64, x4>" -> "conv_ring": what the static guard and the recorded expectations key on"""
    return tag.split("<")[0].split(" ")[0]
