"""References, bounds and inputs of tests/test_s1_ops_gpu.py (and of their CPU-side conditions, tests/test_s1_refs_cpu.py)
for the s1 training kernels of csrc/s1_ops.hip: fused add + LayerNorm, cross-entropy with gradient and top-k hits, and the
two ScaledAdam launches.  Nothing here touches a GPU or the library's kernels.

Every reference is the arithmetic the kernel states, in plain torch ops, with a `dtype` argument: run in float64 on the
operands the kernel reads (converted exactly) it is the reference; run in float32 it is the yardstick -- how far a careful
fp32 evaluation of the same formula lands from the float64 one.  The element-wise tolerances of the GPU tests are tied to
that yardstick (4 x its largest deviation, `slack`), never to the kernel's own numbers.

Bounds.
  round_bound(ref, dtype)   half the spacing of the stored type at ref: what the final rounding of a correct fp32 value adds.
  sum_bound(abs_sum, depth) worst-case forward error of an fp32 sum whose longest chain of dependent additions is `depth`:
                            every addition rounds by at most 2^-24 relative to a partial sum that is at most abs_sum, so the
                            chain adds at most depth * 2^-24 * abs_sum (first order); the 8 further units cover the second-order
                            terms and the final scaling (1/C, the stored fp32 result).  It is an upper bound for ANY order
                            of the same additions, so it cannot fail because threads, waves or atomics arrive differently;
                            a dropped or doubled addend moves the sum by a whole term (tests/test_s1_refs_cpu.py).
  depths are counted from the launch geometry of csrc/s1_ops.hip by ln_fwd_depth / ln_bwd_depth / ce_depth / sa_stats_depth.
"""
import math

import torch

U = 2.0 ** -24                      # fp32 unit round-off
F64 = torch.float64
EPS_LN = 1e-5


def gen(*key):
    """a torch.Generator seeded from the key (hash() of a tuple is not stable across processes)"""
    s = 0
    for part in key:
        for ch in repr(part):
            s = (s * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(s)


def stored(t, dtype):
    """what a kernel of that type reads: the value rounded to the stored type, as float32 (exact)"""
    return t.to(dtype).float()


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def round_bound(ref, dtype):
    """half the spacing of `dtype` at ref: bf16 has 8 significand bits (spacing <= 2^-7 |ref|), f16 has 11 (spacing
    <= 2^-10 |ref|, and 2^-24 below its smallest normal 2^-14); fp32 results are compared to the fp32 yardstick alone"""
    ref = ref.to(F64).abs()
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    if dtype == torch.bfloat16:
        return ref * 2.0 ** -8
    if dtype == torch.float16:
        return torch.clamp(ref * 2.0 ** -11, min=2.0 ** -25)
    raise ValueError(dtype)


def sum_bound(abs_sum, depth):
    return (depth + 8) * U * abs_sum


def slack_of(run32, run64):
    """4 x the largest deviation of the fp32 evaluation of the reference formula from the float64 one: 1 covers what
    a correctly rounded fp32 evaluation does; the hardware's rsqrt / exp / log are about 1 ulp against the CPU's half, and the
    kernel's operation order differs"""
    return 4.0 * float((run32.to(F64) - run64.to(F64)).abs().max())


def elementwise_excess(got, ref, dtype, slack):
    """max over elements of |got - ref| - (round_bound(ref) * (1 + 2^-10) + slack): passes when <= 0"""
    got, ref = got.to(F64), ref.to(F64)
    return float(((got - ref).abs() - (round_bound(ref, dtype) * (1 + 2.0 ** -10) + slack)).max())


# ---- add + LayerNorm -------------------------------------------------------------------------------------------------------
LN_CS = (8, 72, 512, 520, 768, 1024)
LN_ROWS = (1, 3, 5, 67)
LN_FAMILIES = ("randn", "offset")


def ln_inputs(C, with_r, family, dtype):
    """max(LN_ROWS) rows; the smaller row counts run on the first rows of the same tensors.  Everything is rounded to the
    stored type (gamma / beta / the gradient accumulators are fp32 in every build).  Returns float32 tensors."""
    rows = max(LN_ROWS)
    g = gen("ln", C, family)
    if family == "randn":
        x, r = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g) * 0.5
    else:                                               # x + r ~ N(100, 1): a one-pass E[t^2] - E[t]^2 loses 13 of 24 bits
        if with_r:
            x = 60.0 + torch.randn(rows, C, generator=g) * 0.8
            r = 40.0 + torch.randn(rows, C, generator=g) * 0.6
        else:
            x, r = 100.0 + torch.randn(rows, C, generator=g), torch.zeros(rows, C)
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    pre_g = torch.randint(-16, 17, (C,), generator=g).float() / 8 + 0.125      # non-zero preloads of dgamma / dbeta
    pre_b = torch.randint(-16, 17, (C,), generator=g).float() / 8 - 0.125
    return dict(x=stored(x, dtype), r=stored(r, dtype) if with_r else None, gamma=gamma, beta=beta, dy=stored(dy, dtype),
                pre_g=pre_g, pre_b=pre_b)


def add_ln_ref(x, r, gamma, beta, eps, dtype=F64):
    """y, mean, rstd of LayerNorm(x + r) over the last dimension, two-pass variance (csrc/s1_ops.hip add_ln_fwd)"""
    t = x.to(dtype) + (r.to(dtype) if r is not None else 0)
    C = t.shape[-1]
    mean = t.sum(-1) / C
    d = t - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(-1) / C + eps)
    y = d * rstd[:, None] * gamma.to(dtype) + beta.to(dtype)
    return y, mean, rstd


def add_ln_bwd_ref(x, r, gamma, dy, mean, rstd, dtype=F64):
    """dxr, dgamma, dbeta and sum|term| per channel of dgamma / dbeta, from GIVEN statistics (add_ln_bwd)"""
    t = x.to(dtype) + (r.to(dtype) if r is not None else 0)
    C = t.shape[-1]
    d = dy.to(dtype)
    xh = (t - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    dh = d * gamma.to(dtype)
    s1 = dh.sum(-1, keepdim=True) / C
    s2 = (dh * xh).sum(-1, keepdim=True) / C
    dxr = rstd.to(dtype)[:, None] * (dh - s1 - xh * s2)
    tg = d * xh
    return dxr, tg.sum(0), d.sum(0), tg.abs().sum(0), d.abs().sum(0)


def ln_dgamma_term_error(x, r, dy, rstd, abs_terms):
    """per channel: what the fp32 evaluation of the terms dy * ((t - mean) * rstd) adds before any summation.  t = x + r rounds
    by u |t| (absolute; it survives the subtraction of the mean, so it is large where |t| >> |t - mean|), the subtraction and
    the two products by u each relative to the term: sum of |dy| rstd u |t| + 3 u |term|, taken as 4 u for the second order.
    (dbeta's terms are the stored dy themselves: no error of their own.)"""
    t = x.to(F64) + (r.to(F64) if r is not None else 0)
    d = dy.to(F64).abs()
    return (d * rstd.to(F64)[:, None] * U * t.abs()).sum(0) + 4 * U * abs_terms


def ln_np(C, dtype):
    """(lanes' channels per pass V, passes NP) of the instantiation evt_add_layernorm_* picks"""
    if dtype == torch.float32:
        return 4, (2 if C <= 512 else 4)
    return 8, (1 if C <= 512 else 2)


def ln_fwd_depth(C, dtype):
    """a lane adds its NP * V values, the wave butterfly adds 6 times"""
    V, NP = ln_np(C, dtype)
    return NP * V + 6


def ln_bwd_geometry(rows):
    rpb = max(16, (rows + 1023) // 1024)
    return rpb, (rows + rpb - 1) // rpb


def ln_bwd_depth(rows):
    """dgamma / dbeta: a wave adds rows_per_block / 4 rows, 3 additions join the four waves, one atomic per block"""
    rpb, blocks = ln_bwd_geometry(rows)
    return (rpb + 3) // 4 + 3 + blocks


# ---- cross entropy ---------------------------------------------------------------------------------------------------------
CE_PAIRS = ((1, 1), (63, 64), (64, 64), (65, 72), (1025, 1025), (1025, 1088), (1088, 1088), (1089, 1089), (1100, 1152),
            (2500, 2501))
CE_ROWS = (1, 5, 130)
CE_SWEEP = (65, 72, 8197)           # V, ld, rows: more rows than the 2048 * 4 waves of the cached kernel's grid
CE_CACHED_MAX_V = 64 * 17
CE_PRELOAD = 3.25
HITS_PRELOAD = (1000, 70000)


def ce_ignore(V):
    return V - 1                     # the EOS convention of t2s_model.py: a valid column


def ce_inputs(V, ld, rows, dtype, kind="randn"):
    """logits [rows, ld] on the grid of 1/8 (exact in fp32, bf16 and f16 within +-32: ties with the target's logit are exact
    ties in every build), +inf in the padding columns; int64 targets with 0, V - 1 and the ignored index among them.
    Returns float32 logits."""
    g = gen("ce", V, ld, rows, kind)
    z = torch.round(torch.randn(rows, V, generator=g) * 2 * 8).clamp(-96, 96) / 8
    tg = torch.randint(0, V, (rows,), generator=g)
    ign = ce_ignore(V)
    tg[::7] = ign
    tg[0] = 0
    if rows > 1:
        tg[1] = V - 1
    if rows > 2:
        tg[2] = ign
    if kind == "ranked":                                # targets on the 1st .. 5th largest logit: counts next to every top-k
        order = z.argsort(1, descending=True)
        tg = order[torch.arange(rows), torch.arange(rows) % min(5, V)]
    elif kind == "all_ignored":
        tg[:] = ign
    elif kind == "flat":                                # every logit of a row equal
        z = z[:, :1].expand(rows, V).clone()
    elif kind == "hot":                                 # one logit at +80, the rest at -80: exp underflows to 0
        z = torch.full((rows, V), -80.0)
        hot = torch.randint(0, V, (rows,), generator=g)
        z[torch.arange(rows), hot] = 80.0
        tg[::2] = hot[::2]                              # target on the hot column (loss 0) and off it (loss 160)
    elif kind == "offset":                              # fp32 only: 3e4 + z is exact in fp32 (spacing 2^-9)
        z = z + 3.0e4
    logits = torch.full((rows, ld), float("inf"))
    logits[:, :V] = z
    if dtype != torch.float32:
        assert torch.equal(stored(z, dtype), z), "the grid is not exact in the stored type"
    return logits, tg


def ce_ref(logits, targets, V, topk, ignore_index, dloss, dtype=F64):
    """per-row loss, summed loss, dlogits [rows, ld] with exact zeros in the columns V .. ld - 1, hits (hit count, row
    count) over the rows whose target differs from ignore_index (which never removes a row from the loss)"""
    rows, ld = logits.shape
    z = logits[:, :V].to(dtype)
    mx = z.max(1, keepdim=True)[0]
    e = torch.exp(z - mx)
    se = e.sum(1, keepdim=True)
    lt = z.gather(1, targets[:, None])
    row_loss = (mx + torch.log(se) - lt)[:, 0]
    dl = torch.zeros(rows, ld, dtype=dtype)
    dl[:, :V] = e * (dloss / se)
    dl[torch.arange(rows), targets] -= dloss
    keep = targets != ignore_index
    gt = (z > lt).sum(1)
    hits = (int(((gt < topk) & keep).sum()), int(keep.sum()))
    return row_loss, row_loss.sum(), dl, hits


def ce_depth(rows, V):
    """summed loss.  Cached kernel (V <= 1088): min(ceil(rows / 4), 2048) blocks, a wave adds its grid-stride rows, 3
    additions join the four waves, one atomic per block.  Generic kernel: one atomic per row."""
    if V <= CE_CACHED_MAX_V:
        nb = min((rows + 3) // 4, 2048)
        return (rows + 4 * nb - 1) // (4 * nb) + 3 + nb
    return rows


# ---- ScaledAdam kernels ----------------------------------------------------------------------------------------------------
SA_CHUNK = 1 << 16
SA_NUMELS = (1, 1, 7, 256, 257, SA_CHUNK + 3, 3 * SA_CHUNK)
SA_GAPS = (64, 3, 5, 1, 8, 7, 2, 64)          # before tensor 0, between tensors, behind the last one
SA_STEPS = (0, 3, 88, 89, 500)
SA_HP = dict(lr=0.01, beta1=0.9, beta2=0.95, eps=1e-8, scalar_lr_scale=0.1, scalar_max=10.0)


def f32(v):
    """a python float rounded to fp32: what a c_float field of the hyper-parameter struct holds"""
    return float(torch.tensor(v, dtype=torch.float32))


def hp_f32(hp):
    return {k: (f32(v) if isinstance(v, float) else v) for k, v in hp.items()}


def sa_layout():
    """offsets of the tensors in the arena, its size, the chunk table [(begin, end, tensor)] cut as optim.py cuts it"""
    offs, o = [], 0
    for gap, n in zip(SA_GAPS, SA_NUMELS):
        o += gap
        offs.append(o)
        o += n
    total = o + SA_GAPS[-1]
    chunks = [(c0, min(b + n, c0 + SA_CHUNK), t) for t, (b, n) in enumerate(zip(offs, SA_NUMELS))
              for c0 in range(b, b + n, SA_CHUNK)]
    return offs, total, chunks


def sa_arena():
    """param / grad with NaN in the gaps, delta / exp_avg_sq with a fixed finite pattern there; scalar tensors at +-12 (beyond
    scalar_max); coef rows [scale term, alpha, scalar flag, 0] with a zero scale term for every second tensor"""
    offs, total, chunks = sa_layout()
    g = gen("sa")
    live = torch.zeros(total, dtype=torch.bool)
    p = torch.full((total,), float("nan"))
    gr = torch.full((total,), float("nan"))
    delta = torch.full((total,), -4096.0)
    v = torch.full((total,), 8192.0)
    nt = len(SA_NUMELS)
    coef = torch.zeros(nt, 4)
    for t, (b, n) in enumerate(zip(offs, SA_NUMELS)):
        live[b:b + n] = True
        rms = (0.5, 0.5, 2.0, 0.05, 1.0, 0.3, 0.7)[t]
        p[b:b + n] = torch.randn(n, generator=g) * rms
        gr[b:b + n] = torch.randn(n, generator=g) * 0.1
        delta[b:b + n] = torch.randn(n, generator=g) * 1e-3
        v[b:b + n] = torch.rand(n, generator=g) * 0.02 + 1e-4
        coef[t, 0] = 0.0 if t % 2 else -4e-4 * (t + 1)
        coef[t, 1] = -SA_HP["lr"] * (1 - SA_HP["beta1"]) * rms
        coef[t, 2] = 1.0 if n == 1 else 0.0
    p[offs[0]], p[offs[1]] = 12.0, -12.0
    pre = (torch.arange(nt * 3).float().reshape(nt, 3) - 7.0) / 4 + 0.125
    return dict(p=p, g=gr, delta=delta, v=v, coef=coef, live=live, chunks=chunks, offs=offs, pre=pre)


def sa_stats_ref(p, g, chunks, dtype=F64):
    """[tensors, 3] sums of p g, p p, g g over each tensor's chunks, and the same of the absolute terms"""
    nt = max(c[2] for c in chunks) + 1
    s, a = torch.zeros(nt, 3, dtype=dtype), torch.zeros(nt, 3, dtype=dtype)
    for b, e, t in chunks:
        pp, gg = p[b:e].to(dtype), g[b:e].to(dtype)
        terms = torch.stack([pp * gg, pp * pp, gg * gg])
        s[t] += terms.sum(1)
        a[t] += terms.abs().sum(1)
    return s, a


def sa_stats_depth(chunks):
    """a thread adds ceil(chunk / 256) terms, the block reduction adds 6 + 3 times, one atomic per chunk of the tensor"""
    nt = max(c[2] for c in chunks) + 1
    per = [0] * nt
    longest = [0] * nt
    for b, e, t in chunks:
        per[t] += 1
        longest[t] = max(longest[t], (e - b + 255) // 256)
    return [longest[t] + 9 + per[t] for t in range(nt)]


def sa_apply_ref(p, g, delta, v, chunks, coef, hp, dtype=F64):
    """the element-wise update of sa_apply_kernel over the chunks; everything outside them is returned unchanged.
    hp: lr, beta1, beta2, eps, scalar_lr_scale, scalar_max, step (the values the kernel gets: hp_f32)."""
    p2, d2, v2 = p.to(dtype).clone(), delta.to(dtype).clone(), v.to(dtype).clone()
    b1, b2 = hp["beta1"], hp["beta2"]
    bc2 = 1 - torch.tensor(b2, dtype=dtype) ** (hp["step"] + 1)
    low = float(bc2) < f32(0.99)
    for b, e, t in chunks:
        gr, pv = g[b:e].to(dtype), p2[b:e]
        d = d2[b:e] * b1
        vv = v2[b:e] * b2 + (1 - torch.tensor(b2, dtype=dtype)) * gr * gr
        if float(coef[t, 2]) == 0.0:
            d = d + pv * coef[t, 0].to(dtype)
            vh = vv / bc2 if low else vv
            d = d + gr / (vh.sqrt() + hp["eps"]) * coef[t, 1].to(dtype)
            pv = pv + d
        else:
            d = d + gr / ((vv / bc2).sqrt() + hp["eps"]) * (-hp["lr"] * hp["scalar_lr_scale"] * (1 - torch.tensor(b1, dtype=dtype)))
            pv = pv.clamp(-hp["scalar_max"], hp["scalar_max"]) + d
        p2[b:e], d2[b:e], v2[b:e] = pv, d, vv
    return p2, d2, v2


# ---- ScaledAdam.step() restated per tensor ---------------------------------------------------------------------------------
class ScaledAdamRef:
    """auto_reg/optim.py ScaledAdam.step() on a dict of tensors, every operation in `dtype`: param_rms from the initial
    parameters, the clipping history with its median threshold, the size update every P steps with its two rms clamps, alpha,
    the scalar branch and the bias-correction switch of the apply kernel.  `counters` and `margins` record which branches
    ran and how far the quantities that decide a branch stayed from its threshold."""

    def __init__(self, params, lr=3e-2, clipping_scale=None, betas=(0.9, 0.98), scalar_lr_scale=0.1, eps=1e-8,
                 param_min_rms=1e-5, param_max_rms=3.0, scalar_max=10.0, size_update_period=4,
                 clipping_update_period=100, dtype=F64):
        self.dtype, self.lr, self.clipping_scale, self.betas = dtype, lr, clipping_scale, betas
        self.scalar_lr_scale, self.eps, self.min_rms, self.max_rms = scalar_lr_scale, eps, param_min_rms, param_max_rms
        self.scalar_max, self.P, self.clip_period = scalar_max, size_update_period, clipping_update_period
        self.names = list(params)
        self.shapes = {k: v.shape for k, v in params.items()}
        self.p = {k: v.detach().to(dtype).reshape(-1).clone() for k, v in params.items()}
        nt = len(self.names)
        self.numel = torch.tensor([float(self.p[k].numel()) for k in self.names], dtype=dtype)
        self.is_scalar = self.numel == 1
        self.delta = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.exp_avg_sq = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.param_rms = torch.zeros(nt, dtype=dtype)
        self.scale_exp_avg_sq = torch.zeros(nt, dtype=dtype)
        self.scale_grads = torch.zeros(self.P, nt, dtype=dtype)
        self.model_norms = torch.zeros(self.clip_period, dtype=dtype)
        self.threshold = None
        self.step_count = 0
        self.counters = dict(rms_above=0, rms_below=0, clipped=0, bc2_low=0, bc2_high=0, scalar_clamped=0)
        self.margins = dict(rms=math.inf, norms=math.inf, bc2=math.inf)
        self.bc2_by_step = []

    def params(self):
        return {k: self.p[k].reshape(self.shapes[k]) for k in self.names}

    def _clipping(self, gg):
        step = self.step_count
        one = torch.ones((), dtype=self.dtype)
        if self.clipping_scale is None or step == 0:
            return one
        tot_norm = torch.where(self.is_scalar, gg, gg * self.param_rms ** 2).sum().sqrt()
        self.model_norms[step % self.clip_period] = tot_norm
        if step % self.clip_period == 0:
            s = self.model_norms.sort()[0]
            if len(s) > 1:
                self.margins["norms"] = min(self.margins["norms"], float(((s[1:] - s[:-1]) / s[1:]).min()))
            self.threshold = self.clipping_scale * s[min(self.clip_period - 1, (self.clip_period // 4) * 2)]
        if step < self.clip_period or self.threshold is None:
            return one
        clip = torch.clamp(self.threshold / (tot_norm + 1.0e-20), max=1.0)
        self.counters["clipped"] += int(float(clip) < 1.0)
        return clip

    def step(self, grads, lr=None):
        lr = self.lr if lr is None else lr
        dt, (beta1, beta2), step, P = self.dtype, self.betas, self.step_count, self.P
        g = {k: grads[k].detach().to(dt).reshape(-1) for k in self.names}
        pg = torch.stack([(self.p[k] * g[k]).sum() for k in self.names])
        pp = torch.stack([(self.p[k] * self.p[k]).sum() for k in self.names])
        gg = torch.stack([(g[k] * g[k]).sum() for k in self.names])
        if step == 0:
            self.param_rms = (pp / self.numel).sqrt()
        clip = self._clipping(gg)
        self.scale_grads[step % P] = pg * clip
        coef0 = torch.zeros(len(self.names), dtype=dt)
        if step % P == P - 1:
            self.param_rms = (pp / self.numel).sqrt()
            if step > 0:
                size_lr = lr * self.scalar_lr_scale
                beta2_corr = beta2 ** P
                self.scale_exp_avg_sq = self.scale_exp_avg_sq * beta2_corr + (self.scale_grads ** 2).mean(0) * (1 - beta2_corr)
                bc2 = 1 - beta2_corr ** ((step + 1) // P)
                denom = self.scale_exp_avg_sq.sqrt() + self.eps
                scale_step = -size_lr * (bc2 ** 0.5) * self.scale_grads.sum(0) / denom
                below, above = self.param_rms < self.min_rms, self.param_rms > self.max_rms
                scale_step = torch.where(below, torch.zeros_like(scale_step), scale_step)
                scale_step = torch.where(above, torch.full_like(scale_step, -size_lr * P), scale_step)
                coef0 = scale_step * (1 - beta1) * (~self.is_scalar).to(dt)
                vec = ~self.is_scalar
                self.counters["rms_below"] += int((below & vec).sum())
                self.counters["rms_above"] += int((above & vec).sum())
                for lim in (self.min_rms, self.max_rms):
                    self.margins["rms"] = min(self.margins["rms"], float((self.param_rms[vec] / lim - 1).abs().min()))
        alpha = -lr * (1 - beta1) * self.param_rms.clamp(min=self.min_rms)
        hp = hp_f32(dict(lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(self.eps),
                         scalar_lr_scale=float(self.scalar_lr_scale), scalar_max=float(self.scalar_max), step=step))
        bc2 = 1 - hp["beta2"] ** (step + 1)
        self.bc2_by_step.append(bc2)
        self.counters["bc2_low" if bc2 < f32(0.99) else "bc2_high"] += 1
        self.margins["bc2"] = min(self.margins["bc2"], abs(bc2 - 0.99))
        for t, k in enumerate(self.names):
            coef = torch.stack([coef0[t], alpha[t], self.is_scalar[t].to(dt), torch.zeros((), dtype=dt)])[None]
            if bool(self.is_scalar[t]):
                self.counters["scalar_clamped"] += int((self.p[k].abs() > self.scalar_max).any())
            n = self.p[k].numel()
            self.p[k], self.delta[k], self.exp_avg_sq[k] = sa_apply_ref(self.p[k], g[k], self.delta[k], self.exp_avg_sq[k],
                                                                        [(0, n, 0)], coef, hp, dt)
        self.step_count += 1


# ---- the 100-step trajectory of tests/test_s1_ops_gpu.py --------------------------------------------------------------------
TRAJ_STEPS = 100
TRAJ_SPIKE = (50, 30.0)             # step, gradient scale: the model norm jumps far above twice the median
TRAJ_KW = dict(lr=0.01, betas=(0.9, 0.95), clipping_scale=2.0, clipping_update_period=4, size_update_period=4)
TRAJ_SHAPES = {"big": (12, 25), "mid": (17,), "tiny": (40,), "wide": (3, 5, 7), "s_hi": (1,), "s_lo": (1,), "s_in": (1,)}


def traj_init():
    """`big` starts with rms 5 (> param_max_rms), `tiny` with rms 1e-7 (< param_min_rms), two scalars at +-12 (beyond
    scalar_max); the rest sits between the clamps"""
    g = gen("traj", "init")
    scale = dict(big=5.0, mid=0.3, tiny=1e-7, wide=0.8)
    init = {k: torch.randn(s, generator=g) * scale.get(k, 1.0) for k, s in TRAJ_SHAPES.items()}
    init["s_hi"], init["s_lo"], init["s_in"] = torch.tensor([12.0]), torch.tensor([-12.0]), torch.tensor([0.2])
    return init


def traj_grads():
    g = gen("traj", "grads")
    out = []
    for step in range(TRAJ_STEPS):
        # the four norms of a clipping period differ by 30 % and more: their sorted order is the same in every precision
        sc = 0.1 * (0.7, 1.0, 1.4, 1.9)[step % 4] * (TRAJ_SPIKE[1] if step == TRAJ_SPIKE[0] else 1.0)
        out.append({k: torch.randn(s, generator=g) * sc for k, s in TRAJ_SHAPES.items()})
    return out


def traj_run(dtype):
    """the trajectory in `dtype`: list over steps of {name: parameters after the step} (float64 copies) and the optimiser"""
    opt = ScaledAdamRef(traj_init(), dtype=dtype, **TRAJ_KW)
    out = []
    for gs in traj_grads():
        opt.step(gs)
        out.append({k: v.to(F64).clone() for k, v in opt.params().items()})
    return out, opt


def traj_tolerance(run32, run64):
    """{name: [tolerance at step s]}: 8 x the largest deviation of the fp32 run from the float64 run on that tensor up to that
    step (the factor covers fp32 error compounding through a different summation order), and never below 8 x the half
    spacing of fp32 at the tensor's largest parameter -- the stored result cannot be closer than its format allows"""
    tol = {}
    for k in run64[0]:
        worst, tol[k] = 0.0, []
        for a, b in zip(run32, run64):
            worst = max(worst, float((a[k] - b[k]).abs().max()))
            tol[k].append(8.0 * max(worst, U * float(b[k].abs().max())))
    return tol
