"""Float64 oracle and seeded inputs for the semantic-code kernel (evt_semantic_codes_rows): ssl_proj (Conv1d D -> D, k = 2,
stride 2) + the nearest code of a codebook, on ragged batches of channels-last hidden states.  Shares no code with the
library: torch on the CPU only.

The oracle works per row in double: F.conv1d, dist[t][k] = |h_t|^2 - 2 h_t . e_k + |e_k|^2, the FIRST minimum as the code.
Per frame it also gives
  margin  second-best minus best distance (0 for an exact tie);
  E       how far the float64 distance of a code that ANY fp32 evaluation of the formula may choose can lie above the
          minimum.  With u = 2^-24 and g(n) = n u / (1 - n u) for a sum of n terms in any order:
            dh[d]  = g(2 D + 1) (sum_{tap, c} |x| |w| + |b|)[d]                  the projection's rounding
            Exx    = g(D + 1) sum (|h| + dh)^2 + sum (2 |h| dh + dh^2)           xx: its rounding + the projection's error
            Edot_k = g(D) sum (|h| + dh) |e_k| + sum dh |e_k|                    the dot: its rounding + the projection's error
            Eee_k  = g(D) |e_k|^2                                                ee
            Efin_k = 3 u (xx + 2 |dot_k| + ee_k)                                 the two roundings of (xx - 2 dot) + ee
            e_k    = Exx + 2 Edot_k + Eee_k + Efin_k                             bound of the error of one computed distance
          a chosen code c has computed dist_c <= computed dist_best, so its true distance is above the minimum by at most
          e_c + e_best <= E := 2 max_k e_k.  A frame whose margin exceeds E has one possible answer."""
import hashlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FRAMES = [1, 2, 63, 64, 67, 131]          # 0 / 1 / 31 / 32 / 33 / 65 codes: empty, one, a tile edge from both sides, odd, > 2 tiles
SHAPES = [(768, 1024), (128, 72)]         # the model's, and one with a codebook tail (72 = 64 + 8)


def gam(n):
    return n * U / (1.0 - n * U)


def oracle_row(x, w, bias, embed):
    """x [T, D] (any float dtype: widened), w [D, D, 2], bias [D], embed [K, D] -> dict of codes int64 [T // 2], margin, E
    float64 [T // 2] and dist float64 [T // 2, K]"""
    T, D = x.shape
    K = embed.size(0)
    n = T // 2
    if n == 0:
        z = torch.zeros(0, dtype=torch.float64)
        return dict(codes=torch.zeros(0, dtype=torch.int64), margin=z, E=z, dist=torch.zeros(0, K, dtype=torch.float64))
    xd, wd, bd, ed = x.double(), w.double(), bias.double(), embed.double()
    xin = xd[: 2 * n].t().unsqueeze(0)                                          # [1, D, 2 n]
    h = F.conv1d(xin, wd, bd, stride=2)[0].t()                                  # [n, D]
    habs = F.conv1d(xin.abs(), wd.abs(), bd.abs(), stride=2)[0].t()
    dh = gam(2 * D + 1) * habs
    xx = (h * h).sum(1, keepdim=True)
    ee = (ed * ed).sum(1)[None]
    dot = h @ ed.t()
    dist = xx - 2 * dot + ee
    best = dist.min(1, keepdim=True).values
    idx = torch.arange(K)[None].expand_as(dist)
    codes = torch.where(dist == best, idx, torch.full_like(idx, K)).min(1).values
    two = torch.topk(dist, min(2, K), dim=1, largest=False).values
    margin = two[:, -1] - two[:, 0] if K > 1 else torch.full((n,), float("inf"), dtype=torch.float64)
    hup = h.abs() + dh
    exx = gam(D + 1) * (hup * hup).sum(1, keepdim=True) + (2 * h.abs() * dh + dh * dh).sum(1, keepdim=True)
    edot = gam(D) * (hup @ ed.abs().t()) + dh @ ed.abs().t()
    eee = gam(D) * ee
    efin = 3 * U * (xx + 2 * dot.abs() + ee)
    E = 2 * (exx + 2 * edot + eee + efin).max(1).values
    return dict(codes=codes, margin=margin, E=E, dist=dist)


def oracle(x, frames, w, bias, embed):
    """x [B, Tmax, D]: one oracle_row per row over its first frames[b] frames (nothing behind them is looked at)"""
    return [oracle_row(x[b, :t], w, bias, embed) for b, t in enumerate(frames)]


def fp32_codes(x, frames, w, bias, embed):
    """the reference's formula (core_vq.py:172-180) composed from fp32 torch operators, first maximum"""
    out = []
    for b, t in enumerate(frames):
        n = t // 2
        if n == 0:
            out.append(torch.zeros(0, dtype=torch.int64))
            continue
        h = F.conv1d(x[b, : 2 * n].float().t().unsqueeze(0), w.float(), bias.float(), stride=2)[0].t()
        e = embed.float()
        dist = -(h.pow(2).sum(1, keepdim=True) - 2 * h @ e.t() + e.pow(2).sum(1)[None])
        idx = torch.arange(e.size(0))[None].expand_as(dist)
        out.append(torch.where(dist == dist.max(1, keepdim=True).values, idx, torch.full_like(idx, e.size(0))).min(1).values)
    return out


def _pad(rows, tmax):
    """rows: list of [T_b, D] -> [B, tmax, D] with NaN behind every row's frames"""
    out = torch.full((len(rows), tmax, rows[0].size(1)), float("nan"), dtype=torch.float32)
    for b, r in enumerate(rows):
        out[b, : r.size(0)] = r
    return out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_inputs(D, K, frames=FRAMES, tmax=None, seed=11):
    """Integer-exact: features with 4 entries of {+-1, +-2} per frame (8 per pair), a dense {+-1, +-2} projection, bias in
    -1 .. 1, codebook in -2 .. 2 (two planted codes in -3 .. 3).  |h| <= 8 * 4 + 1 = 33, xx <= D * 33^2, |dot| <= D * 33 * 3,
    ee <= 9 D: for D <= 1152 every partial sum of every product is an integer below 2^24 in magnitude, so fp32 is exact in
    any order.  Codes K/2 + i copy code i for i % 4 != 3 (exact ties whose lower index must win).  Codes 3 and 7 are
    bias + r and bias - r (r: +-2 on the first D / 3 coordinates): every all-zero pair of frames (each third pair) projects
    onto the bias, at distance |r|^2 from both and further from every other code."""
    g = _gen(seed)
    pm = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1) * torch.randint(1, 3, shape, generator=g)
    w = pm((D, D, 2)).float()
    bias = torch.randint(-1, 2, (D,), generator=g).float()
    embed = torch.randint(-2, 3, (K, D), generator=g).float()
    half = K // 2
    for i in range(half):
        if i % 4 != 3:
            embed[half + i] = embed[i]
    r = torch.zeros(D)
    r[: D // 3] = 2.0 * (torch.randint(0, 2, (D // 3,), generator=g) * 2 - 1)
    embed[3], embed[7] = bias + r, bias - r
    rows = []
    for t in frames:
        r = torch.zeros(t, D)
        for f in range(t):
            if (f // 2) % 3 == 2:
                continue                                    # a zero pair: equidistant from codes 3 and 7
            pos = torch.randperm(D, generator=g)[:4]
            r[f, pos] = pm((4,)).float()
        rows.append(r)
    return dict(x=_pad(rows, tmax or max(frames) + 5), frames=list(frames), w=w, bias=bias, embed=embed)


def _planted(D, K, frames, tmax, seed, target_fn):
    g = _gen(seed)
    q, _ = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
    bmat = 0.05 * torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5          # tap 1: small
    bias = 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    embed = torch.randn(K, D, generator=g, dtype=torch.float64)
    w = torch.stack([q.t(), bmat.t()], dim=2)                                             # h = x0 Q + x1 B + b
    rows = []
    for t in frames:
        n = t // 2
        r = torch.randn(t, D, generator=g, dtype=torch.float64)
        if n:
            target = target_fn(g, n, embed)
            r[0: 2 * n: 2] = (target - bias - r[1: 2 * n: 2] @ bmat) @ q.t()
        rows.append(r.float())
    return dict(x=_pad(rows, tmax or max(frames) + 5), frames=list(frames), w=w.float(), bias=bias.float(),
                embed=embed.float())


def planted_inputs(D, K, frames=FRAMES, tmax=None, seed=12):
    """tap 0 of the projection is a float64-orthogonal Q, tap 1 small; x[2t] = (e_c + noise - b - x[2t + 1] B) Q^T, so frame t
    projects onto code c plus noise of 0.5 (even t) or 0.9 (odd t) of the codebook's unit scale per coordinate"""
    def target(g, n, embed):
        c = torch.randint(0, embed.size(0), (n,), generator=g)
        scale = torch.where(torch.arange(n) % 2 == 0, 0.5, 0.9).double()[:, None]
        return embed[c] + scale * torch.randn(n, embed.size(1), generator=g, dtype=torch.float64)
    return _planted(D, K, frames, tmax, seed, target)


CLOSE_DELTA = 0.05


def close_pair_inputs(D, K, frames=FRAMES, tmax=None, seed=13, delta=CLOSE_DELTA):
    """the projected frame lies between two different codes a, b: at their midpoint moved by the fraction `delta` of the way
    towards a, where dist_b - dist_a = delta |e_a - e_b|^2 (about 2 D delta)"""
    def target(g, n, embed):
        a = torch.randint(0, embed.size(0), (n,), generator=g)
        b = (a + 1 + torch.randint(0, embed.size(0) - 1, (n,), generator=g)) % embed.size(0)
        mid = 0.5 * (embed[a] + embed[b])
        return mid + delta * (embed[a] - mid)
    return _planted(D, K, frames, tmax, seed, target)


def unplanted_inputs(D, K, frames=FRAMES, tmax=None, seed=14):
    """random normal everywhere (the projection scaled to keep h at unit scale): margins are of the size of E here, so only
    the per-frame bound can be asked"""
    g = _gen(seed)
    w = torch.randn(D, D, 2, generator=g) / (2 * D) ** 0.5
    bias = 0.1 * torch.randn(D, generator=g)
    embed = torch.randn(K, D, generator=g)
    rows = [torch.randn(t, D, generator=g) for t in frames]
    return dict(x=_pad(rows, tmax or max(frames) + 5), frames=list(frames), w=w, bias=bias, embed=embed)


GENERATORS = dict(exact=exact_inputs, planted=planted_inputs, close=close_pair_inputs, unplanted=unplanted_inputs)


def checksum(inp):
    """sha256 over the live values of the inputs (the NaN padding left out), each rounded to a grid of 2^-10: the planted
    inputs come out of float64 QR and matrix products, whose last bits may differ between BLAS builds -- far below what
    moves a value across that grid, or a planted frame to another code"""
    h = hashlib.sha256()
    grid = lambda t: (t.double() * 1024).round().to(torch.int32).contiguous().numpy().tobytes()
    for b, t in enumerate(inp["frames"]):
        h.update(grid(inp["x"][b, :t]))
    for k in ("w", "bias", "embed"):
        h.update(grid(inp[k]))
    return h.hexdigest()
