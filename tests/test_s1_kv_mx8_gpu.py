"""GPU: the MXFP8 key/value cache of s1 decode streams (csrc/s1_decode_mx8.hip, StreamSession(kv_dtype="mxfp8")): the pack
kernel against the format's definition restated on the host (bytes), the attention kernel against float64 on the
dequantised cache and against itself row by row (bits), the refusals, and the cache through decode_stream / score_stream.
Both tolerances are measured inside the tests from parent code and printed before the assertion (figures: DESIGN §11)."""
import os
import sys

import pytest
import torch

from test_s1_stream_gpu import _i32, model  # noqa: F401  (the small seeded model of the stream tests)

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
IDLE, RUNNING, STOP_EOS = 0, 1, 2


def mx_quant(v):
    """the definition of include/evt.h on the host: v [..., 32] -> (codes uint8 [..., 32], scale bytes uint8 [...])"""
    v = v.double().cpu()
    bad = ~torch.isfinite(v).all(-1)
    a = v.abs().amax(-1).masked_fill(bad, 1.0)
    m, x = torch.frexp(a)
    e = torch.where(m <= 0.875, x - 9, x - 8).clamp(-127, 127)
    e = torch.where(a == 0, torch.full_like(e, -127), e)
    codes = torch.ldexp(v, -e.unsqueeze(-1)).float().to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.masked_fill(bad.unsqueeze(-1), 0), (e + 127).masked_fill(bad, 255).to(torch.uint8)


def mx_dequant(codes, s):
    """float64 values of (codes, scale bytes); NaN rows for the scale byte 0xFF"""
    val = codes.cpu().view(torch.float8_e4m3fn).double() * torch.exp2(s.cpu().double() - 127).unsqueeze(-1)
    return val.masked_fill((s.cpu() == 255).unsqueeze(-1), float("nan"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "h16"])
def test_pack_bit_for_bit(gpu, dtype):
    """k = 3 prompt rows, S = 19, H = 2 into five of six cache rows (source 1 twice; n_pos 19 / 7 / 1): the host quantiser's
    bytes, planted edge rows included; every other byte (behind n_pos, the unmapped row) keeps its 0xA5"""
    from easevoice_trainer_amd.hip import lib as L

    k, S, H, B, Lmax, E = 3, 19, 2, 6, 32, 64
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(k, S, 3 * E, generator=g) * torch.exp2(torch.randint(-9, 9, (k, S, 1), generator=g).float())).to(dtype)
    up = lambda t: (t.view(torch.int32 if dtype == torch.float32 else torch.int16) + 1).view(dtype)     # one ulp above
    rows = qkv[1, :7, E:2 * E].view(7, H, 32)                  # key head rows of source 1, all inside its n_pos = 7
    rows[0, 0] = torch.tensor([0.0, -0.0] * 16, dtype=dtype)                                            # signed zeros
    rows[1, 1], rows[1, 1, 5] = rows[1, 1].clamp(-50, 50), 56.0                                         # amax = 448 * 2^-3: m = 0.875
    rows[2, 0], rows[2, 0, 5:6] = rows[1, 1], up(rows[1, 1, 5:6].clone())                               # ... and one ulp above
    rows[3, 1] = (1.3 * 2.0 ** torch.linspace(-20, 10, 32) * torch.tensor([1.0, -1.0] * 16)).to(dtype)  # subnormal codes
    rows[4, 0, 7], rows[5, 1, 31] = float("nan"), float("-inf")
    q = qkv.to(gpu)
    dst, src, npos = [4, 0, 2, 5, 1], [0, 1, 1, 2, 0], [19, 7, 7, 1, 19]
    maps = [_i32(v, gpu) for v in (dst, src, npos)]
    bufs = [torch.full(s, 0xA5, dtype=torch.uint8, device=gpu) for s in ((B, H, Lmax, 32), (B, H, Lmax)) * 2]
    L.check(L.lib().evt_kv_pack_mx8_rows(L.dt_of(q), L.ptr(q), *map(L.ptr, maps), *map(L.ptr, bufs), 5, k, S, B, H, 32, Lmax,
                                         L.stream_ptr()), "evt_kv_pack_mx8_rows")
    torch.cuda.synchronize()
    want = [torch.full_like(b, 0xA5).cpu() for b in bufs]
    for d, s_, n in zip(dst, src, npos):
        for o, part in ((0, qkv[s_, :n, E:2 * E]), (2, qkv[s_, :n, 2 * E:])):
            c, s = mx_quant(part.float().reshape(n, H, 32))
            want[o][d, :, :n], want[o + 1][d, :, :n] = c.transpose(0, 1), s.t()
    assert (want[1][0, :, :7] == 255).sum() == 2 and (want[0][0, 1, 3] & 0x78 == 0).sum() > 4     # NaN rows, subnormal codes
    assert [torch.equal(got.cpu(), w) for got, w in zip(bufs, want)] == [True] * 4      # k codes, k scales, v codes, v scales


POS = [40, 41, 255, 256, 257, 511, 100, 300]
X_LENS = [0, 1, 33, 40, 40, 33, 0, 1]
STATUS = [RUNNING] * 6 + [IDLE, STOP_EOS]


def _attn(L, qkv, cache, rstate, xl, out, B, H, Lmax, x_len, D=32):
    rc = L.lib().evt_dec_attn_rows_mx8(L.ptr(qkv), *map(L.ptr, cache), L.ptr(rstate), L.ptr(out), B, H, D, Lmax, L.ptr(xl),
                                       x_len, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def case(gpu):
    """a host-quantised random cache, a NaN head row in reach of row 2 / head 1, ONE launch of the kernel under test; k and v
    of qkv are made representable, so that the fp32 kernel sees the same values"""
    from easevoice_trainer_amd.hip import lib as L

    B, H, Lmax, x_len, E = 8, 2, 512, 40, 64
    g = torch.Generator().manual_seed(11)
    scale = torch.exp2(torch.randint(-3, 3, (B, H, Lmax, 1), generator=g).float())
    cache0 = [t for _ in range(2) for t in mx_quant(torch.randn(B, H, Lmax, 32, generator=g) * scale)]
    cache0[1][2, 1, 100], cache0[0][2, 1, 100] = 255, 0
    qkv = torch.randn(B, 3, H, 32, generator=g)
    qkv[:, 1:] = mx_dequant(*mx_quant(qkv[:, 1:])).float()
    rstate = _i32([[POS[b], 3, 9, 5, 100, STATUS[b], 0, 0] for b in range(B)], gpu)
    t = dict(L=L, B=B, H=H, Lmax=Lmax, x_len=x_len, E=E, cache0=cache0, qkv=qkv.view(B, 3 * E).to(gpu), rstate=rstate,
             xl=_i32(X_LENS, gpu), cache=[c.to(gpu) for c in cache0], out=torch.full((B, E), -7.0, device=gpu))
    L.check(_attn(L, t["qkv"], t["cache"], rstate, t["xl"], t["out"], B, H, Lmax, x_len), "evt_dec_attn_rows_mx8")
    return t


def test_attn_against_float64(gpu, case):
    """float64 softmax attention over the dequantised cache and new token; bound: 4x the error of evt_dec_attn_rows on an fp32
    cache of the same values.  Exact: the bytes appended at POS, all other cache bytes, idle / stopped rows, the NaN head"""
    t, L = case, case["L"]
    B, H, Lmax, E = t["B"], t["H"], t["Lmax"], t["E"]
    kd, vd = mx_dequant(*t["cache0"][:2]), mx_dequant(*t["cache0"][2:])
    q3 = t["qkv"].cpu().view(B, 3, H, 32)
    ref, want = torch.full((B, H, 32), -7.0, dtype=torch.float64), [c.clone() for c in t["cache0"]]
    for b in range(B):
        if STATUS[b] != RUNNING:
            continue
        keep = [j for j in range(POS[b]) if not X_LENS[b] <= j < t["x_len"]]
        K = torch.cat([kd[b][:, keep], q3[b, 1].double().unsqueeze(1)], 1)
        V = torch.cat([vd[b][:, keep], q3[b, 2].double().unsqueeze(1)], 1)
        p = torch.softmax((K @ q3[b, 0].double().unsqueeze(-1)).squeeze(-1) / 32 ** 0.5, -1)
        ref[b] = (p.unsqueeze(-1) * V).sum(1)
        for o in (0, 2):
            want[o][b, :, POS[b]], want[o + 1][b, :, POS[b]] = mx_quant(q3[b, 1 + o // 2])
    # the parent's kernel on the same values: fp32 slabs [B][Lmax][E]
    kc, vc = (d.float().permute(0, 2, 1, 3).reshape(B, Lmax, E).contiguous().to(gpu) for d in (kd, vd))
    out32 = torch.full((B, E), -7.0, device=gpu)
    L.check(L.lib().evt_dec_attn_rows(L.DT_F32, L.ptr(t["qkv"]), L.ptr(kc), L.ptr(vc), L.ptr(t["rstate"]), L.ptr(out32), B, H,
                                      32, Lmax, L.ptr(t["xl"]), t["x_len"], L.stream_ptr()), "evt_dec_attn_rows")
    torch.cuda.synchronize()
    ok = torch.isfinite(ref) & (torch.tensor(STATUS) == RUNNING).view(B, 1, 1)
    err = [float(((o.cpu().view(B, H, 32).double() - ref)[ok]).abs().max() / ref[ok].abs().max()) for o in (out32, t["out"])]
    print(f"max error / max |ref|: evt_dec_attn_rows fp32 cache {err[0]:.3e}, evt_dec_attn_rows_mx8 {err[1]:.3e}")
    assert 0 < err[0] < 1e-5 and err[1] <= 4 * err[0], err
    got = t["out"].cpu().view(B, H, 32)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.isnan(got[2, 1]).all() and int(torch.isnan(got).sum()) == 32
    assert torch.equal(got[6:], torch.full((2, H, 32), -7.0))
    assert [torch.equal(c.cpu(), w) for c, w in zip(t["cache"], want)] == [True] * 4     # k codes, k scales, v codes, v scales


def test_attn_row_is_the_row_alone(gpu, case):
    """every running row of the batched launch, launched again alone (B = 1): output and slabs bit for bit"""
    t, L = case, case["L"]
    for b in range(6):
        one, out = [c[b:b + 1].to(gpu) for c in t["cache0"]], torch.full((1, t["E"]), -7.0, device=gpu)
        L.check(_attn(L, t["qkv"][b:b + 1].contiguous(), one, t["rstate"][b:b + 1].contiguous(), t["xl"][b:b + 1].contiguous(), out,
                      1, t["H"], t["Lmax"], t["x_len"]), "evt_dec_attn_rows_mx8")
        assert torch.equal(out.view(torch.int32), t["out"][b:b + 1].view(torch.int32)), b
        assert all(torch.equal(o[0], c[b]) for o, c in zip(one, t["cache"])), b


def _reqs(gpu, rows):
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(8)
    return [(d["x"][r].to(gpu), d["bert"][r].to(gpu), d["prompts"][r].to(gpu), dict(seed=100 + r)) for r in rows]


def test_refusals(gpu, case, model, monkeypatch):
    """D = 64: the not-supported code; an unknown kv_dtype; a 64-slot session over half the free memory, the 33-byte count named"""
    from easevoice_trainer_amd.hip.lib import EVT_ENOTSUP, EvtError

    t = case
    assert _attn(t["L"], t["qkv"], t["cache"], t["rstate"], t["xl"], t["out"], t["B"], 1, t["Lmax"], t["x_len"], D=64) == EVT_ENOTSUP
    with pytest.raises(EvtError, match="fp4"):
        model.decode_stream(_reqs(gpu, [0]), kv_dtype="fp4")
    need = 2 * model.num_layers * 64 * 512 * model.num_head * 33
    for name, v in (("memory_reserved", 0), ("memory_allocated", 0), ("mem_get_info", (2 * need - 1, 4 * need))):
        monkeypatch.setattr(torch.cuda, name, lambda dev=None, v=v: v)
    with pytest.raises(EvtError, match=f"64 slots.*{need} bytes.*{2 * need - 1} bytes free"):
        model._infer().stream_session(64, 24, 100, 50, torch.float32, str(gpu), "mxfp8")


def test_stream_rows_and_candidates(gpu, model):
    """(a) seeded requests: the same tokens alone in one slot and among others in four; (b) n = 3: a request's three slots hold
    the same prompt bytes in every layer, other bytes than another request's"""
    kw = dict(kv_dtype="mxfp8", top_k=15, top_p=1, early_stop_num=8, max_text_len=24, max_prompt_len=12)
    alone = {r: y for r, y, _i in model.decode_stream(_reqs(gpu, [0, 1, 2]), slots=1, **kw)}
    order = [5, 0, 6, 1, 2, 7]
    among = {order[r]: y for r, y, _i in model.decode_stream(_reqs(gpu, order), slots=4, **kw)}
    assert all(torch.equal(alone[r], among[r]) for r in range(3)) and not torch.equal(alone[0][12:], alone[1][12:])
    outs = list(model.decode_stream(_reqs(gpu, [0, 1]), slots=6, n=3, **kw))
    inf = model._infer()
    S = inf._sessions[inf._wide[-1]]
    n = S.Xmax + 12
    assert len(outs) == 6 and S.kv_dtype == "mxfp8" and S.kc is None
    for buf in (S.kq, S.ks, S.vq, S.vs):
        assert buf.dtype == torch.uint8 and buf[:, 0, :, :n].any()
        assert all(torch.equal(buf[:, s, :, :n], buf[:, 3 * (s // 3), :, :n]) for s in range(6))
        assert not torch.equal(buf[:, 0, :, :n], buf[:, 3, :, :n])


def test_score_stream_gate(gpu, model):
    """mean |model log-prob - fp32 session's|: d8 with the MXFP8 cache under fp32 weights, d16 of the bf16 session (parent
    code).  0 < d8 <= 32 d16: e4m3's rounding step is 16x bf16's, 2x on top; a mis-wired layer or row moves far more"""
    g = torch.Generator().manual_seed(9)
    toks = [torch.randint(0, 1024, (10,), generator=g) for _ in range(4)]

    def score(cd, **kw):
        model.cd = cd
        try:
            got = dict(model.score_stream(_reqs(gpu, range(4)), toks, slots=4, **kw))
            return torch.stack([got[r][:, 0].cpu() for r in range(4)])
        finally:
            model.cd = torch.float32

    lp32, lp8, lp16 = score(torch.float32), score(torch.float32, kv_dtype="mxfp8"), score(torch.bfloat16)
    d8, d16 = float((lp8 - lp32).abs().mean()), float((lp16 - lp32).abs().mean())
    print(f"mean |d log-prob| against the fp32 session: mxfp8 cache d8 = {d8:.3e}, bf16 session d16 = {d16:.3e}")
    assert d16 >= 1e-5, d16      # the gate is not vacuous with the default fill
    assert 0 < d8 <= 32 * d16, (d8, d16)
