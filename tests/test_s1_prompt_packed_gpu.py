"""GPU: the packed prompt pass of s1 decode streams (csrc/attn_packed.hip, decode_stream(prompt_pass="packed")): the attention
against float64 with the padded kernel's own error as the bound, a sequence against itself packed alone (bits), the fused
cache write in the three formats (bytes), the refusals, and the pass through score_stream / decode_stream.  Every bound is
measured inside its test from parent code and printed before the assertion (figures: DESIGN §11)."""
import pytest
import torch

from test_s1_kv_mx8_gpu import _reqs
from test_s1_stream_gpu import _i32, model  # noqa: F401  (the small seeded model of the stream tests)

pytestmark = pytest.mark.gpu
H, D, E, XMAX, LMAX, B = 2, 32, 64, 96, 256, 6
PACKS = {"edges16": [(1, 1), (15, 0), (16, 17), (17, 64)], "edges64": [(63, 1), (64, 65), (65, 130)]}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "h16"])


def _qkv(pack, dtype, gpu, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sum(a + b for a, b in pack), 3 * E, generator=g).to(dtype).to(gpu)


def _caches(fmt, gpu):
    """sentinel-filled caches of one layer as bytes: slab [B][Lmax][E * itemsize] x 2, or MXFP8 codes / scales"""
    if fmt == "mx8":
        shapes = ((B, H, LMAX, 32), (B, H, LMAX, 32), (B, H, LMAX), (B, H, LMAX))
    else:
        shapes = ((B, LMAX, E * fmt.itemsize),) * 2
    return [torch.full(s, 0xA5, dtype=torch.uint8, device=gpu) for s in shapes]


def _launch(qkv, pack, slots, fmt, gpu, D=D):
    """one launch on sentinel caches -> (return code, out [T][E], caches as bytes)"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import packed_layout
    from easevoice_trainer_amd.hip import lib as L

    xl, yl = [a for a, _b in pack], [b for _a, b in pack]
    tok0, tiles, off, slot = packed_layout(xl, yl, slots)
    desc = [_i32(v, gpu) for v in (tok0, xl, yl, tiles, off, slot)]
    out, cache = torch.full((qkv.size(0), E), -7.0, dtype=qkv.dtype, device=gpu), _caches(fmt, gpu)
    mx = fmt == "mx8"
    rc = L.lib().evt_attn_prefixlm_packed_fwd(
        L.dt_of(qkv), L.ptr(qkv), L.ptr(out), *map(L.ptr, desc), 1 if mx else 0, 0 if mx else L.dt_code(fmt),
        L.ptr(cache[0]), L.ptr(cache[1]), L.ptr(cache[2] if mx else None), L.ptr(cache[3] if mx else None), qkv.size(0),
        len(pack), len(tiles) // 2, len(slot), H, D, B, LMAX, XMAX, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, cache


def _padded(qkv, pack, gpu):
    """the pack as the rectangle of the padded pass [k][x_len + P][3E] (zeros as padding) and each packed row's place in it"""
    x_len, P = max(a for a, _b in pack), max(b for _a, b in pack)
    pad, where, t = torch.zeros(len(pack), x_len + P, 3 * E, dtype=qkv.dtype, device=gpu), [], 0
    for s, (a, b) in enumerate(pack):
        rows = list(range(a)) + list(range(x_len, x_len + b))
        pad[s, rows] = qkv[t:t + a + b]
        where += [(s, r) for r in rows]
        t += a + b
    return pad, x_len, tuple(torch.tensor(w, device=gpu) for w in zip(*where))


@DTYPES
@pytest.mark.parametrize("name", list(PACKS))
def test_attention_against_float64(gpu, dtype, name):
    """float64 softmax attention of every sequence alone, the mask written out; bound: twice the error of
    evt_attn_prefixlm_fwd on the same sequences padded (the same MFMA arithmetic, other tile boundaries), at least one
    rounding step of the output dtype"""
    from easevoice_trainer_amd.auto_reg.ops import PrefixLMAttentionFn

    pack = PACKS[name]
    qkv = _qkv(pack, dtype, gpu)
    ref, t = [], 0
    for a, b in pack:
        q, k, v = (qkv[t:t + a + b, i * E:(i + 1) * E].double().cpu().view(a + b, H, D).transpose(0, 1) for i in range(3))
        i, j = torch.arange(a + b).view(-1, 1), torch.arange(a + b).view(1, -1)
        see = torch.where(i < a, j < a, j <= i)
        p = torch.softmax((q @ k.transpose(1, 2) / D ** 0.5).masked_fill(~see, float("-inf")), -1)
        ref.append((p @ v).transpose(0, 1).reshape(a + b, E))
        t += a + b
    ref = torch.cat(ref)
    rc, out, _c = _launch(qkv, pack, [[s] for s in range(len(pack))], dtype, gpu)
    assert rc == 0
    pad, x_len, (ps, pr) = _padded(qkv, pack, gpu)
    old = PrefixLMAttentionFn.apply(pad, _i32([a for a, _b in pack], gpu), _i32([b for _a, b in pack], gpu), x_len, H, 0.0, 0)
    err = [float((o.double().cpu() - ref).abs().max() / ref.abs().max()) for o in (old[ps, pr], out)]
    print(f"{name} {dtype}: max error / max |ref|: evt_attn_prefixlm_fwd {err[0]:.3e}, packed {err[1]:.3e}")
    assert 0 < err[0] and err[1] <= max(2 * err[0], torch.finfo(dtype).eps), err


@DTYPES
def test_sequence_is_the_sequence_alone(gpu, dtype):
    """every sequence of the 64-edge pack, packed alone into the same slot: output rows and cache bytes, both formats"""
    pack = PACKS["edges64"]
    qkv = _qkv(pack, dtype, gpu)
    for fmt in (dtype, "mx8"):
        _rc, out, cache = _launch(qkv, pack, [[s] for s in range(len(pack))], fmt, gpu)
        t = 0
        for s, (a, b) in enumerate(pack):
            rc, o1, c1 = _launch(qkv[t:t + a + b].contiguous(), [(a, b)], [[s]], fmt, gpu)
            assert rc == 0 and torch.equal(o1.view(torch.int16), out[t:t + a + b].view(torch.int16)), (fmt, s)
            assert all(torch.equal(x[s], y[s]) and not (x[s] == 0xA5).all() for x, y in zip(c1, cache)), (fmt, s)
            t += a + b


@pytest.mark.parametrize("fmt", [torch.float32, torch.bfloat16, "mx8"], ids=["slab_f32", "slab_h16", "mx8"])
def test_cache_write_bit_for_bit(gpu, fmt):
    """sequence 0 into slots 0 and 3, sequence 1 into slot 1 and the out-of-range slot 9, sequence 2 into slot 4: the mapped
    positions hold the K / V columns of qkv (slab) or the bytes of evt_kv_pack_mx8_rows (MXFP8), every other byte its 0xA5"""
    from easevoice_trainer_amd.hip import lib as L

    pack, slots = PACKS["edges64"], [[0, 3], [1, 9], [4]]
    qkv = _qkv(pack, torch.float32 if fmt == "mx8" else fmt, gpu)
    rc, _out, cache = _launch(qkv, pack, slots, fmt, gpu)
    assert rc == 0
    want, t = _caches(fmt, gpu), 0
    if fmt == "mx8":        # the pack kernel on the padded rectangle [k][Xmax + P][3E]; it also fills xl <= j < Xmax: put back
        P = max(b for _a, b in pack)
        pad = torch.zeros(len(pack), XMAX + P, 3 * E, device=gpu)
        maps = [[], [], []]
        for s, (a, b) in enumerate(pack):
            pad[s, :a], pad[s, XMAX:XMAX + b] = qkv[t:t + a], qkv[t + a:t + a + b]
            for d in (x for x in slots[s] if x < B):
                maps[0].append(d), maps[1].append(s), maps[2].append(XMAX + b)
            t += a + b
        dev_maps = [_i32(v, gpu) for v in maps]
        L.check(L.lib().evt_kv_pack_mx8_rows(L.dt_of(pad), L.ptr(pad), *map(L.ptr, dev_maps), L.ptr(want[0]),
                                             L.ptr(want[2]), L.ptr(want[1]), L.ptr(want[3]), len(maps[0]), len(pack), XMAX + P,
                                             B, H, 32, LMAX, L.stream_ptr()), "evt_kv_pack_mx8_rows")
        for d, s in zip(maps[0], maps[1]):
            for w in want:
                w[d, :, pack[s][0]:XMAX] = 0xA5
    else:
        for s, (a, b) in enumerate(pack):
            for d in (x for x in slots[s] if x < B):
                for w, c0 in zip(want, (E, 2 * E)):
                    w = w.view(fmt)
                    w[d, :a], w[d, XMAX:XMAX + b] = qkv[t:t + a, c0:c0 + E], qkv[t + a:t + a + b, c0:c0 + E]
            t += a + b
    torch.cuda.synchronize()
    assert [torch.equal(c, w) for c, w in zip(cache, want)] == [True] * len(want)
    assert (want[0][5] == 0xA5).all() and not (want[0][3] == 0xA5).all()


def test_refusals(gpu, model):
    """an unknown prompt_pass names the keyword; D = 64 is not supported; a NULL pointer is invalid: no launch in any"""
    from easevoice_trainer_amd.hip import lib as L

    with pytest.raises(L.EvtError, match="prompt_pass = 'dense'"):
        model.decode_stream(_reqs(gpu, [0]), prompt_pass="dense")
    pack = PACKS["edges16"]
    qkv = _qkv(pack, torch.float32, gpu)
    rc, out, cache = _launch(qkv, pack, [[0], [1], [2], [3]], torch.float32, gpu, D=64)
    assert rc == L.EVT_ENOTSUP and (out == -7.0).all() and (cache[0] == 0xA5).all()
    d = _i32([0], gpu)
    rc = L.lib().evt_attn_prefixlm_packed_fwd(0, L.ptr(qkv), None, L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d), 0, 0,
                                            L.ptr(cache[0]), L.ptr(cache[1]), None, None, 2, 1, 1, 1, H, D, B, LMAX, XMAX,
                                            L.stream_ptr())
    assert rc == L.EVT_EINVAL


def _score(model, gpu, cd, **kw):
    g = torch.Generator().manual_seed(9)
    toks = [torch.randint(0, 1024, (10,), generator=g) for _ in range(4)]
    model.cd = cd
    try:
        got = dict(model.score_stream(_reqs(gpu, range(4)), toks, slots=4, **kw))
        return torch.stack([got[r][:, 0].cpu() for r in range(4)])
    finally:
        model.cd = torch.float32


@pytest.fixture(scope="module")
def parent(gpu, model):
    """the fp32 and the bf16 session on the default path (parent code): (lp32, d16)"""
    lp32 = _score(model, gpu, torch.float32)
    return lp32, float((_score(model, gpu, torch.bfloat16) - lp32).abs().mean())


@pytest.mark.parametrize("kv", [None, "mxfp8"])
def test_stream_gate(gpu, model, parent, kv):
    """mean |model log-prob - fp32 default session's|.  Default cache: the packed fp32 pass differs from the padded one by
    summation order alone, <= d16 / 16 (fp32 rounds 2^16 finer than bf16: a margin of 2^12); the packed bf16 session <= 2 d16.
    MXFP8 cache: the bound of its own gate, 32 d16.  Then n = 2 candidates and a forced request through the packed stream:
    token counts and slot bookkeeping of the default path"""
    lp32, d16 = parent
    assert d16 >= 1e-5, d16      # the gate is not vacuous
    d32p = float((_score(model, gpu, torch.float32, prompt_pass="packed", kv_dtype=kv) - lp32).abs().mean())
    if kv is not None:
        print(f"mean |d log-prob| against the fp32 session: packed pass + mxfp8 cache {d32p:.3e}, bf16 session d16 = {d16:.3e}")
        assert 0 < d32p <= 32 * d16, (d32p, d16)
        return
    d16p = float((_score(model, gpu, torch.bfloat16, prompt_pass="packed") - lp32).abs().mean())
    print(f"mean |d log-prob| against the fp32 session: packed fp32 {d32p:.3e}, packed bf16 {d16p:.3e}, bf16 session d16 = {d16:.3e}")
    assert d32p <= d16 / 16 and d16p <= 2 * d16, (d32p, d16p, d16)
    runs = []
    for pp in (None, "packed"):
        reqs = _reqs(gpu, [0, 1, 2])
        reqs[0][3]["n"], reqs[1][3]["force"] = 2, [5, 6, 7]
        outs = list(model.decode_stream(reqs, slots=3, top_k=15, top_p=1, early_stop_num=8, prompt_pass=pp))
        runs.append((sorted((o.request, o.candidate, len(o.y)) for o in outs), model._infer().stream_stats["events"],
                     {o.request: o.y for o in outs if o.candidate == 0}))
    assert runs[0][:2] == runs[1][:2] and len(runs[1][0]) == 4
    P = reqs[1][2].numel()
    assert runs[1][2][1][P:P + 3].tolist() == [5, 6, 7]
