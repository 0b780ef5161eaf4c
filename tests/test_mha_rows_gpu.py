"""evt_mha_rows_f32 (csrc/mha_rows.hip): the fp32 MFMA flash attention of the feature extractors on ragged rows, against
float64 softmax attention of each row alone.  Row lengths sit around the kernel's two tile sizes; everything at or behind a
row's length in q, k and v is NaN (or 1e30)."""
import ctypes as C
import math

import pytest
import torch

from easevoice_trainer_amd.hip.feat import MHA_ROWS_KEY_TILE as KT
from easevoice_trainer_amd.hip.feat import MHA_ROWS_QUERY_TILE as QT

pytestmark = pytest.mark.gpu
H = 3
QLENS = (1, QT - 1, QT, QT + 1, 2 * QT + 3, 1, 5)
KLENS = (1, 3, KT - 1, KT, KT + 1, 2 * KT + 5, 0)                     # the last item has no live key
NAN = float("nan")
CASES = pytest.mark.parametrize("D,layout,fill", [(32, "packed", NAN), (64, "planes", NAN), (64, "packed", 1e30),
                                                  (32, "planes", NAN)])
_DATA = {}


def _data(D, probe=False):
    """seeded q, k, v [B, max len, H * D] on the CPU and the float64 attention of each row alone, built once.  probe: q = 0 and
    small integer v, so that the exact result is the mean of v over the live keys"""
    if (D, probe) not in _DATA:
        g = torch.Generator().manual_seed(D + probe)
        q = torch.randn(len(QLENS), max(QLENS), H * D, generator=g) * (not probe)
        k = torch.randn(len(KLENS), max(KLENS), H * D, generator=g)
        v = torch.randint(-4, 5, k.shape, generator=g).float() if probe else torch.randn(k.shape, generator=g)
        refs = []
        for b, (nq, nk) in enumerate(zip(QLENS, KLENS)):
            qh, kh, vh = (t.double().view(-1, H, D).transpose(0, 1) for t in (q[b, :nq], k[b, :nk], v[b, :nk]))
            p = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(D), -1)
            ref = (p @ vh).transpose(0, 1).reshape(nq, H * D) if nk else torch.zeros(nq, H * D, dtype=torch.float64)
            if probe and nk:      # the mean itself, an exact integer sum and one division: p @ v leaves 1e-16 where it is 0
                ref = (v[b, :nk].double().sum(0) / nk).expand(nq, -1)
            refs.append(ref)
        _DATA[D, probe] = (q, k, v, refs)
    return _DATA[D, probe]


def _run(gpu, D, layout, fill, probe=False, order=None, pad=2, qlens=QLENS, klens=KLENS):
    """the batch (items in `order`, `fill` at and behind every length, `pad` rows of padding) through mha_rows_f32"""
    from easevoice_trainer_amd.hip.feat import mha_rows_f32

    q, k, v, _ = _data(D, probe)
    order = list(range(len(qlens))) if order is None else order
    Cc, B = H * D, len(order)
    tq, tk = max(QLENS) + pad, max(KLENS) + pad + (3 if layout == "planes" else 0)
    if layout == "packed":
        tq = tk = max(tq, tk)
        buf = torch.full((B, tq, 3 * Cc), fill)
        dq, dk, dv = buf[..., :Cc], buf[..., Cc:2 * Cc], buf[..., 2 * Cc:]
    else:
        dq, dk, dv = torch.full((B, tq, Cc), fill), torch.full((B, tk, Cc), fill), torch.full((B, tk, Cc), fill)
    for i, b in enumerate(order):
        dq[i, :qlens[b]], dk[i, :klens[b]], dv[i, :klens[b]] = q[b, :qlens[b]], k[b, :klens[b]], v[b, :klens[b]]
    if layout == "packed":
        buf = buf.to(gpu)
        dq, dk, dv = buf[..., :Cc], buf[..., Cc:2 * Cc], buf[..., 2 * Cc:]
    else:
        dq, dk, dv = dq.to(gpu), dk.to(gpu), dv.to(gpu)
    lq = torch.tensor([qlens[b] for b in order], dtype=torch.int32).to(gpu)
    lk = torch.tensor([klens[b] for b in order], dtype=torch.int32).to(gpu)
    with torch.no_grad():
        return mha_rows_f32(dq, dk, dv, lq, lk, H, D ** -0.5), (dq, dk, dv, lq, lk)


def _rel_err(out, refs, qlens=QLENS):
    err = max(float((out[b, :n].double().cpu() - refs[b]).abs().max()) for b, n in enumerate(qlens))
    return err / max(float(r.abs().max()) for r in refs)


@CASES
def test_mask_probe(gpu, D, layout, fill):
    out, _ = _run(gpu, D, layout, fill, probe=True)
    refs = _data(D, True)[3]
    assert torch.isfinite(out).all()
    for b, (nq, nk) in enumerate(zip(QLENS, KLENS)):
        got = out[b, :nq].double().cpu()
        assert ((got - refs[b]).abs() <= 2.0 ** -22 * refs[b].abs()).all(), (b, nq, nk)   # a 1-ulp reciprocal + two roundings
        assert not out[b, nq:].any() and (nk or not out[b].any()), (b, nq, nk)


@CASES
def test_parity_against_float64(gpu, D, layout, fill):
    from easevoice_trainer_amd.hip.enc import mha_core

    out, (dq, dk, dv, lq, lk) = _run(gpu, D, layout, fill)
    qz, kz, vz = (torch.nan_to_num(t, nan=0.0).contiguous() for t in (dq, dk, dv))
    with torch.no_grad():
        old = mha_core(qz, kz, vz, lq, lk, H, 0.0, 0, D ** -0.5)
    refs = _data(D)[3]
    new_err, old_err = _rel_err(out, refs), _rel_err(old, refs)
    print(f"D {D} {layout}: max-abs error / max|ref|  mha_rows_f32 {new_err:.3e}  evt_mha_fwd fp32 {old_err:.3e}")
    assert new_err <= 4 * old_err and new_err < 1e-3 and old_err < 1e-3


@CASES
def test_a_row_is_the_row_alone(gpu, D, layout, fill):
    from easevoice_trainer_amd.hip.feat import mha_rows_f32

    base, (dq, dk, dv, lq, lk) = _run(gpu, D, layout, fill)
    order = list(reversed(range(len(QLENS))))
    other, _ = _run(gpu, D, layout, 1e30 if fill != fill else NAN, order=order, pad=9)    # other neighbours, padding and fill
    for b, (nq, nk) in enumerate(zip(QLENS, KLENS)):
        assert torch.equal(other[order.index(b), :nq], base[b, :nq]), (b, nq, nk)
        if nk:
            with torch.no_grad():
                alone = mha_rows_f32(dq[b:b + 1, :nq], dk[b:b + 1, :nk], dv[b:b + 1, :nk], lq[b:b + 1], lk[b:b + 1], H, D ** -0.5)
            assert torch.equal(alone[0], base[b, :nq]), (b, nq, nk)


def test_cross_attention(gpu):
    from easevoice_trainer_amd.hip.enc import mha_core

    klens = KLENS[1:-1] + (KLENS[0], 7)                              # every query length meets another key length
    out, (dq, dk, dv, lq, lk) = _run(gpu, 64, "planes", NAN, klens=klens)
    assert dq.size(1) != dk.size(1)
    q, k, v, _ = _data(64)
    refs = []
    for b, (nq, nk) in enumerate(zip(QLENS, klens)):
        qh, kh, vh = (t.double().view(-1, H, 64).transpose(0, 1) for t in (q[b, :nq], k[b, :nk], v[b, :nk]))
        refs.append((torch.softmax(qh @ kh.transpose(1, 2) / 8.0, -1) @ vh).transpose(0, 1).reshape(nq, H * 64))
    with torch.no_grad():
        old = mha_core(*(torch.nan_to_num(t, nan=0.0) for t in (dq, dk, dv)), lq, lk, H, 0.0, 0, 0.125)
    new_err, old_err = _rel_err(out, refs), _rel_err(old, refs)
    print(f"cross: max-abs error / max|ref|  mha_rows_f32 {new_err:.3e}  evt_mha_fwd fp32 {old_err:.3e}")
    assert new_err <= 4 * old_err and new_err < 1e-3 and old_err < 1e-3


def test_refusals(gpu):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.feat import mha_rows_f32

    x, y = torch.randn(2, 40, 3 * 128 + 4, device=gpu), torch.randn(2, 40, 130, device=gpu)
    lens = torch.tensor([40, 7], dtype=torch.int32).to(gpu)
    q, k, v = x[..., :128], x[..., 128:256], x[..., 256:384]
    mha_rows_f32(q, k, v, lens, lens, 2, 0.125)
    for bad in (dict(q=x[..., :96], k=x[..., 128:224], v=x[..., 256:352]),                    # D = 48
                dict(q=q.bfloat16(), k=k.bfloat16(), v=v.bfloat16()), dict(q=x[..., 2:130]),  # 16 bit; rows 8 bytes off
                dict(q=y[..., :128]), dict(lens_k=lens.long())):                              # rows 520 bytes apart
        args = dict(q=q, k=k, v=v, lens_q=lens, lens_k=lens, n_heads=2, scale=0.125)
        args.update(bad)
        with pytest.raises(L.EvtError):
            mha_rows_f32(**args)
    out = torch.zeros(2, 40, 128, device=gpu)
    for kw in (dict(window=4), dict(dtype=1), dict(D=48), dict(ldq=x.stride(1) + 2), dict(dropout_p=0.1), dict(B=0)):
        f = dict(dtype=0, B=2, H=2, D=64, Tq=40, Tk=40, window=-1, n_heads_rel=1, ldq=x.stride(1), ldk=x.stride(1), ldo=128,
                 scale=0.125, dropout_p=0.0, site=0, pad_=0, seed_dev=None)
        f.update(kw)
        rc = L.lib().evt_mha_rows_f32(C.byref(L.MhaParams(**f)), q.data_ptr(), k.data_ptr(), v.data_ptr(), lens.data_ptr(),
                                      lens.data_ptr(), out.data_ptr(), L.stream_ptr())
        assert rc == L.EVT_EINVAL, kw
    torch.cuda.synchronize()
    assert not out.any()                                             # nothing was launched
