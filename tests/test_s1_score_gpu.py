"""GPU: teacher-forced scoring in one pass (csrc/s1_score.hip, score_stream(prompt_pass="teacher")): evt_score_rows against
a float64 reference built from oracle/s1_step.py::logits_to_probs, a launch against its sequences launched alone (bits),
and score_stream's teacher pass against its stepped path on the small seeded model."""
import pytest
import torch

from oracle.s1_step import logits_to_probs
from test_s1_kv_mx8_gpu import _reqs
from test_s1_stream_gpu import _i32, model  # noqa: F401  (the small seeded model of the stream tests)

pytestmark = pytest.mark.gpu
SEQS = [(0, 1), (3, 16), (5, 17), (0, 33)]          # (P, f): one position, exactly a tile, a tile plus one, three tiles
TABLES = {"k15": [(15, 1.0, 1.0, 1.35)] * 4, "nucleus": [(5, 0.8, 0.7, 1.35)] * 4, "off": [(0, 1.0, 1.0, 1.0)] * 4,
          "mixed": [(15, 1.0, 1.0, 1.35), (5, 0.8, 0.7, 1.35), (0, 1.0, 1.0, 1.0), (3, 0.6, 1.3, 0.8)],
          "k3": [(3, 1.0, 1.0, 1.35)] * 4}
# (512, 1025): the model; (64, 35): one K slice, three column tiles -- under every table of the issue.  (80, 35): a K tail;
# (1024, 2048): K chunks and 32 logits a lane -- other paths of the logits phase only, under the two tables whose cuts stay
# clear of 4 delta at that E (delta grows with E, the gaps between sorted logits shrink with V)
CASES = [(E, V, t) for E, V in ((512, 1025), (64, 35)) for t in ("k15", "nucleus", "off", "mixed")] + \
        [(E, V, t) for E, V in ((80, 35), (1024, 2048)) for t in ("k3", "off")]
# the seed was chosen on the CPU, from the float64 reference alone, so that no case below has more than 2 % of its 67
# positions within 4 delta of a cut (the only positions whose [1] may be skipped)
SEED = 7


def _case(E, V, dtype):
    """h [T][E] with unused rows between the sequences, Wp, the histories.  Logits of one sign pattern per column
    (h >= 0, Wp[v] = a_v |noise|), so that sum |h w| is |logit| and delta small against the gaps: 16 head columns 0.3 apart,
    the rest far below.  Tokens: half of them head columns; an EOS among the given tokens of the last sequence below and
    above step 11, one token outside [0, V) in the third"""
    g = torch.Generator().manual_seed(SEED)
    row0, t = [], 2
    for _P, f in SEQS:
        row0.append(t)
        t += f + 1
    h = torch.randn(t, E, generator=g).abs().to(dtype)
    head = torch.randperm(V - 1, generator=g)[:16]
    a = -4.5 + 0.5 * torch.randn(V, generator=g)
    a[head] = 3.5 - 0.3 * torch.arange(16) + 0.2 * (torch.rand(16, generator=g) - 0.5)
    Wp = (a[:, None] * torch.randn(V, E, generator=g).abs() / (0.6366 * E)).to(dtype)
    hist = [torch.where(torch.rand(P + f, generator=g) < 0.5, head[torch.randint(0, 16, (P + f,), generator=g)],
                        torch.randint(0, V - 1, (P + f,), generator=g)) for P, f in SEQS]
    hist[3][5], hist[3][20], hist[2][5 + 7] = V - 1, V - 1, V + 5
    return h, Wp, hist, row0


def _launch(h, Wp, hist, row0, seqs, tabs, no_eos, gpu):
    from easevoice_trainer_amd.hip import lib as L

    V, f = Wp.size(0), [f for _P, f in seqs]
    hist0 = [sum(p + n for p, n in seqs[:s]) for s in range(len(seqs))]
    tiles = [v for s, n in enumerate(f) for i0 in range(0, n, 16) for v in (s, i0)]
    tab = torch.tensor([[0.0, *t[1:]] for t in tabs])
    tab.view(torch.int32)[:, 0] = torch.tensor([t[0] for t in tabs], dtype=torch.int32)
    dev = [_i32(v, gpu) for v in (torch.cat(hist).tolist(), hist0, row0, [p for p, _n in seqs], f)]
    tab, tiles_d, hd, Wd = tab.to(gpu), _i32(tiles, gpu), h.to(gpu), Wp.to(gpu)
    out = torch.full((sum(f), 2), 7.0, device=gpu)
    rc = L.lib().evt_score_rows(L.dt_of(hd), L.ptr(hd), L.ptr(Wd), *map(L.ptr, dev), L.ptr(tab), L.ptr(tiles_d), L.ptr(out),
                                V - 1, no_eos, len(seqs), len(tiles) // 2, hd.size(0), hd.size(1), V, dev[0].numel(),
                                out.size(0), L.stream_ptr())
    assert rc == 0
    return out.cpu()


def _reference(h, Wp, hist, row0, tabs, no_eos):
    """per position: ([0], [1]) in float64, delta = E 2^-24 max_v sum_k |h_k w_vk|, and whether a cut lies within 4 delta"""
    E, V, rows, Wd = h.size(1), Wp.size(0), [], Wp.double()
    for (P, f), hs, r0, (top_k, top_p, temp, rp) in zip(SEQS, hist, row0, tabs):
        for i in range(f):
            x, tok = h[r0 + i].double(), int(hs[P + i])
            Ve = V - 1 if i < no_eos else V
            delta = float(E * 2.0 ** -24 * (Wd.abs() @ x.abs()).max())
            lg = (Wd @ x)[None, :Ve]
            prev = hs[:P + i]
            prev = prev[prev < Ve][None]
            pr = logits_to_probs(lg, prev, temp, top_k if top_k > 0 else None, top_p, rp)
            cur = lg.clone()                        # the penalised logits once more, for the distances to the two cuts
            if prev.numel() and rp != 1.0:
                sc = torch.gather(cur, 1, prev)
                cur.scatter_(1, prev, torch.where(sc < 0, sc * rp, sc / rp))
            srt = torch.sort(cur[0], descending=True)[0]
            amb = top_p < 1.0 and bool(((torch.cumsum(torch.softmax(srt, 0), 0) - top_p).abs() < 4 * delta).any())
            kk = min(top_k, Ve)
            amb = amb or (0 < kk < Ve and float(srt[kk - 1] - srt[kk]) < 4 * delta)
            ok = 0 <= tok < V
            nan, ninf = float("nan"), float("-inf")
            r = (float(torch.log_softmax(lg, 1)[0, tok]), float(torch.log(pr[0, tok]))) if ok and tok < Ve else \
                (ninf, ninf) if ok else (nan, nan)
            rows.append((*r, delta, amb))
    return torch.tensor(rows, dtype=torch.float64)


@pytest.mark.parametrize("no_eos", [0, 11])
@pytest.mark.parametrize("E,V,table", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "h16"])
def test_score_rows_against_float64(gpu, dtype, E, V, table, no_eos):
    """|[0] - ref| <= 2 delta + 1e-5 everywhere; [1] likewise wherever no cut of the reference lies within 4 delta (at most
    2 % of the positions are skipped for that); -inf and NaN in the same places; then every sequence launched alone: the
    same bits"""
    h, Wp, hist, row0 = _case(E, V, dtype)
    tabs = [(V, 1.0, 1.0, 1.0)] * 4 if table == "off" else TABLES[table]
    got = _launch(h, Wp, hist, row0, SEQS, tabs, no_eos, gpu).double()
    ref = _reference(h, Wp, hist, row0, tabs, no_eos)
    bound, amb = 2 * ref[:, 2] + 1e-5, ref[:, 3] > 0
    assert amb.sum() <= 0.02 * len(ref), int(amb.sum())
    for c, keep in ((0, torch.ones_like(amb)), (1, ~amb)):
        a, b = got[keep, c], ref[keep, c]
        fin = torch.isfinite(b)
        print(f"[{c}] max |got - ref| = {float((a - b)[fin].abs().max()):.3e}, smallest bound {float(bound.min()):.3e}")
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a == float("-inf"), b == float("-inf"))
        assert ((a - b)[fin].abs() <= bound[keep][fin]).all()
    assert torch.isnan(got[17 + 7]).all() and (got[34 + 5, 0] == float("-inf")) == (no_eos > 5)
    at = 0
    for s, (P, f) in enumerate(SEQS):
        alone = _launch(h, Wp, hist[s:s + 1], row0[s:s + 1], SEQS[s:s + 1], tabs[s:s + 1], no_eos, gpu).double()
        assert torch.equal(alone.view(torch.int64), got[at:at + f].view(torch.int64)), s
        at += f


# the largest |teacher - stepped| over both values of every position below, measured on an MI355X (3.338e-06 with and
# without append_eos); the two paths differ by summation order alone, and 4x that is allowed for the pool's variance of
# nothing else
TEACHER_VS_STEPPED = 3.338e-6


@pytest.mark.parametrize("append_eos", [False, True])
def test_teacher_pass_against_stepped_path(gpu, model, append_eos, monkeypatch):
    """fp32, four requests of different lengths, one with cuts of its own: the teacher pass against the steps of
    prompt_pass="packed"; then the same requests in groups of at most 60 packed rows: no bit changes"""
    from easevoice_trainer_amd.auto_reg.t2s_infer import T2SInfer

    g = torch.Generator().manual_seed(11)
    toks = [torch.randint(0, 1024, (n,), generator=g) for n in (5, 16, 17, 33)]
    reqs = _reqs(gpu, range(4))
    reqs[3][3].update(top_k=900, top_p=0.999)
    kw = dict(slots=4, append_eos=append_eos, temperature=0.8)
    step = dict(model.score_stream(reqs, toks, prompt_pass="packed", **kw))
    one = list(model.score_stream(reqs, toks, prompt_pass="teacher", **kw))
    assert [r for r, _lp in one] == [0, 1, 2, 3]
    a, b = torch.cat([lp for _r, lp in one]).cpu(), torch.cat([step[r] for r in range(4)]).cpu()
    fin = torch.isfinite(b)
    d = float((a - b)[fin].abs().max())
    print(f"append_eos={append_eos}: max |teacher - stepped| = {d:.3e} over {int(fin.sum())} finite of {b.numel()} values")
    assert a.shape == (sum(t.numel() + append_eos for t in toks), 2) and fin.sum() > 0.9 * b.numel()
    assert torch.equal(a[~fin], b[~fin]) and d <= 4 * TEACHER_VS_STEPPED
    monkeypatch.setattr(T2SInfer, "TEACHER_ROWS", 60)
    split = torch.cat([lp for _r, lp in model.score_stream(reqs, toks, prompt_pass="teacher", **kw)]).cpu()
    assert torch.equal(split.view(torch.int32), a.view(torch.int32))
