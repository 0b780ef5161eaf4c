"""GPU: Chinese-RoBERTa phone-level features on ragged batches of sentences -- the two ends of a group
(evt_phone_expand_rows, evt_bert_embed_ln_rows of csrc/feat_ops.hip), BertFeatures.hidden_rows /
phone_level_features_batch, FeatureWriter.text_batch and inference.text.fragment_bert_features.
The expander is checked bit for bit against torch indexing of the same rows; the embedding kernel against a float64
restatement, bounded by TWICE the error the unfused path (`_Embeddings.forward` through evt_add_layernorm_fwd) shows against
the same reference on the same inputs (the fused kernel rounds once where that path rounds three times); the model against
transformers' BertForMaskedLM on each sentence ALONE at the stage tolerances of test_feature_extractors_gpu.py (1e-3 of
max-abs in fp32, 6e-2 in 16-bit).

Measured on one MI355X (`_rel` = max-abs error over max-abs reference; the tests print these figures):
embedding kernel / unfused path against float64 at C = 1024: 1.27e-7 / 1.27e-7 in fp32, 2.74e-3 / 3.41e-3 in bf16, 3.46e-4 /
4.54e-4 in f16; at C = 72: 1.78e-7 / 1.75e-7, 3.47e-3 / 3.56e-3, 4.36e-4 / 4.44e-4.  Small model against transformers: 2.9e-7
in fp32, 7.0e-3 in bf16; against phone_level_feature: 2.5e-7, 8.4e-3 (not bit-identical).  BERT-large dimensions in bf16:
9.1e-3 and 1.2e-2."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = {torch.float32: 1e-3, torch.bfloat16: 6e-2, torch.float16: 6e-2}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _select(dtype):
    from easevoice_trainer_amd.hip import lib as L

    L.set_half(dtype)
    return L


# ---------------------------------------------------------------- expand kernel
EXP_T, EXP_B = 122, 4
SENTINEL, GUARD = 7777.0, 96


def _expand_case():
    """one call with every edge: items of 0 / 1 / 63 / 64 / 65 / 300 columns, zeros only, zh + zero + zh, counts of 0 and 5,
    two items over the same prompt rows, src entries outside the rows.  Sentence b's [CLS] is flat row b * T."""
    from easevoice_trainer_amd.feature_extractor.roberta import column_map

    T = EXP_T
    rs = np.random.RandomState(5)
    s0, s1, s2, s3 = 0 * T + 1, 1 * T + 1, 2 * T + 1, 3 * T + 1            # first character rows; 120 / 17 / 64 / 9 characters
    w300 = [5, 0, 3, 2] * 30
    w17 = rs.randint(0, 4, 17).tolist()
    w9 = rs.randint(1, 4, 9).tolist()
    items = [
        [],
        [("rows", s1 + 3, [1])],
        [("rows", s2, [1] * 63)],
        [("rows", s2, [1] * 64)],
        [("rows", s2, [1] * 63 + [2])],
        [("rows", s0, w300)],
        [("zero", 7)],
        [("rows", s1, w17), ("zero", 4), ("rows", s2, [2, 0, 1] * 10)],
        [("rows", s3, w9), ("rows", s1, w17)],
        [("rows", s3, w9), ("zero", 3)],
        [],
    ]
    src, item_off = column_map(items)
    sizes = np.diff(item_off).tolist()
    assert sizes[:7] == [0, 1, 63, 64, 65, 300, 7] and sizes[-1] == 0
    src = src.copy()
    o300 = int(item_off[5])
    src[o300 + 70], src[o300 + 71], src[o300 + 200] = -7, EXP_B * T + 3, EXP_B * T          # outside [-1, B * T): zero columns
    return src, item_off


def _expand_ref(h, src, item_off, out_dtype):
    Cc = h.size(-1)
    flat = h.reshape(-1, Cc)
    s = torch.from_numpy(src).long().to(h.device)
    ok = (s >= 0) & (s < flat.size(0))
    cols = torch.where(ok[:, None], flat[s.clamp(0, flat.size(0) - 1)], torch.zeros((), dtype=h.dtype, device=h.device))
    cols = cols.to(out_dtype)
    return torch.cat([cols[int(item_off[i]):int(item_off[i + 1])].T.reshape(-1) for i in range(len(item_off) - 1)])


def _expand_raw(L, h, src_d, off_d, n_items, total, buf):
    """the C entry on a caller's buffer: `buf` has GUARD elements in front of and behind the packed range"""
    B, T, Cc = h.shape
    rc = L.lib().evt_phone_expand_rows(
        L.dt_of(h), h.data_ptr(), B, T, Cc, src_d.data_ptr(), off_d.data_ptr(), n_items, total, L.dt_code(buf.dtype),
        buf.data_ptr() + GUARD * buf.element_size(), L.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("half_out", [False, True], ids=["out_f32", "out_16"])
@pytest.mark.parametrize("channels", [72, 1024])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_phone_expand_rows_bit_exact(gpu, dtype, channels, half_out):
    from easevoice_trainer_amd.hip.feat import phone_expand_rows

    L = _select(dtype)
    out_dtype = torch.float32 if not half_out else (L.half() if dtype == torch.float32 else dtype)
    _select(out_dtype)
    src, item_off = _expand_case()
    n_items, total = len(item_off) - 1, int(item_off[-1])
    g = torch.Generator().manual_seed(channels)
    h = torch.randn(EXP_B, EXP_T, channels, generator=g).to(dtype).to(gpu)
    src_d, off_d = torch.from_numpy(src).to(gpu), torch.from_numpy(item_off).to(gpu)
    ref = _expand_ref(h, src, item_off, out_dtype)
    sentinel = torch.tensor(SENTINEL, dtype=out_dtype)
    assert ref.numel() == channels * total and not bool((ref == sentinel.to(gpu)).any())
    buf = torch.full((GUARD + channels * total + GUARD,), SENTINEL, dtype=out_dtype, device=gpu)
    _expand_raw(L, h, src_d, off_d, n_items, total, buf)
    body = buf[GUARD:GUARD + channels * total]
    assert bool((buf[:GUARD] == sentinel.to(gpu)).all()) and bool((buf[-GUARD:] == sentinel.to(gpu)).all())
    assert torch.equal(_bits(body), _bits(ref))                  # every element written, as specified: no sentinel is left
    # the columns whose src lies outside the rows are zero
    o300, n300 = int(item_off[5]), 300
    item = body[channels * o300:channels * (o300 + n300)].view(channels, n300)
    assert not bool(item[:, [70, 71, 200]].any()) and bool(item[:, 72].any())
    # the binding: the same bits in its own tensor
    got = phone_expand_rows(h, src_d, off_d, n_items, total, out_dtype)
    assert got.dtype == out_dtype and got.shape == (channels * total,) and torch.equal(_bits(got), _bits(ref))
    # NaN and 1e30 in every token row that no column names (CLS, SEP, padding): not a bit changes
    flat_ok = (src >= 0) & (src < EXP_B * EXP_T)
    named = torch.zeros(EXP_B * EXP_T, dtype=torch.bool)
    named[torch.from_numpy(src[flat_ok]).long()] = True
    assert not named[0] and not named[EXP_T - 1] and not named[EXP_T + 19:2 * EXP_T].any()
    h2 = h.clone().view(-1, channels)
    poison = torch.where(torch.arange(EXP_B * EXP_T) % 2 == 0, float("nan"), 1e30)[:, None].expand(-1, channels)
    h2[~named.to(gpu)] = poison[~named].to(dtype).to(gpu)
    buf2 = torch.full_like(buf, SENTINEL)
    _expand_raw(L, h2.view_as(h), src_d, off_d, n_items, total, buf2)
    assert torch.equal(_bits(buf2), _bits(buf))


def test_phone_expand_rows_refuses_bad_arguments(gpu):
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.feat import phone_expand_rows

    h = torch.zeros(1, 4, 64, device=gpu)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=gpu)  # noqa: E731
    with pytest.raises(L.EvtError):
        phone_expand_rows(torch.zeros(1, 4, 60, device=gpu), i32([1]), i32([0, 1]), 1, 1)          # C % 8
    with pytest.raises(L.EvtError):
        phone_expand_rows(h, i32([1, 2]), i32([0, 1]), 1, 1)                                          # src of another size
    with pytest.raises(L.EvtError):
        phone_expand_rows(h, i32([1]).long(), i32([0, 1]), 1, 1)
    with pytest.raises(L.EvtError):
        phone_expand_rows(torch.zeros(2, 4, 64, device=gpu).transpose(0, 1), i32([1]), i32([0, 1]), 1, 1)   # not contiguous
    empty = phone_expand_rows(h, i32([]), i32([0, 0, 0]), 2, 0)                                       # items without columns
    assert empty.numel() == 0


# ---------------------------------------------------------------- embedding kernel
EMB_B, EMB_T, EMB_LENS, EMB_VOCAB, EMB_POS, EMB_EPS = 3, 40, (2, 19, 40), 300, 64, 1e-12
_EMB = {}


def _embed_case(channels):
    """tables, ids and the float64 reference, built once per width"""
    if channels not in _EMB:
        g = torch.Generator().manual_seed(100 + channels)
        word = torch.randn(EMB_VOCAB, channels, generator=g)
        pos = 0.5 * torch.randn(EMB_POS, channels, generator=g)
        typ = 0.5 * torch.randn(2, channels, generator=g)
        word[:, 7] = 30.0 + 0.1 * torch.randn(EMB_VOCAB, generator=g)       # one channel with a mean 300 x its deviation
        gamma = 1 + 0.1 * torch.randn(channels, generator=g)
        beta = 0.05 * torch.randn(channels, generator=g)
        ids = torch.randint(0, EMB_VOCAB, (EMB_B, EMB_T), generator=g, dtype=torch.int32)
        tt = torch.randint(0, 2, (EMB_B, EMB_T), generator=g, dtype=torch.int32)
        v = word.double()[ids.long()] + pos.double()[:EMB_T][None] + typ.double()[tt.long()]
        mean, var = v.mean(-1, keepdim=True), v.var(-1, unbiased=False, keepdim=True)
        ref = (v - mean) / torch.sqrt(var + EMB_EPS) * gamma.double() + beta.double()
        _EMB[channels] = dict(word=word, pos=pos, typ=typ, gamma=gamma, beta=beta, ids=ids, tt=tt, ref=ref)
    return _EMB[channels]


def _live_err(out, ref):
    """max-abs error over the live rows, over the max-abs of the reference's live rows"""
    num = den = 0.0
    for b, n in enumerate(EMB_LENS):
        num = max(num, float((out[b, :n].double().cpu() - ref[b, :n]).abs().max()))
        den = max(den, float(ref[b, :n].abs().max()))
    return num / den


@pytest.mark.parametrize("channels", [1024, 72])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bert_embed_ln_rows(gpu, dtype, channels):
    from easevoice_trainer_amd.feature_extractor.roberta import _Embeddings
    from easevoice_trainer_amd.hip.feat import bert_embed_ln_rows

    _select(dtype)
    c = _embed_case(channels)
    d = {k: v.to(gpu) for k, v in c.items() if k != "ref"}
    lens = torch.tensor(EMB_LENS, dtype=torch.int32, device=gpu)
    tables = (d["word"], d["pos"], d["typ"], d["gamma"], d["beta"], EMB_EPS, dtype)
    out = bert_embed_ln_rows(d["ids"], lens, *tables, token_type_ids=d["tt"])
    assert out.shape == (EMB_B, EMB_T, channels) and out.dtype == dtype
    # the unfused path on the same inputs: three gathers, the add, two casts and evt_add_layernorm_fwd
    emb = _Embeddings(EMB_VOCAB, channels, EMB_POS, 2, EMB_EPS).to(gpu)
    with torch.no_grad():
        emb.word_embeddings.weight.copy_(d["word"])
        emb.position_embeddings.weight.copy_(d["pos"])
        emb.token_type_embeddings.weight.copy_(d["typ"])
        emb.LayerNorm.weight.copy_(d["gamma"])
        emb.LayerNorm.bias.copy_(d["beta"])
        parent = emb(d["ids"].long(), d["tt"].long(), dtype)
    err, err_parent = _live_err(out, c["ref"]), _live_err(parent, c["ref"])
    print(f"embed C={channels} {dtype}: fused {err:.3e}, unfused {err_parent:.3e}")
    assert err <= 2 * err_parent, (err, err_parent)
    # rows behind a sentence's length are exactly zero
    for b, n in enumerate(EMB_LENS):
        assert not bool(out[b, n:].any()) and bool(out[b, :n].any())
    # a row alone, with T = its length: bit for bit the row of the batch
    for b, n in enumerate(EMB_LENS):
        alone = bert_embed_ln_rows(d["ids"][b:b + 1, :n].contiguous(), lens[b:b + 1].contiguous(), *tables,
                                   token_type_ids=d["tt"][b:b + 1, :n].contiguous())
        assert torch.equal(_bits(alone[0]), _bits(out[b, :n]))
    # other valid ids (and types) in the padding change nothing
    ids2, tt2 = d["ids"].clone(), d["tt"].clone()
    for b, n in enumerate(EMB_LENS):
        ids2[b, n:] = (ids2[b, n:] + 17) % EMB_VOCAB
        tt2[b, n:] = 1 - tt2[b, n:]
    assert torch.equal(_bits(bert_embed_ln_rows(ids2, lens, *tables, token_type_ids=tt2)), _bits(out))
    # ids outside the table are clamped on the device: vocab + 5 is the last row, a negative id the first
    ids3 = d["ids"].clone()
    ids3[1, 4], ids3[2, 9] = EMB_VOCAB + 5, -3
    ids4 = ids3.clone()
    ids4[1, 4], ids4[2, 9] = EMB_VOCAB - 1, 0
    o3, o4 = bert_embed_ln_rows(ids3, lens, *tables, token_type_ids=d["tt"]), bert_embed_ln_rows(ids4, lens, *tables, token_type_ids=d["tt"])
    assert torch.equal(_bits(o3), _bits(o4)) and bool(torch.isfinite(o3.float()).all())
    assert not torch.equal(_bits(o3[1, 4]), _bits(out[1, 4]))
    # no token types = all zero
    zero_tt = bert_embed_ln_rows(d["ids"], lens, *tables, token_type_ids=torch.zeros_like(d["tt"]))
    assert torch.equal(_bits(bert_embed_ln_rows(d["ids"], lens, *tables)), _bits(zero_tt))


# ---------------------------------------------------------------- the model
SMALL = dict(vocab=512, hidden=128, heads=2, inner=512, num_layers=4, read_layer=2)
_HF = {}


def _hf_bert(key, **cfg):
    """a seeded random BertForMaskedLM with shifted LayerNorm weights and biases (test_feature_extractors_gpu.py's
    construction), built once"""
    if key not in _HF:
        from transformers import BertConfig, BertForMaskedLM

        torch.manual_seed(1)
        hf = BertForMaskedLM(BertConfig(max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, **cfg)).eval()
        with torch.no_grad():
            for n, p in hf.named_parameters():
                if n.endswith("LayerNorm.weight"):
                    p.add_(0.1 * torch.randn_like(p))
                elif n.endswith(".bias"):
                    p.add_(0.05 * torch.randn_like(p))
        _HF[key] = hf
    return _HF[key]


def _hf_small():
    return _hf_bert("small", vocab_size=512, hidden_size=128, num_hidden_layers=4, num_attention_heads=2, intermediate_size=512)


def _hf_feature(hf, ids, word2ph):
    """normalize.py:88-105 on one sentence alone"""
    ids = torch.as_tensor(ids).long().view(1, -1)
    with torch.no_grad():
        res = hf(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids),
                 output_hidden_states=True)["hidden_states"][-3][0, 1:-1]
    return torch.repeat_interleave(res, torch.as_tensor(word2ph, dtype=torch.long), dim=0).T


def _sentences(seed, chars, vocab=512, low=0):
    g = torch.Generator().manual_seed(seed)
    ids = [torch.randint(5, vocab, (n + 2,), generator=g) for n in chars]
    word2ph = [torch.randint(low, 4, (n,), generator=g).tolist() for n in chars]
    return ids, word2ph


_SMALL_REF = {}


def _small_refs():
    """the four sentences of the model tests and transformers' features of each alone, computed once"""
    if not _SMALL_REF:
        ids, word2ph = _sentences(4, (1, 17, 120, 17))
        _SMALL_REF.update(ids=ids, word2ph=word2ph, ref=[_hf_feature(_hf_small(), a, w) for a, w in zip(ids, word2ph)])
    return _SMALL_REF


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def small(request, gpu):
    from easevoice_trainer_amd.feature_extractor import BertFeatures

    return BertFeatures(_hf_small().state_dict(), gpu, request.param, **SMALL)


def test_batch_matches_transformers_on_each_sentence_alone(gpu, small):
    r = _small_refs()
    tol = TOL[small.dtype]
    got = small.phone_level_features_batch(r["ids"], r["word2ph"], group=3)             # two groups, re-ordered
    assert len(got) == 4
    print(f"{small.dtype}: batch against transformers alone: {max(_rel(g, ref) for g, ref in zip(got, r['ref'])):.3e}")
    for k, (g, ref) in enumerate(zip(got, r["ref"])):
        assert g.shape == ref.shape == (128, sum(r["word2ph"][k])) and g.dtype == torch.float32 and g.device.type == "cpu"
        assert _rel(g, ref) < tol, (k, _rel(g, ref))
    dev = small.phone_level_features_batch(r["ids"], r["word2ph"], group=3, device_out=True)
    for g, d in zip(got, dev):
        assert d.device == gpu and torch.equal(d.cpu(), g)
    half = small.phone_level_features_batch(r["ids"], r["word2ph"], group=3, out_dtype=small.rt.dtype, device_out=True)
    for g, d in zip(dev, half):
        assert d.dtype == small.dtype and torch.equal(d, g.to(small.dtype))
    # the one-sentence path on the same sentences
    same, worst = True, 0.0
    for k, g in enumerate(got):
        one = small.phone_level_feature(r["ids"][k].view(1, -1), r["word2ph"][k])
        assert one.shape == g.shape and _rel(g, one) < tol, (k, _rel(g, one))
        same, worst = same and torch.equal(one, g), max(worst, _rel(g, one))
    print(f"{small.dtype}: batch equals phone_level_feature bit for bit: {same} (largest difference {worst:.3e})")
    # hidden_rows: shape, lengths
    h, lens = small.hidden_rows(r["ids"])
    assert h.shape == (4, 122, 128) and h.dtype == small.dtype and list(lens) == [3, 19, 122, 19]


def test_hidden_rows_do_not_depend_on_the_neighbours(gpu, small):
    """two groups with the same longest sentence length and different neighbours: a sentence's live rows are bit-identical,
    because padded keys are excluded (not weighted down) and every row-wise launch treats rows apart"""
    ids, _ = _sentences(9, (17, 38, 38, 5))
    a, long1, long2, short = ids
    h1, _ = small.hidden_rows([a, long1])
    h2, _ = small.hidden_rows([a, long2])
    assert h1.shape == h2.shape == (2, 40, 128) and not torch.equal(h1[1], h2[1])
    assert torch.equal(_bits(h1[0, :19]), _bits(h2[0, :19]))
    h3, _ = small.hidden_rows([long2, a])                                                # another row of the group
    assert torch.equal(_bits(h3[1, :19]), _bits(h1[0, :19])) and torch.equal(_bits(h3[0]), _bits(h2[1]))
    h4, _ = small.hidden_rows([short, long1])
    assert torch.equal(_bits(h4[1]), _bits(h1[1]))


def test_bert_large_dimensions_bf16(gpu):
    """the shipped shape through both new kernels once: hidden 1024, 16 heads, 22 of 24 layers"""
    from easevoice_trainer_amd.feature_extractor import BertFeatures

    hf = _hf_bert("large", vocab_size=2048, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                  intermediate_size=4096)
    ours = BertFeatures(hf.state_dict(), gpu, torch.bfloat16, vocab=2048)
    ids, word2ph = _sentences(6, (5, 30), vocab=2048)
    got = ours.phone_level_features_batch(ids, word2ph)
    for k, g in enumerate(got):
        ref = _hf_feature(hf, ids[k], word2ph[k])
        print(f"BERT-large bf16, {ids[k].numel() - 2} characters: {_rel(g, ref):.3e}")
        assert g.shape == ref.shape == (1024, sum(word2ph[k])) and _rel(g, ref) < 6e-2, (k, _rel(g, ref))
    _HF.pop("large")


# ---------------------------------------------------------------- writers and helper
def test_text_batch_against_text(gpu, small, tmp_path, monkeypatch):
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter

    ids, word2ph = _sentences(12, (6, 1, 33, 9, 14), low=1)
    lang = ["zh", "zh", "en", "zh", "zh"]
    names = ["a.wav", "b.wav", "c.wav", "have.wav", "d.wav"]
    items = [(names[i], ["p"] * sum(word2ph[i]), word2ph[i], "text %d" % i, lang[i], ids[i].view(1, -1)) for i in range(5)]
    dirs = [tmp_path / "one", tmp_path / "batch"]
    writers = [FeatureWriter(str(d), None, small) for d in dirs]
    for d in dirs:
        torch.save(torch.zeros(1), d / "3-bert" / "have.wav.pt")
    for it in items:
        writers[0].text(*it)
    writers[1].text_batch(items, group=2)
    for w in writers:
        w.close()
    assert sorted(os.listdir(dirs[0] / "3-bert")) == sorted(os.listdir(dirs[1] / "3-bert")) == \
        ["a.wav.pt", "b.wav.pt", "d.wav.pt", "have.wav.pt"]
    for name in ("a.wav.pt", "b.wav.pt", "d.wav.pt"):
        one, batch = torch.load(dirs[0] / "3-bert" / name), torch.load(dirs[1] / "3-bert" / name)
        assert batch.dtype == torch.float32 and batch.device.type == "cpu" and batch.shape == one.shape
        assert _rel(batch, one) < TOL[small.dtype], (name, _rel(batch, one))
    assert open(dirs[0] / "2-name2text.txt", "rb").read() == open(dirs[1] / "2-name2text.txt", "rb").read()
    with pytest.raises(ValueError, match="bert_feature and phones not match"):
        FeatureWriter(str(tmp_path / "bad"), None, small).text_batch([("x.wav", ["p"], word2ph[0], "t", "zh", ids[0])])
    # an existing file and an `en` item: skipped without a pass of the model
    calls = []
    monkeypatch.setattr(small, "hidden_rows", lambda *a, **k: calls.append(a), raising=False)
    w = FeatureWriter(str(dirs[1]), None, small)
    w.text_batch([items[2], items[3], items[0]])
    assert not calls and len(w._text_lines) == 3


def _host_assembly(bert, segments):
    """the reference's own assembly (tts.py:508-531) from phone_level_feature outputs: cat over the segments, torch.zeros
    for the others"""
    parts = [bert.phone_level_feature(torch.as_tensor(s[1]).view(1, -1), s[2]) if s[0] == "zh" else torch.zeros(bert.hidden_size, s[1])
             for s in segments]
    return torch.cat(parts, 1) if parts else torch.zeros(bert.hidden_size, 0)


def test_fragment_bert_features_against_host_assembly(gpu, small):
    from easevoice_trainer_amd.inference.text import fragment_bert_features

    ids, word2ph = _sentences(21, (7, 12, 3, 40, 9, 5))
    zh = lambda k: ("zh", ids[k], word2ph[k])  # noqa: E731
    prompt_a, prompt_b = [zh(0), ("zero", 3)], [("zero", 2), zh(5)]
    frags = [[zh(1)], [("zero", 6)], [zh(2), ("zero", 4), zh(3)], [zh(4), ("zero", 0)]]
    cases = {"shared": (prompt_a, [prompt_a] * 4), "per fragment": ([prompt_a, prompt_b, [], prompt_a], [prompt_a, prompt_b, [], prompt_a]),
             "none": (None, [[]] * 4)}
    tol = TOL[small.dtype]
    for name, (prompt, per) in cases.items():
        got = fragment_bert_features(small, frags, prompt, group=3)
        assert len(got) == 4
        for f, g in enumerate(got):
            segs = list(per[f]) + frags[f]
            want = _host_assembly(small, segs)
            assert g.device == gpu and g.dtype == torch.float32 and g.shape == want.shape, (name, f)
            # the zero segments are exactly zero and sit where the reference puts them; the rest agrees column by column
            o = 0
            for s in segs:
                n = s[1] if s[0] == "zero" else sum(s[2])
                if s[0] == "zero":
                    assert not bool(g[:, o:o + n].any()), (name, f)
                o += n
            assert o == g.size(1) and _rel(g, want) < tol, (name, f, _rel(g, want))
    half = fragment_bert_features(small, frags, prompt_a, out_dtype=small.dtype)
    full = fragment_bert_features(small, frags, prompt_a)
    for a, b in zip(half, full):
        assert a.dtype == small.dtype and torch.equal(a, b.to(small.dtype))


def test_fragment_features_decode_to_the_same_tokens(gpu):
    """the [1024, n] of one fragment with a prompt, fed to the s1 decoder (random-initialised, as the stream tests build
    it): the tokens that the host-assembled features give"""
    import yaml

    from easevoice_trainer_amd.feature_extractor import BertFeatures
    from easevoice_trainer_amd.inference.text import fragment_bert_features
    from easevoice_trainer_amd.train.s1_engine import S1Engine
    from util_fill import fill_module

    torch.manual_seed(2)
    bert = BertFeatures(None, gpu, torch.float32, vocab=512, hidden=1024, heads=16, inner=512, num_layers=2, read_layer=2)
    ids, word2ph = _sentences(31, (6, 11), low=1)
    prompt, frag = [("zh", ids[0], word2ph[0])], [("zh", ids[1], word2ph[1]), ("zero", 3)]
    dev = fragment_bert_features(bert, [frag], prompt)[0]
    host = _host_assembly(bert, prompt + frag)
    assert dev.shape == host.shape and _rel(dev, host) < 1e-3
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    eng = S1Engine(cfg, gpu, torch.float32)
    fill_module(eng.model, 3)
    eng.model.eval()
    g = torch.Generator().manual_seed(8)
    n = dev.size(1)
    x = torch.randint(0, 732, (n,), generator=g).to(gpu)
    prompts = torch.randint(0, 1024, (1, 12), generator=g).to(gpu)
    kw = dict(top_k=15, top_p=1, early_stop_num=12, seed=4242)
    with torch.no_grad():
        y1, i1 = eng.model.infer_panel_batch_infer([x], torch.tensor([n]).to(gpu), prompts, [dev], **kw)
        y2, i2 = eng.model.infer_panel_batch_infer([x], torch.tensor([n]).to(gpu), prompts, [host.to(gpu)], **kw)
    assert i1 == i2 and torch.equal(y1[0], y2[0]) and y1[0].numel() > 12
