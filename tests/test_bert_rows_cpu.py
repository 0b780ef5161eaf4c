"""Host side of Chinese-RoBERTa on ragged batches of sentences (no GPU): the column-map builder of
hip/feat.py::phone_expand_rows against np.repeat, the length sorting / grouping of
BertFeatures.phone_level_features_batch with a fake encoder, the mismatch errors and that they come before any upload,
FeatureWriter.text_batch's skip logic and file formats with a fake `bert`, the plan of
inference.text.fragment_bert_features, and the C ABI of the two new entry points in both builds of the library."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _expand_host(h, src, item_off, out_dtype=torch.float32):
    """what evt_phone_expand_rows is defined to write, with torch indexing on the host"""
    C = h.size(-1)
    flat = h.reshape(-1, C)
    src_t = torch.from_numpy(np.asarray(src)).long()
    cols = torch.where((src_t >= 0)[:, None], flat[src_t.clamp(min=0)], torch.zeros(1, C, dtype=h.dtype)).to(out_dtype)
    return torch.cat([cols[int(item_off[i]):int(item_off[i + 1])].T.reshape(-1) for i in range(len(item_off) - 1)]
                     + [torch.zeros(0, dtype=out_dtype)])


def test_column_map_against_np_repeat():
    from easevoice_trainer_amd.feature_extractor.roberta import column_map

    rs = np.random.RandomState(0)
    w_a = rs.randint(0, 4, 17).tolist()                   # zeros among the counts
    w_b = [0, 5, 0, 0, 2]
    w_p = rs.randint(1, 4, 9).tolist()                    # the shared prompt's sentence: rows 300 ..
    items = [
        [("rows", 1, w_a)],                                                    # a plain sentence
        [],                                                                    # an empty item
        [("zero", 7)],                                                         # zero columns only
        [("rows", 300, w_p), ("rows", 123, w_b), ("zero", 3), ("rows", 1, w_a)],   # shared prompt + zh + zero + zh
        [("rows", 300, w_p), ("zero", 0), ("rows", 123, [0, 0, 0])],           # the same prompt rows again; nothing behind them
        [("rows", 300, w_p)],
    ]
    src, item_off = column_map(items)
    assert src.dtype == np.int32 and item_off.dtype == np.int32
    rep = lambda first, w: np.repeat(np.arange(first, first + len(w)), w)  # noqa: E731
    want = [rep(1, w_a), np.zeros(0), np.full(7, -1),
            np.concatenate([rep(300, w_p), rep(123, w_b), np.full(3, -1), rep(1, w_a)]), rep(300, w_p), rep(300, w_p)]
    assert item_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert np.array_equal(src, np.concatenate(want).astype(np.int32))
    assert item_off[2] == item_off[1] and item_off[-1] == len(src)
    # nothing at all
    src, item_off = column_map([[], []])
    assert src.size == 0 and item_off.tolist() == [0, 0, 0]
    for bad in ([[("rows", 0, [1, -1])]], [[("zero", -2)]], [[("other", 3)]]):
        with pytest.raises(ValueError):
            column_map(bad)


class _FakeEncoder:
    """BertFeatures without a model: hidden row (b, t) = its id in channel 0, 1000 * t + c in channel c > 0"""
    C = 8

    def __init__(self):
        self.groups, self.uploads = [], 0

    def make(self):
        from easevoice_trainer_amd.feature_extractor.roberta import BertFeatures

        class Fake(BertFeatures):
            hidden_size, device = self.C, torch.device("cpu")

        bert = Fake.__new__(Fake)
        bert.hidden_rows = self.hidden_rows
        bert._expand = self.expand
        return bert

    def hidden_rows(self, ids_list):
        lens = [len(a) for a in ids_list]
        self.groups.append(lens)
        h = torch.full((len(ids_list), max(lens), self.C), float("nan"))
        for b, a in enumerate(ids_list):
            t = torch.arange(len(a), dtype=torch.float32)
            h[b, :len(a)] = 1000 * t[:, None] + torch.arange(self.C, dtype=torch.float32)[None]
            h[b, :len(a), 0] = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        return h, lens

    def expand(self, h, src, item_off, out_dtype):
        self.uploads += 1
        return _expand_host(h, src, item_off, out_dtype)

    def want(self, ids, word2ph):
        ids = np.asarray(ids)
        rows = torch.stack([torch.cat([torch.tensor([float(ids[t])]), 1000.0 * t + torch.arange(1, self.C)])
                            for t in range(1, len(ids) - 1)]) if len(ids) > 2 else torch.zeros(0, self.C)
        return torch.repeat_interleave(rows, torch.as_tensor(word2ph, dtype=torch.long), dim=0).T


def _sentences(seed, chars):
    rs = np.random.RandomState(seed)
    ids = [rs.randint(5, 500, n + 2).astype(np.int64) for n in chars]
    word2ph = [rs.randint(0, 4, n).tolist() for n in chars]
    return ids, word2ph


@pytest.mark.parametrize("group", [1, 2, 3, 4, 5])
def test_batch_sorts_groups_and_returns_input_order(group):
    chars = [9, 3, 30, 1, 3, 17, 12]
    ids, word2ph = _sentences(1, chars)
    fake = _FakeEncoder()
    got = fake.make().phone_level_features_batch([torch.from_numpy(a) for a in ids], word2ph, group=group)
    assert len(got) == 7
    for a, w, g in zip(ids, word2ph, got):
        assert g.shape == (fake.C, sum(w)) and g.dtype == torch.float32
        assert torch.equal(g, fake.want(a, w))
    flat = [n for grp in fake.groups for n in grp]
    assert flat == sorted(n + 2 for n in chars)                               # sorted by length over the whole call
    assert [len(grp) for grp in fake.groups] == [group] * (7 // group) + ([7 % group] if 7 % group else [])
    assert fake.uploads == len(fake.groups)                                   # one expand per group


def test_mismatch_errors_name_the_sentence_before_any_upload():
    from easevoice_trainer_amd.feature_extractor.roberta import BertFeatures
    from easevoice_trainer_amd.inference.text import plan_fragments

    ids, word2ph = _sentences(2, [4, 6, 5])
    fake = _FakeEncoder()
    bert = fake.make()
    bad = [word2ph[0], word2ph[1], word2ph[2] + [1]]
    with pytest.raises(ValueError, match=r"text and word2ph not match \(sentence 2"):
        bert.phone_level_features_batch(ids, bad)
    with pytest.raises(ValueError, match="2 word2ph lists for 3"):
        bert.phone_level_features_batch(ids, word2ph[:2])
    with pytest.raises(ValueError, match="sentence 1"):
        bert.phone_level_features_batch([ids[0], ids[1][:1]], [word2ph[0], []])
    with pytest.raises(ValueError, match="sentence 0"):
        bert.phone_level_features_batch([np.zeros(513, dtype=np.int64)], [[1] * 511])
    with pytest.raises(ValueError):
        bert.phone_level_features_batch(ids, word2ph, group=0)
    assert not fake.groups and not fake.uploads
    # the real hidden_rows refuses before it touches its model or a device (this object has neither)
    bare = BertFeatures.__new__(BertFeatures)
    for wrong in ([np.zeros(1, dtype=np.int64)], [np.zeros(513, dtype=np.int64)], [np.zeros((1, 5), dtype=np.int64)], []):
        with pytest.raises(ValueError):
            bare.hidden_rows(wrong)
    frags = [[("zh", ids[0], word2ph[0])], [("zero", 3), ("zh", ids[1], word2ph[1][:-1])]]
    with pytest.raises(ValueError, match=r"fragment 1, segment 1: text and word2ph not match"):
        plan_fragments(frags)
    with pytest.raises(ValueError, match="prompt 0, segment 0"):
        plan_fragments([frags[0], frags[0]], prompt=[[("zh", ids[2], [1])], []])
    with pytest.raises(ValueError, match="1 prompts for 2 fragments"):
        plan_fragments([frags[0], frags[0]], prompt=[[("zero", 1)]])
    with pytest.raises(ValueError, match="fragment 0, segment 0"):
        plan_fragments([[("ja", 3)]])


def test_fragment_plan_encodes_a_shared_prompt_once():
    from easevoice_trainer_amd.inference.text import fragment_bert_features, plan_fragments

    ids, word2ph = _sentences(3, [5, 2, 8, 3])
    prompt = [("zh", ids[0], word2ph[0]), ("zero", 2)]
    frags = [[("zh", ids[1], word2ph[1])], [("zero", 4)], [("zh", ids[2], word2ph[2]), ("zero", 1), ("zh", ids[3], word2ph[3])]]
    sentences, items = plan_fragments(frags, prompt)
    assert len(sentences) == 4 and np.array_equal(sentences[0][0], ids[0])       # the prompt's sentence once, first
    assert items == [[("sent", 0), ("zero", 2), ("sent", 1)], [("sent", 0), ("zero", 2), ("zero", 4)],
                     [("sent", 0), ("zero", 2), ("sent", 2), ("zero", 1), ("sent", 3)]]
    sentences, items = plan_fragments(frags, [prompt, [], prompt])                # per fragment: encoded per fragment
    assert len(sentences) == 5 and items[1] == [("zero", 4)] and items[2][0] == ("sent", 2) and items[0][0] == ("sent", 0)
    sentences, items = plan_fragments(frags)
    assert len(sentences) == 3 and items[0] == [("sent", 0)]
    assert plan_fragments([], prompt) == ([], [])
    # through the fake encoder: the reference's assembly, cat(prompt, fragment) with zeros
    fake = _FakeEncoder()
    bert = fake.make()
    feat =lambda seg: fake.want(seg[1], seg[2]) if seg[0] == "zh" else torch.zeros(fake.C, seg[1])  # noqa: E731
    for pr, per in ((prompt, [prompt] * 3), ([prompt, [], prompt], [prompt, [], prompt]), (None, [[]] * 3)):
        fake.groups.clear()
        got = fragment_bert_features(bert, frags, pr, group=2)
        for f, g in enumerate(got):
            want = torch.cat([feat(s) for s in per[f] + frags[f]], 1)
            assert g.shape == want.shape and torch.equal(g, want), (f, pr is None)
        assert sum(len(grp) for grp in fake.groups) == (4 if pr is prompt else 5 if pr is not None else 3)
    fake.groups.clear()
    got = fragment_bert_features(bert, [[("zero", 3)], []], [("zero", 2)])       # no Chinese at all: no pass, no launch
    assert [tuple(g.shape) for g in got] == [(fake.C, 5), (fake.C, 2)] and not fake.groups and not any(g.any() for g in got)


class _FakeBert:
    """stands for BertFeatures behind FeatureWriter: records what it is given; a feature's value is its sentence's length"""

    def __init__(self):
        self.single, self.batches = [], []

    def phone_level_feature(self, input_ids, word2ph):
        self.single.append(torch.as_tensor(input_ids).numel())
        return torch.full((1024, sum(word2ph)), float(torch.as_tensor(input_ids).numel()))

    def phone_level_features_batch(self, ids_list, word2ph_list, group=16):
        self.batches.append([a.numel() for a in ids_list])
        packed = torch.cat([torch.full((1024 * sum(w),), float(a.numel())) for a, w in zip(ids_list, word2ph_list)])
        out, o = [], 0
        for w in word2ph_list:                                   # views of one buffer, as the real method returns them
            out.append(packed[o:o + 1024 * sum(w)].view(1024, sum(w)))
            o += 1024 * sum(w)
        return out


def test_text_batch_skip_logic_and_file_formats(tmp_path):
    from easevoice_trainer_amd.feature_extractor.normalize import FeatureWriter

    ids, word2ph = _sentences(4, [3, 5, 2, 4, 6])
    word2ph = [[max(c, 1) for c in w] for w in word2ph]
    lang = ["zh", "en", "zh", "zh", "zh"]
    names = ["a.wav", "b.wav", "have.wav", "c.wav", "a.wav"]                     # one exists, one comes twice
    items = [(names[i], ["p%d" % k for k in range(sum(word2ph[i]))], word2ph[i], "text %d" % i, lang[i],
              torch.from_numpy(ids[i]).unsqueeze(0)) for i in range(5)]
    items[4] = (names[4], items[0][1], word2ph[0], "again", "zh", items[0][5])
    dirs = [tmp_path / "one", tmp_path / "batch"]
    berts = [_FakeBert(), _FakeBert()]
    writers = [FeatureWriter(str(d), None, b) for d, b in zip(dirs, berts)]
    for d in dirs:
        torch.save(torch.zeros(1), d / "3-bert" / "have.wav.pt")
    for it in items:
        writers[0].text(*it)
    writers[1].text_batch(items)
    for w in writers:
        w.close()
    assert berts[0].single == [5, 6] and not berts[0].batches
    assert berts[1].batches == [[5, 6]] and not berts[1].single                  # en, the existing and the repeated name dropped
    assert sorted(os.listdir(dirs[0] / "3-bert")) == sorted(os.listdir(dirs[1] / "3-bert")) == ["a.wav.pt", "c.wav.pt", "have.wav.pt"]
    for name in ("a.wav.pt", "c.wav.pt"):
        a, b = torch.load(dirs[0] / "3-bert" / name), torch.load(dirs[1] / "3-bert" / name)
        assert b.dtype == torch.float32 and b.device.type == "cpu" and b.shape == a.shape and torch.equal(a, b)
        assert b.is_contiguous() and b.untyped_storage().nbytes() == 4 * b.numel()     # the item alone, not the packed buffer
        assert abs(os.path.getsize(dirs[0] / "3-bert" / name) - os.path.getsize(dirs[1] / "3-bert" / name)) < 64
    one, batch = (open(d / "2-name2text.txt", "rb").read() for d in dirs)
    assert one == batch and one.count(b"\n") == 5
    # nothing left to encode: no call at all, the lines still come
    w = FeatureWriter(str(dirs[1]), None, berts[1])
    w.text_batch([items[1], items[2], items[0]])
    assert len(berts[1].batches) == 1 and len(w._text_lines) == 3
    w.text_batch([])
    # the per-item check of the phones
    bad = (("new.wav",) + (items[3][1][:-1],) + items[3][2:])
    with pytest.raises(ValueError, match="bert_feature and phones not match"):
        w.text_batch([items[1], bad])
    assert not os.path.exists(dirs[1] / "3-bert" / "new.wav.pt")


def test_libraries_export_the_bert_rows_entry_points():
    """both builds export evt_phone_expand_rows / evt_bert_embed_ln_rows, and the bindings pass as many arguments as
    include/evt.h declares"""
    from easevoice_trainer_amd.hip import lib as L

    hdr = open(os.path.join(HERE, "..", "include", "evt.h")).read()
    declared = {}
    for name in ("evt_phone_expand_rows", "evt_bert_embed_ln_rows"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in evt.h"
        declared[name] = len(m.group(1).split(","))
    assert declared == {"evt_phone_expand_rows": 12, "evt_bert_embed_ln_rows": 18}
    for half in (torch.bfloat16, torch.float16):
        L.set_half(half)
        lib = L.lib()
        for name, count in declared.items():
            assert hasattr(lib, name), f"{name} is not exported by the {half} build"
            assert len(getattr(lib, name).argtypes) == count, f"{name} of the {half} build"
        # the argument checks return an error code before anything is launched (NULL pointers, C not a multiple of 8)
        fn = lib.evt_phone_expand_rows
        assert fn(L.DT_F32, None, 1, 10, 64, None, None, 1, 5, L.DT_F32, None, None) == 22
        assert fn(L.DT_F32, 16, 1, 10, 60, 16, 16, 1, 5, L.DT_F32, 16, None) == 22
        assert fn(L.DT_F32, 16, 1, 10, 4104, 16, 16, 1, 5, L.DT_F32, 16, None) == 22
        assert fn(L.DT_F32, 16, 1, 10, 64, 16, 16, 1, 0, L.DT_F32, 16, None) == 0          # no columns: nothing to do
        assert fn(7, 16, 1, 10, 64, 16, 16, 1, 5, L.DT_F32, 16, None) == 95
        fn = lib.evt_bert_embed_ln_rows
        assert fn(L.DT_F32, None, None, None, 1, 4, None, 10, None, 512, None, 2, None, None, 1e-12, 64, None, None) == 22
        assert fn(L.DT_F32, 16, None, 16, 1, 600, 16, 10, 16, 512, 16, 2, 16, 16, 1e-12, 64, 16, None) == 22   # T > max_pos
    L.set_half(torch.bfloat16)
