"""The text end of inference on the device: the phone-level BERT features of all fragments of a request in one call.

Reference: inference/tts.py:508-531 and inference/preprocessor.py:110-210 build, per fragment, `all_bert_features =
torch.cat([prompt_bert, fragment_bert], 1)` of shape [1024, n_prompt + n_fragment], where the features of a text are the
concatenation over its language segments of `get_bert_feature` (Chinese: chinese-roberta-wwm-ext-large, one sentence per
pass) or `torch.zeros((1024, n_phones))` (every other language, `get_bert_inf`).  `fragment_bert_features` produces those
tensors for many fragments from grouped passes of feature_extractor.BertFeatures and ONE hip/feat.py::phone_expand_rows.
Tokenising and text cleaning stay on the host in front of this: a segment arrives as ids + word2ph, or as a
count of phones."""
import torch

from ..feature_extractor.roberta import check_sentences, column_map, length_groups


def _is_segment(x):
    return isinstance(x, (tuple, list)) and len(x) > 0 and isinstance(x[0], str)


def _prompts(prompt, n):
    """-> (one segment list per fragment, shared): a shared prompt is the SAME list object for every fragment"""
    if prompt is None:
        prompt = []
    prompt = list(prompt)
    if not prompt or all(_is_segment(s) for s in prompt):
        return [prompt] * n, True
    if len(prompt) != n:
        raise ValueError(f"{len(prompt)} prompts for {n} fragments")
    return [list(p) for p in prompt], False


def plan_fragments(fragments, prompt=None):
    """the host half of fragment_bert_features, no device: -> (sentences, items).  sentences: the (ids, word2ph) of every
    Chinese segment that has to be encoded, a shared prompt's ONCE; items: per fragment the segments of prompt + fragment as
    ("sent", index into sentences) or ("zero", n).  ValueError naming the fragment for a malformed segment and for the
    reference's "text and word2ph not match"."""
    fragments = [list(f) for f in fragments]
    prompts, shared = _prompts(prompt, len(fragments))
    sentences = []

    def plan(segments, where):
        out = []
        for k, seg in enumerate(segments):
            if not _is_segment(seg):
                raise ValueError(f"{where}, segment {k}: ('zh', input_ids, word2ph) or ('zero', n_phones) expected")
            if seg[0] == "zh" and len(seg) == 3:
                try:
                    ids = check_sentences([seg[1]], [list(seg[2])])[0]
                except ValueError as e:
                    raise ValueError(f"{where}, segment {k}: {e}") from None
                out.append(("sent", len(sentences)))
                sentences.append((ids, list(seg[2])))
            elif seg[0] == "zero" and len(seg) == 2 and int(seg[1]) >= 0:
                out.append(("zero", int(seg[1])))
            else:
                raise ValueError(f"{where}, segment {k}: ('zh', input_ids, word2ph) or ('zero', n_phones) expected")
        return out

    shared_plan = plan(prompts[0], "prompt") if shared and fragments else None
    items = []
    for f, segments in enumerate(fragments):
        head = shared_plan if shared else plan(prompts[f], f"prompt {f}")
        items.append(head + plan(segments, f"fragment {f}"))
    return sentences, items


@torch.no_grad()
def fragment_bert_features(bert, fragments, prompt=None, out_dtype=torch.float32, group=16):
    """fragments: per fragment a list of segments, ("zh", input_ids, word2ph) -- 1-D ids [CLS] chars [SEP], a count per
    character -- or ("zero", n_phones); prompt: None, one such list for all fragments, or one list per fragment (several
    voices) -> per fragment the [hidden, n] tensor of out_dtype on bert's device whose columns are the prompt's segments
    followed by the fragment's: what synthesize_stream / synthesize_pcm / decode_stream take as all_bert_features.
    bert: feature_extractor.BertFeatures.  All Chinese segments of the call are sorted by length and encoded in groups of
    at most `group` (BertFeatures.hidden_rows); a prompt shared by all fragments is encoded once and its token rows are
    named by every item's column map; one phone_expand_rows writes all items, zero columns included, into one packed
    buffer, of which the results are views.  Every check is made before anything is uploaded."""
    sentences, items = plan_fragments(fragments, prompt)
    if not items:
        return []
    hidden = bert.hidden_size
    if not sentences:
        return [torch.zeros(hidden, sum(n for _kind, n in it), dtype=out_dtype, device=bert.device) for it in items]
    first = [0] * len(sentences)          # flat index of every sentence's [CLS] row in the concatenated hidden rows
    rows, n_rows = [], 0
    for members in length_groups([ids.size for ids, _w in sentences], group):
        h, _lens = bert.hidden_rows([sentences[i][0] for i in members])
        for j, i in enumerate(members):
            first[i] = n_rows + j * h.size(1)
        n_rows += h.size(0) * h.size(1)
        rows.append(h.reshape(-1, hidden))
    rows = rows[0] if len(rows) == 1 else torch.cat(rows)
    src, item_off = column_map([[("rows", first[s[1]] + 1, sentences[s[1]][1]) if s[0] == "sent" else s for s in it]
                                for it in items])
    packed = bert._expand(rows.view(1, n_rows, hidden), src, item_off, out_dtype)
    off = [int(o) for o in item_off]
    return [packed[hidden * off[f]:hidden * off[f + 1]].view(hidden, off[f + 1] - off[f]) for f in range(len(items))]
