"""The model-side core of TTS.run for one batch of text fragments (src/easevoice/inference/tts.py:756-817): semantic
tokens from the s1 decoder, waveform fragments from the s2 decoder.  Everything around it in the reference -- text
front-end, BERT / CN-HuBERT feature extraction, bucketing, audio post-processing -- is outside SURVEY §8."""
import math

import torch


@torch.no_grad()
def synthesize_fragments(t2s, voice, batch_phones, all_phoneme_ids, all_bert_features, prompt_semantic, refer_specs,
                         top_k=5, top_p=1, temperature=1.0, repetition_penalty=1.35, speed_factor=1.0,
                         parallel_infer=True, max_len=None, decode_kwargs=None, sample_kwargs=None):
    """batch_phones: the fragments' own phoneme ids (list of 1-D); all_phoneme_ids / all_bert_features: prompt + fragment
    ids and their BERT features [1024, n] (lists); prompt_semantic [1, P] or None; refer_specs: list of [1, spec, T].
    Returns the list of waveform fragments (1-D tensors on the device), tts.py:794-817."""
    model = t2s.model
    dev = t2s.device
    n = len(all_phoneme_ids)
    prompt = None if prompt_semantic is None else prompt_semantic.expand(n, -1).to(dev)
    infer = model.infer_panel_batch_infer if parallel_infer else model.infer_panel_naive_batched
    lens = torch.tensor([int(p.numel()) for p in all_phoneme_ids])
    pred, idx_list = infer([p.to(dev) for p in all_phoneme_ids], lens, prompt, [b.to(dev) for b in all_bert_features],
                           top_k=top_k, top_p=top_p, temperature=temperature, early_stop_num=t2s.early_stop_num,
                           max_len=max_len, repetition_penalty=repetition_penalty, **(sample_kwargs or {}))
    refer = [r.to(dev) for r in refer_specs]
    kw = decode_kwargs or {}
    if speed_factor == 1.0:
        # one decode over the concatenated fragments, then cut (tts.py:795-807)
        pred = [p[-i:] for p, i in zip(pred, idx_list)]
        up = math.prod(voice.model.upsample_rates)
        ends = [0]
        for p in pred:
            ends.append(ends[-1] + p.shape[0] * 2 * up)
        sem = torch.cat(pred).unsqueeze(0).unsqueeze(0)
        phones = torch.cat([p.to(dev) for p in batch_phones]).unsqueeze(0)
        audio = voice.model.decode(sem, phones, refer, speed=speed_factor, **kw)[0, 0, :]
        return [audio[ends[i - 1]:ends[i]] for i in range(1, len(ends))]
    out = []
    for p, i, ph in zip(pred, idx_list, batch_phones):
        sem = p[-i:].unsqueeze(0).unsqueeze(0)
        out.append(voice.model.decode(sem, ph.to(dev).unsqueeze(0), refer, speed=speed_factor, **kw)[0, 0, :])
    return out


def synthesize_stream(t2s, voice, batch_phones, all_phoneme_ids, all_bert_features, prompt_semantic, refer_specs,
                      top_k=5, top_p=1, temperature=1.0, repetition_penalty=1.35, speed_factor=1.0, slots=32,
                      decode_kwargs=None, sample_kwargs=None, fragment_sampling=None, control=None, candidates=1,
                      choose=None, wide=False):
    """synthesize_fragments handing the fragments out one by one (the model-side core of TTS.run's return_fragment
    mode): a generator of (index, waveform) in the order in which the fragments' semantic tokens are complete.  The
    fragments decode in a refilled s1 session of up to `slots` rows (decode_stream: more fragments than slots wait for a
    free row; wide=True allows up to 128 slots, decode_stream's `wide`); each is turned into audio on its own by the
    s2 decoder as soon as its tokens are there, at any
    speed_factor, while the other rows' tokens wait in the session.  prompt_semantic: [1, P] for all fragments, or a
    list with one token vector per fragment (fragments of several reference voices in one session).
    fragment_sampling: a list with one dict (keys out of top_k, top_p, temperature, repetition_penalty, early_stop_num)
    or None per fragment, replacing the values above for that fragment alone; the dicts go to decode_stream as they are,
    so "seed" (the fragment's own noise seed) and "force" (given first tokens, e.g. those of a preempted take) work here
    too.  control: a StreamControl of auto_reg/t2s_infer.py; a fragment cancelled through it is yielded as (index, None)
    and never reaches the s2 decoder, and so is a fragment preempted through it (decode_stream hands out its partial
    tokens with idx = None; a caller who wants to resume it drives decode_stream itself).
    candidates > 1: every fragment is decoded `candidates` times after one prompt pass (decode_stream's n, with
    log-probabilities on) and choose(fragment_index, outputs) -- required then -- is called once all of them are in,
    with the fragment's StreamOutputs in candidate order (a cancelled take has y = None); it returns the number of the
    take to keep, and only that take goes through the s2 decoder.  A fragment whose takes were all cancelled is yielded
    as (index, None) without a call.  The project ships no default rule: mean log-probability is no proven quality
    criterion for this model (loops are likely sequences)."""
    model, dev = t2s.model, t2s.device
    n = len(all_phoneme_ids)
    candidates = int(candidates)
    if candidates < 1:
        raise ValueError(f"candidates = {candidates} must be >= 1")
    if candidates > 1 and choose is None:
        raise ValueError("candidates > 1 needs choose(fragment_index, outputs) -> candidate number")
    if prompt_semantic is None:
        raise ValueError("synthesize_stream needs the prompt's semantic tokens")
    prompts = ([p.reshape(-1).to(dev) for p in prompt_semantic] if isinstance(prompt_semantic, (list, tuple))
               else [prompt_semantic.reshape(-1).to(dev)] * n)
    if fragment_sampling is not None and len(fragment_sampling) != n:
        raise ValueError(f"fragment_sampling has {len(fragment_sampling)} entries for {n} fragments")
    reqs = [(p.to(dev), b.to(dev), pr) for p, b, pr in zip(all_phoneme_ids, all_bert_features, prompts)]
    if fragment_sampling is not None:
        reqs = [q if fs is None else (*q, dict(fs)) for q, fs in zip(reqs, fragment_sampling)]
    refer = [r.to(dev) for r in refer_specs]
    kw = decode_kwargs or {}

    def audio(r, y, idx):
        with torch.no_grad():
            sem = y[-idx:].unsqueeze(0).unsqueeze(0)
            return voice.model.decode(sem, batch_phones[r].to(dev).unsqueeze(0), refer, speed=speed_factor, **kw)[0, 0, :]

    if candidates > 1:
        if int(slots) < candidates:
            raise ValueError(f"slots = {int(slots)} cannot hold the {candidates} candidates of one fragment")
        stream = model.decode_stream(reqs, slots=min(int(slots), max(n, 1) * candidates), top_k=top_k, top_p=top_p,
                                     temperature=temperature, early_stop_num=t2s.early_stop_num,
                                     repetition_penalty=repetition_penalty, control=control, n=candidates, logprobs=True,
                                     wide=wide, **(sample_kwargs or {}))
        takes = {}
        for o in stream:
            got = takes.setdefault(o.request, {})
            got[o.candidate] = o
            if len(got) < candidates:
                continue
            outs = [got[c] for c in range(candidates)]
            del takes[o.request]
            if all(t.y is None or t.idx is None for t in outs):
                yield o.request, None
                continue
            t = outs[int(choose(o.request, outs))]
            yield o.request, (None if t.y is None or t.idx is None else audio(o.request, t.y, t.idx))
        return
    stream = model.decode_stream(reqs, slots=max(1, min(int(slots), n)), top_k=top_k, top_p=top_p, temperature=temperature,
                                 early_stop_num=t2s.early_stop_num, repetition_penalty=repetition_penalty,
                                 control=control, wide=wide, **(sample_kwargs or {}))
    for r, y, idx in stream:
        if y is None or idx is None:       # cancelled, or preempted with partial tokens: no s2 decode
            yield r, None
            continue
        with torch.no_grad():
            sem = y[-idx:].unsqueeze(0).unsqueeze(0)
            wav = voice.model.decode(sem, batch_phones[r].to(dev).unsqueeze(0), refer, speed=speed_factor, **kw)[0, 0, :]
        yield r, wav
