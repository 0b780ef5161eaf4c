"""The model-side core of TTS.run for one batch of text fragments (src/easevoice/inference/tts.py:756-817): semantic
tokens from the s1 decoder, waveform fragments from the s2 decoder.  Everything around it in the reference -- text
front-end, BERT / CN-HuBERT feature extraction, bucketing -- is outside SURVEY §8.  The audio post-processing
(TTS.audio_postprocess, tts.py:878-908: int16 with a silence interval behind every fragment) is synthesize_pcm, with any
output rate; synthesize_stream hands out single fragments at a rate and in a format of the caller's choice."""
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


def _poll_groups(stream, stats, per_waiting):
    """The outputs of a decode_stream generator, grouped by the poll that completed them: lists of outputs the session had
    ready at the same time.  The session records every output in stream_stats["events"] (a finish / cancel / preempt event
    per row; one "cancel" event without a slot for a request withdrawn while it waited, which is handed out once per
    candidate = per_waiting times) before it yields the first of them, so after an output the events say how many more
    are already there: those are taken at once, and the generator is never advanced into its next poll for a group.
    stats() -> the session's stream_stats or None (a decoder that keeps none: every output is its own group)."""
    seen, expected, received, group = 0, 0, 0, []
    for o in stream:
        received += 1
        st = stats()
        events = None if st is None else st.get("events")
        if events is None:
            yield [o]
            continue
        for kind, _steps, _r, slot in events[seen:]:
            if kind != "admit":
                expected += per_waiting if slot is None else 1
        seen = len(events)
        group.append(o)
        if received >= expected:
            yield group
            group = []
    if group:
        yield group


def _finish(voice, wav, out):
    """one waveform of decode -> the caller's rate and format: resample_pack with nseq = 1, the launch a group's rows get
    behind decode_batch (a row comes out of it bit for bit as it does alone).  out: {} (the waveform as it is), or the
    out_rate / out_format that were set"""
    if not out:
        return wav
    from ..hip.audio import resample_pack

    rate = getattr(voice.model, "sampling_rate", 32000)
    return resample_pack(wav, [wav.numel()], 1, rate, out.get("out_rate", rate), out.get("out_format", "float32")).row(0)


def _decode_group(voice, dev, batch_phones, refer, kw, items, speeds=None, out=None, styles=None):
    """items: [(fragment index, y, idx)] of one poll, at most s2_batch of them -> their waveforms, through ONE decode_batch
    call (a single fragment: the decode call of the one-by-one path).  speeds: None, or one speed per fragment of the
    whole request (fragment_speed); decode_batch gets the group's values only when one of them is not 1.  out: the
    out_rate / out_format keywords that were set; decode_batch gets them only then, and its PackedAudio is handed out row
    by row.  styles: None, or one [1, gin] style vector per fragment of the whole request (fragment_style): the group then
    goes through decode_batch(refer=None, style=<its rows stacked, in order>), a single fragment through decode(style=...)"""
    out = out or {}
    with torch.no_grad():
        if len(items) == 1:
            r, y, idx = items[0]
            sem = y[-idx:].unsqueeze(0).unsqueeze(0)
            one = 1.0 if speeds is None else speeds[r]
            if styles is not None:
                return [_finish(voice, voice.model.decode(sem, batch_phones[r].to(dev).unsqueeze(0), None, speed=one,
                                                          style=styles[r], **kw)[0, 0, :], out)]
            return [_finish(voice, voice.model.decode(sem, batch_phones[r].to(dev).unsqueeze(0), refer, speed=one, **kw)[0, 0, :],
                            out)]
        if speeds is not None and any(speeds[r] != 1.0 for r, _y, _idx in items):
            kw = dict(kw, speed=[speeds[r] for r, _y, _idx in items])
        sems = [y[-idx:] for _r, y, idx in items]
        phones = [batch_phones[r].to(dev) for r, _y, _idx in items]
        codes = torch.nn.utils.rnn.pad_sequence(sems, batch_first=True).unsqueeze(0)
        text = torch.nn.utils.rnn.pad_sequence(phones, batch_first=True)
        if styles is not None:
            got = voice.model.decode_batch(codes, [int(t.numel()) for t in sems], text, [int(t.numel()) for t in phones],
                                           None, style=torch.cat([styles[r] for r, _y, _idx in items], 0), **kw, **out)
            return [got.row(b) for b in range(len(items))] if out else got
        # one entry per row, all the same object: decode_batch encodes the shared reference(s) once
        got = voice.model.decode_batch(codes, [int(t.numel()) for t in sems], text, [int(t.numel()) for t in phones],
                                       [refer] * len(items), **kw, **out)
        return [got.row(b) for b in range(len(items))] if out else got


def synthesize_stream(t2s, voice, batch_phones, all_phoneme_ids, all_bert_features, prompt_semantic, refer_specs,
                      top_k=5, top_p=1, temperature=1.0, repetition_penalty=1.35, speed_factor=1.0, slots=32,
                      decode_kwargs=None, sample_kwargs=None, fragment_sampling=None, control=None, candidates=1,
                      choose=None, wide=False, s2_batch=1, fragment_speed=None, out_rate=None, out_format=None,
                      fragment_style=None):
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
    criterion for this model (loops are likely sequences).
    s2_batch = k > 1 (with speed_factor == 1; any other speed decodes one by one as with k = 1): fragments whose tokens
    the s1 session delivers from the SAME poll go through the s2 decoder in groups of at most k, one decode_batch call
    per group (SynthesizerTrn.decode_batch: every row is what decode gives for it alone), and are yielded in the order
    they arrived; cancelled and preempted fragments pass through as (index, None) in that order.  It never waits for a
    later poll: a fragment that finishes alone is decoded alone.  With candidates > 1 the chosen takes go through the
    groups.  decode_kwargs then go to decode_batch (noise_scale; a `noise` of batch 1 is shared by the rows).
    fragment_speed: None, or a list with one speed per fragment (speed_factor must then be 1.0): fragment r is decoded
    at fragment_speed[r].  With s2_batch > 1 the groups stay batched -- a group goes through one
    decode_batch(speed=[the group's speeds]) call, which resamples every row on its own lengths, and through the call
    without the keyword when all its speeds are 1 --; with s2_batch == 1, for a fragment that finishes alone and with
    candidates > 1 outside the groups it is decode(speed=fragment_speed[r]).
    out_rate / out_format (both None: the waveforms as the decoder gives them): every fragment is yielded as a 1-D device
    tensor at out_rate Hz (None: the model's rate) in out_format "int16" or "float32" (None: "float32") -- the operator of
    hip/audio.py.  A group's decode_batch call gets the keywords that were set (and no others) and finishes its rows with
    one more launch; a fragment decoded alone goes through decode and then resample_pack with one row, which gives the
    same bits.
    fragment_style: None (every fragment speaks with the shared refer_specs: the calls above, unchanged), or a list with one
    precomputed voice per fragment -- a [1, gin] style vector (SynthesizerTrn.style_rows / _style) or an
    inference/voice.py::EnrolledVoice --, the companion of a per-fragment prompt_semantic: fragment r is decoded with voice
    r.  refer_specs may then be empty; a group goes through decode_batch(refer=None, style=<the group's rows stacked>),
    whose rows may all differ, a fragment decoded alone through decode(refer=None, style=...)."""
    model, dev = t2s.model, t2s.device
    out = {k: v for k, v in (("out_rate", out_rate), ("out_format", out_format)) if v is not None}
    s2_batch = int(s2_batch)
    if s2_batch < 1:
        raise ValueError(f"s2_batch = {s2_batch} must be >= 1")
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
    if fragment_speed is not None:
        if speed_factor != 1.0:
            raise ValueError(f"fragment_speed gives every fragment its own speed: speed_factor must be 1.0, not {speed_factor}")
        if len(fragment_speed) != n:
            raise ValueError(f"fragment_speed has {len(fragment_speed)} entries for {n} fragments")
        fragment_speed = [float(v) for v in fragment_speed]
    if fragment_style is not None:
        if len(fragment_style) != n:
            raise ValueError(f"fragment_style has {len(fragment_style)} entries for {n} fragments")
        fragment_style = [getattr(v, "style", v).to(dev).reshape(1, -1) for v in fragment_style]
    reqs = [(p.to(dev), b.to(dev), pr) for p, b, pr in zip(all_phoneme_ids, all_bert_features, prompts)]
    if fragment_sampling is not None:
        reqs = [q if fs is None else (*q, dict(fs)) for q, fs in zip(reqs, fragment_sampling)]
    refer = [r.to(dev) for r in refer_specs]
    kw = decode_kwargs or {}

    def audio(r, y, idx):
        with torch.no_grad():
            sem = y[-idx:].unsqueeze(0).unsqueeze(0)
            one = speed_factor if fragment_speed is None else fragment_speed[r]
            if fragment_style is not None:
                return _finish(voice, voice.model.decode(sem, batch_phones[r].to(dev).unsqueeze(0), None, speed=one,
                                                         style=fragment_style[r], **kw)[0, 0, :], out)
            return _finish(voice, voice.model.decode(sem, batch_phones[r].to(dev).unsqueeze(0), refer, speed=one, **kw)[0, 0, :],
                           out)

    if candidates > 1 and int(slots) < candidates:
        raise ValueError(f"slots = {int(slots)} cannot hold the {candidates} candidates of one fragment")

    def open_stream():
        if candidates > 1:
            return model.decode_stream(reqs, slots=min(int(slots), max(n, 1) * candidates), top_k=top_k, top_p=top_p,
                                       temperature=temperature, early_stop_num=t2s.early_stop_num,
                                       repetition_penalty=repetition_penalty, control=control, n=candidates, logprobs=True,
                                       wide=wide, **(sample_kwargs or {}))
        return model.decode_stream(reqs, slots=max(1, min(int(slots), n)), top_k=top_k, top_p=top_p, temperature=temperature,
                                   early_stop_num=t2s.early_stop_num, repetition_penalty=repetition_penalty,
                                   control=control, wide=wide, **(sample_kwargs or {}))

    if s2_batch > 1 and speed_factor == 1.0:
        stream = open_stream()

        def stats():
            owner = model._infer() if hasattr(model, "_infer") else model
            return getattr(owner, "stream_stats", None)

        takes = {}
        for group in _poll_groups(stream, stats, candidates):
            ready = []               # this poll's fragments in arrival order: (index, y, idx), y None = no decode
            for o in group:
                if candidates == 1:
                    r, y, idx = o
                    ready.append((r, None, None) if y is None or idx is None else (r, y, idx))
                    continue
                got = takes.setdefault(o.request, {})
                got[o.candidate] = o
                if len(got) < candidates:
                    continue
                outs = [got[c] for c in range(candidates)]
                del takes[o.request]
                if all(t.y is None or t.idx is None for t in outs):
                    ready.append((o.request, None, None))
                    continue
                t = outs[int(choose(o.request, outs))]
                ready.append((o.request, None, None) if t.y is None or t.idx is None else (o.request, t.y, t.idx))
            while ready:
                if ready[0][1] is None:
                    yield ready.pop(0)[0], None
                    continue
                # up to s2_batch fragments to decode, with the cancelled ones that arrived between them
                take, live = 0, 0
                while take < len(ready) and (ready[take][1] is None or live < s2_batch):
                    live += ready[take][1] is not None
                    take += 1
                chunk, ready = ready[:take], ready[take:]
                wavs = iter(_decode_group(voice, dev, batch_phones, refer, kw, [c for c in chunk if c[1] is not None],
                                          fragment_speed, out, fragment_style))
                for r, y, _idx in chunk:
                    yield r, (None if y is None else next(wavs))
        return
    stream = open_stream()
    if candidates > 1:
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
    for r, y, idx in stream:
        if y is None or idx is None:       # cancelled, or preempted with partial tokens: no s2 decode
            yield r, None
            continue
        yield r, audio(r, y, idx)


def synthesize_pcm(t2s, voice, batch_phones, all_phoneme_ids, all_bert_features, prompt_semantic, refer_specs, out_rate=None,
                   fragment_interval=0.3, **stream_kwargs):
    """The non-streaming end of TTS.run (tts.py:878-908, audio_postprocess): -> (rate, int16 tensor on the host) holding the
    fragments in INPUT order, int(rate * fragment_interval) zeros behind each (the reference's zero_wav).  out_rate None:
    the model's rate.  It drains synthesize_stream(out_rate=rate, out_format="int16", **stream_kwargs) -- s2_batch, slots,
    fragment_speed, control ... as there --, so conversion and resampling happen on the device, one launch per group;
    fragments that come back cancelled (or preempted) are left out together with their interval.  The pieces are joined
    on the device and leave it in ONE device -> host copy.  fragment_style (one voice per fragment, refer_specs may be
    empty) goes through as the other stream keywords do."""
    rate = int(getattr(voice.model, "sampling_rate", 32000) if out_rate is None else out_rate)
    if fragment_interval < 0:
        raise ValueError(f"fragment_interval = {fragment_interval} must be >= 0")
    for k in ("out_rate", "out_format"):
        if k in stream_kwargs:
            raise ValueError(f"synthesize_pcm sets {k} itself")
    got = {}
    for r, wav in synthesize_stream(t2s, voice, batch_phones, all_phoneme_ids, all_bert_features, prompt_semantic, refer_specs,
                                    out_rate=rate, out_format="int16", **stream_kwargs):
        if wav is not None:
            got[r] = wav
    if not got:
        return rate, torch.zeros(0, dtype=torch.int16)
    silence = torch.zeros(int(rate * fragment_interval), dtype=torch.int16, device=next(iter(got.values())).device)
    pieces = [t for r in sorted(got) for t in (got[r], silence)]
    return rate, torch.cat(pieces).cpu()
