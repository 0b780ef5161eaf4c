"""The `token` step of the reference's normalisation (src/normalization/normalize.py:181-211): semantic codes of every
extracted CN-HuBERT feature file, written as 6-name2semantic.tsv -- the s1 stage's training targets.

The reference pins this step to the CPU (normalize.py:58-60); here `extract_latent` runs through SoVITSVoice on the GPU.
Format kept byte for byte: header `item_name\\tsemantic_audio`, one `name\\tc0 c1 ...` line per item whose
`4-cnhubert/<name>.pt` exists, items in the order given, trailing newline."""
import os

import torch


PROMPT_MIN, PROMPT_MAX = 48000, 160000      # 3 .. 10 s at 16 kHz (inference/tts.py:418)
PROMPT_TAIL = int(32000 * 0.3)               # tts.py:412-413: zero_wav, sized from the model's 32 kHz sampling_rate


def prompt_semantics(hubert, extract_latent, wavs16k, extract_latent_rows=None):
    """The reference's _set_prompt_semantic (inference/tts.py:411-437) for SEVERAL reference clips in one pass each of the
    two models.  hubert: feature_extractor.CNHubert (or any object with its last_hidden_state_batch); extract_latent:
    callable ssl [B, 768, T] -> codes [B, 1, T // 2]; wavs16k: 1-D 16 kHz clips of 3 .. 10 s (OSError otherwise, as the
    reference).  Every clip gets the reference's 0.3 s of zeros appended; the ragged batch goes through
    last_hidden_state_batch; extract_latent takes the padded [B, 768, Tmax] -- its k = 2, stride 2 convolution and the
    per-frame quantiser neither mix rows nor let a kept code read past the row's T_b frames -- and row b is cut to
    T_b // 2 codes.  -> list of 1-D code tensors, what synthesize_stream(prompt_semantic=[...]) takes.
    extract_latent_rows (SoVITSVoice.extract_latent_rows): when given, the hidden states and the frame counts go to it as
    they are -- no transposed fp32 copy, no codes for the padding -- and extract_latent is not called."""
    clips = []
    for b, w in enumerate(wavs16k):
        w = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        if w.numel() > PROMPT_MAX or w.numel() < PROMPT_MIN:
            raise OSError(f"reference clip {b}: audio length should be in 3~10 seconds.")
        clips.append(torch.cat([w, torch.zeros(PROMPT_TAIL, dtype=torch.float32, device=w.device)]))
    if not clips:
        return []
    with torch.no_grad():
        hs, frame_lens = hubert.last_hidden_state_batch(clips)              # [B, Tmax, 768]
        if extract_latent_rows is not None:
            rows = extract_latent_rows(hs, frame_lens)
            if len(rows) != len(clips) or any(r.dim() != 1 or r.numel() != t // 2 for r, t in zip(rows, frame_lens)):
                raise ValueError(f"extract_latent_rows returned {[tuple(r.shape) for r in rows]} for frame counts {frame_lens}")
            return [r.clone() for r in rows]
        codes = extract_latent(hs.transpose(1, 2).float().contiguous())     # [B, 1, Tmax // 2]
    if codes.dim() != 3 or codes.size(0) != len(clips) or codes.size(2) != hs.size(1) // 2:
        raise ValueError(f"extract_latent returned {tuple(codes.shape)} for features {tuple(hs.shape)}")
    return [codes[b, 0, :t // 2].clone() for b, t in enumerate(frame_lens)]


def write_semantic_tsv(extract_latent, names, hubert_dir, out_path, device="cpu"):
    """extract_latent: callable ssl [1, 768, T] -> codes [1, 1, T'] (SoVITSVoice.extract_latent or
    SynthesizerTrn.extract_latent); names: item names (the wav basenames of the refinement list)."""
    opt = ["item_name\tsemantic_audio"]
    for name in names:
        path = os.path.join(hubert_dir, name + ".pt")
        if not os.path.exists(path):
            continue
        ssl = torch.load(path, map_location="cpu").float().to(device)
        codes = extract_latent(ssl)
        opt.append("%s\t%s" % (name, " ".join(str(int(i)) for i in codes[0, 0, :].tolist())))
    with open(out_path, "w", encoding="utf8") as f:
        f.write("\n".join(opt) + "\n")
    return len(opt) - 1


def codes_to_host(rows):
    """a list of 1-D code tensors -> a list of lists of ints with ONE device-to-host copy: of the packed buffer the rows are
    consecutive views of (what extract_latent_rows returns), of their concatenation otherwise"""
    rows = list(rows)
    if not rows:
        return []
    base, at, packed = rows[0]._base, 0, True
    for r in rows:
        packed = packed and base is not None and r._base is base and r.dim() == 1 and r.is_contiguous() \
            and r.storage_offset() == base.storage_offset() + at
        at += r.numel()
    flat = base if packed and base.dim() == 1 and base.numel() == at else torch.cat([r.reshape(-1) for r in rows])
    flat, out, at = flat.cpu().tolist(), [], 0
    for r in rows:
        out.append(flat[at: at + r.numel()])
        at += r.numel()
    return out


def codes_of_files(extract_latent_rows, paths, group=16, device="cuda:0"):
    """the codes of feature files ([1, 768, T] float32, as 4-cnhubert/<name>.pt) in groups of at most `group` -> a list of
    lists of ints, in the order of paths.  Per group the files are read into ONE zero-padded channels-last host buffer
    [G, Tmax, 768] (page-locked and reused by the groups when the target is a GPU), uploaded in one copy, tokenised by one
    call of extract_latent_rows, and the packed codes come back in one copy.  The writers of these files (CNHubert.__call__ /
    batch, as the reference) save a transposed view of [1, T, 768] hidden states and torch.save keeps the strides, so a
    loaded file IS channels-last in memory and filling a row is a straight copy; a file saved C-contiguous is served too,
    through a strided copy."""
    group = int(group)
    if group < 1:
        raise ValueError(f"group must be at least 1, got {group}")
    out, stage = [], None
    for g0 in range(0, len(paths), group):
        feats = [torch.load(p, map_location="cpu").float() for p in paths[g0: g0 + group]]
        for p, f in zip(paths[g0:], feats):
            if f.dim() != 3 or f.size(0) != 1 or f.size(1) != feats[0].size(1):
                raise ValueError(f"{p}: features [1, C, T] expected, got {tuple(f.shape)}")
        frames = [f.size(2) for f in feats]
        G, tmax, C = len(feats), max(max(frames), 1), feats[0].size(1)
        if stage is None or stage.numel() < G * tmax * C:     # one staging buffer for all groups, page-locked for a GPU
            stage = torch.empty(G * tmax * C, dtype=torch.float32, pin_memory=torch.device(device).type == "cuda")
        host = stage[: G * tmax * C].view(G, tmax, C)
        for b, (f, t) in enumerate(zip(feats, frames)):
            host[b, :t].copy_(f[0].t())
            host[b, t:].zero_()
        with torch.no_grad():
            rows = extract_latent_rows(host.to(device), frames)
        if len(rows) != G or any(r.dim() != 1 or r.numel() != t // 2 for r, t in zip(rows, frames)):
            raise ValueError(f"extract_latent_rows returned {[tuple(r.shape) for r in rows]} for frame counts {frames}")
        out.extend(codes_to_host(rows))
    return out


def semantic_line(name, codes):
    return "%s\t%s" % (name, " ".join(str(int(i)) for i in codes))


def write_semantic_tsv_batch(extract_latent_rows, names, hubert_dir, out_path, group=16, device="cuda:0"):
    """`write_semantic_tsv` in groups of at most `group` items: the same file byte for byte (header, one line per name whose
    feature file exists, names in the order given), with one upload of the padded channels-last group, one launch
    (evt_semantic_codes_rows) and one read-back per group (codes_of_files) instead of an upload, a transposed copy, four
    launches and a synchronisation per item.  extract_latent_rows: SoVITSVoice.extract_latent_rows (or
    SynthesizerTrn's): (hs [B, Tmax, 768], frame counts) -> B 1-D code tensors."""
    names = [n for n in names if os.path.exists(os.path.join(hubert_dir, n + ".pt"))]
    codes = codes_of_files(extract_latent_rows, [os.path.join(hubert_dir, n + ".pt") for n in names], group, device)
    with open(out_path, "w", encoding="utf8") as f:
        f.write("\n".join(["item_name\tsemantic_audio"] + [semantic_line(n, c) for n, c in zip(names, codes)]) + "\n")
    return len(names)
