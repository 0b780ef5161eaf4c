"""The `token` step of the reference's normalisation (src/normalization/normalize.py:181-211): semantic codes of every
extracted CN-HuBERT feature file, written as 6-name2semantic.tsv -- the s1 stage's training targets.

The reference pins this step to the CPU (normalize.py:58-60); here `extract_latent` runs through SoVITSVoice on the GPU.
Format kept byte for byte: header `item_name\\tsemantic_audio`, one `name\\tc0 c1 ...` line per item whose
`4-cnhubert/<name>.pt` exists, items in the order given, trailing newline."""
import os

import torch


PROMPT_MIN, PROMPT_MAX = 48000, 160000      # 3 .. 10 s at 16 kHz (inference/tts.py:418)
PROMPT_TAIL = int(32000 * 0.3)               # tts.py:412-413: zero_wav, sized from the model's 32 kHz sampling_rate


def prompt_semantics(hubert, extract_latent, wavs16k):
    """The reference's _set_prompt_semantic (inference/tts.py:411-437) for SEVERAL reference clips in one pass each of the
    two models.  hubert: feature_extractor.CNHubert (or any object with its last_hidden_state_batch); extract_latent:
    callable ssl [B, 768, T] -> codes [B, 1, T // 2]; wavs16k: 1-D 16 kHz clips of 3 .. 10 s (OSError otherwise, as the
    reference).  Every clip gets the reference's 0.3 s of zeros appended; the ragged batch goes through
    last_hidden_state_batch; extract_latent takes the padded [B, 768, Tmax] -- its k = 2, stride 2 convolution and the
    per-frame quantiser neither mix rows nor let a kept code read past the row's T_b frames -- and row b is cut to
    T_b // 2 codes.  -> list of 1-D code tensors, what synthesize_stream(prompt_semantic=[...]) takes."""
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
