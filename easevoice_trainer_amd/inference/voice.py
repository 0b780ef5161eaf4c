"""Enrolment of reference voices: what the reference computes per clip when a reference is set -- `_get_ref_spec`
(inference/tts.py:390-409: the 32 kHz clip, peak, division, linear spectrogram) with the style encoder behind it, and
`_set_prompt_semantic` (tts.py:411-437: the 16 kHz clip through CN-HuBERT and the quantiser) -- for SEVERAL voices at once,
every stage on the ragged batch: one upload, one hip/audio.py::ref_spec_rows, one SynthesizerTrn.style_rows, one
hip/audio.py::resample_pack to 16 kHz, one inference/semantic.py::prompt_semantics.  The result is computed once and reused:
`EnrolledVoice.style` goes to decode / decode_batch (`style=`) and to synthesize_stream (`fragment_style=`),
`EnrolledVoice.prompt_semantic` to synthesize_stream's per-fragment `prompt_semantic`."""
import os
from dataclasses import dataclass
from typing import List

import torch

from ..audiokit import wav
from ..hip import lib as L
from .semantic import PROMPT_MAX, PROMPT_MIN, prompt_semantics


@dataclass
class EnrolledVoice:
    """style [1, gin] on the device in the dtype the decoder takes; prompt_semantic: 1-D codes; frames: spectrogram frames
    of the main clip"""
    style: torch.Tensor
    prompt_semantic: torch.Tensor
    frames: int


def enroll_voices(voice, hubert, clips32k, aux=None, clips16k=None) -> List[EnrolledVoice]:
    """voice: inference/sovits.py::SoVITSVoice; hubert: feature_extractor.CNHubert (or any object with its
    last_hidden_state_batch); clips32k: one 1-D float32 clip per voice at the model's sampling rate, 3 .. 10 s long (OSError
    otherwise, as the reference; checked before anything is uploaded); aux: None, or per voice a list (possibly empty) of
    further clips of that voice of any length the spectrogram accepts -- the reference's aux_ref_audio_paths, to which the
    3 .. 10 s rule does not apply.  All clips, main and aux, are padded into one buffer, uploaded once and go through one
    ref_spec_rows and one style_rows; a voice's style is the mean over its clips' vectors, as decode averages a list of
    references (the vector itself without aux clips).
    The prompt's 16 kHz clips come from one resample_pack 32 -> 16 kHz of the main clips (as FeatureWriter.ssl_batch), or
    are clips16k where the caller has the reference's own librosa.load(sr=16000) result.  The two differ by the resampler:
    the reference's librosa.load resamples the FILE from its native rate in one step (librosa 0.9.2: resampy's kaiser_best
    in float64), this module the 32 kHz clip -- itself a resampled file -- with the same filter accumulated in fp32
    (hip/audio.py); the two 16 kHz clips are not the same samples, and no token parity between them is claimed.
    An entry of clips32k or aux may also be the path of a WAV file (audiokit/wav.py: any served encoding, channel count and
    rate): the 3 .. 10 s rule is then checked on frames / rate from the header, the files' bytes are uploaded once and
    ingested at the model's rate next to the arrays (hip/audio.py::ingest_pcm), and -- clips16k being None -- the prompt clip
    of a main clip given as a file is ingested from the same upload at 16 kHz directly: one step from the file's own rate,
    librosa.load's operator with fp32 accumulation.  Clips given as arrays keep the 32 -> 16 kHz step.
    -> one EnrolledVoice per voice, in order."""
    if not clips32k:
        return []
    rate = int(voice.sampling_rate)
    nv = len(clips32k)
    entries, owner = list(clips32k), list(range(nv))
    for v, extra in enumerate(aux if aux is not None and len(aux) == nv else []):
        for c in extra or []:
            entries.append(c)
            owner.append(v)
    files = [b for b, c in enumerate(entries) if isinstance(c, (str, os.PathLike))]
    infos = {b: wav.probe(entries[b]) for b in files}
    rows = [None if b in infos else torch.as_tensor(c, dtype=torch.float32).reshape(-1) for b, c in enumerate(entries)]
    for v in range(nv):                # the reference's rule, on the clip at the model's rate or on the header's frames / rate
        n, r = (infos[v].frames, infos[v].rate) if v in infos else (rows[v].numel(), rate)
        if n * 16000 > PROMPT_MAX * r or n * 16000 < PROMPT_MIN * r:
            raise OSError(f"reference clip {v}: audio length should be in 3~10 seconds.")
    if aux is not None and len(aux) != nv:
        raise ValueError(f"aux has {len(aux)} entries for {nv} voices")
    if clips16k is not None and len(clips16k) != nv:
        raise ValueError(f"clips16k has {len(clips16k)} entries for {nv} voices")
    if int(voice.filter_length) != 2048 or int(voice.win_length) != 2048:
        raise L.EvtError("enroll_voices: the spectrogram kernel serves filter_length = win_length = 2048 (configs/s2.json)")
    from ..hip.audio import ingest_pcm, out_len, rate_ratio, ref_spec_rows, resample_pack, upload_raw

    main_files = [b for b in files if b < nv] if clips16k is None else []
    for b in files:                                         # EvtError for a rate that is not served, before any upload
        rate_ratio(infos[b].rate, rate)
    for b in main_files:
        rate_ratio(infos[b].rate, 16000)
    lens = [out_len(infos[b].frames, *rate_ratio(infos[b].rate, rate)) if b in infos else int(rows[b].numel())
            for b in range(len(entries))]
    host = torch.zeros(len(entries), max(lens), dtype=torch.float32)
    for b, c in enumerate(rows):
        if c is not None:
            host[b, :lens[b]] = c

    L.set_half(voice.dtype)
    with torch.no_grad():
        x = host.to(voice.device)
        if files:                                           # one upload of the files' bytes; a launch per input rate
            batch = wav.stage([entries[b] for b in files], infos=[infos[b] for b in files])
            raw_dev = upload_raw(batch, voice.device)
            ingest_pcm(batch, rate, voice.device, raw_dev=raw_dev, out=x.view(-1),
                       offsets=[b * x.size(1) for b in files])
        lens_dev = torch.tensor(lens, dtype=torch.int32).to(voice.device)
        bins = 704 if voice.model.version != "v1" else voice.model.spec_channels
        spec, frames, _peak = ref_spec_rows(x, lens, hop=int(voice.hop_length), bins=bins, lens_dev=lens_dev)
        ge = voice.style_rows(spec, frames)                                          # [rows, gin]
        styles = []
        for v in range(nv):
            mine = [b for b, o in enumerate(owner) if o == v]
            styles.append(ge[v:v + 1] if len(mine) == 1 else torch.stack([ge[b:b + 1] for b in mine], 0).mean(0))
        if clips16k is None and not main_files:
            packed = resample_pack(x[:nv], lens[:nv], 1, rate, 16000, "float32", lens_dev=lens_dev[:nv].contiguous())
            wavs16k = [packed.row(v) for v in range(nv)]
        elif clips16k is None:
            # a main clip that is a file: its prompt clip straight from the file's own rate, as librosa.load(sr=16000) does
            wavs16k = [None] * nv
            direct = ingest_pcm(batch.subset([files.index(v) for v in main_files]), 16000, voice.device, raw_dev=raw_dev)
            for k, v in enumerate(main_files):
                wavs16k[v] = direct.row(k)
            arrays = [v for v in range(nv) if v not in infos]
            if arrays:
                packed = resample_pack(x[arrays].contiguous(), [lens[v] for v in arrays], 1, rate, 16000, "float32")
                for k, v in enumerate(arrays):
                    wavs16k[v] = packed.row(k)
        else:
            wavs16k = [torch.as_tensor(c, dtype=torch.float32).reshape(-1).to(voice.device) for c in clips16k]
        prompts = prompt_semantics(hubert, voice.extract_latent, wavs16k)
    return [EnrolledVoice(styles[v], prompts[v], frames[v]) for v in range(nv)]
