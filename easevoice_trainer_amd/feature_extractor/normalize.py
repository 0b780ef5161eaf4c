"""The `ssl` and `text` steps of the reference's normalisation (src/normalization/normalize.py:65-180) with the two models on
the GPU: per clip 4-cnhubert/<name>.pt ([1, 768, T] float32) and 5-wav32k/<name> (int16, 32 kHz); per Chinese sentence
3-bert/<name>.pt ([1024, n_phones] float32) and the line of 2-name2text.txt.  File names and tensor layouts are the
reference's (src/utils/config/__init__.py:27-31), so train/dataset.py -- and the reference's own readers -- load them.

What stays outside (host-side text / audio plumbing of the reference, not arithmetic of this path): decoding the source file
to 32 kHz float (ffmpeg, src/utils/audio/__init__.py:13-32), the text cleaner / g2p (src/easevoice/text) and the tokenizer:
the callers hand over the decoded clip, and `input_ids` + `word2ph` + the cleaned `phones` / `norm_text`.

Resampling 32 kHz -> 16 kHz: the reference calls librosa.resample (normalize.py:154-156; librosa 0.9.2, uv.lock:1805-1806,
default res_type "kaiser_best" = resampy's windowed-sinc interpolator).  librosa / resampy are third-party packages that are
not under /root/reference: `resample_half` restates resampy's published algorithm for the ratio 1/2, where its
interpolation table is only ever read at every 256th entry and the interpolator degenerates to a symmetric 255-tap FIR
(64 zero crossings, roll-off 0.9475937167399596, Kaiser beta 14.769656459379492, gain 1/2) followed by taking every second
sample.  Parity of this one function is UNPINNED (no golden vector in the reference, package absent); it is checked against
its own definition and against the ideal half-band behaviour (tests/test_feature_extractors_cpu.py).

`FeatureWriter.ssl_batch` is `ssl` for a group of clips: peak, rescaling and resampling on the GPU (hip/feat.py::
clip_rescale_rows, hip/audio.py::resample_pack at 1/2) and one ragged pass of the model (CNHubert.batch)."""
import os

import numpy as np
import torch

MAXX, ALPHA = 0.95, 0.5                  # normalize.py:61-62
_ROLLOFF, _BETA, _ZEROS, _PRECISION = 0.9475937167399596, 14.769656459379492, 64, 9


def _half_band_taps():
    """h[j], j = 0 .. 127: resampy's kaiser_best table (sinc_window(num_zeros=64, precision=9, kaiser(beta), rolloff)) at the
    entries a ratio of exactly 1/2 reads (index 256 j), times the sample ratio"""
    n = (2 ** _PRECISION) * _ZEROS
    step = 2 ** (_PRECISION - 1)
    j = np.arange(0, n + 1, step)[: 2 * _ZEROS]
    sinc = _ROLLOFF * np.sinc(_ROLLOFF * j / float(2 ** _PRECISION))
    taper = np.kaiser(2 * n + 1, _BETA)[n:][j]
    return 0.5 * sinc * taper


def resample_half(x: np.ndarray) -> np.ndarray:
    """32 kHz -> 16 kHz: y[t] = sum_{|j| <= 127} h[|j|] x[2 t + j], samples outside the clip are zeros, int(n / 2) outputs"""
    h = _half_band_taps()
    taps = np.concatenate([h[:0:-1], h]).astype(np.float64)            # j = -127 .. 127
    n_out = int(len(x) * 0.5)
    xp = np.concatenate([np.zeros(127), np.asarray(x, dtype=np.float64), np.zeros(128)])
    t = torch.from_numpy(xp)[None, None]
    y = torch.nn.functional.conv1d(t, torch.from_numpy(taps[::-1].copy())[None, None], stride=2)[0, 0]
    return y[:n_out].numpy().astype(np.float32)


def rescale_clip(audio32k: np.ndarray):
    """normalize.py:148-153 -> (the int16 clip written to 5-wav32k, the float clip that is resampled for HuBERT), or None for
    a clip the reference skips (peak above 2.2)"""
    tmp_max = np.abs(audio32k).max()
    if tmp_max > 2.2:
        return None
    a32 = (audio32k / tmp_max * (MAXX * ALPHA * 32768)) + ((1 - ALPHA) * 32768) * audio32k
    a32b = (audio32k / tmp_max * (MAXX * ALPHA * 1145.14)) + ((1 - ALPHA) * 1145.14) * audio32k
    return a32.astype("int16"), a32b.astype(np.float32)


class FeatureWriter:
    """writes the feature directory of one data set: `ssl(name, audio32k)` and `text(name, ...)` per item, `close()` writes
    2-name2text.txt.  hubert: feature_extractor.CNHubert (or any callable wav16k [n] -> [1, 768, T]); bert:
    feature_extractor.BertFeatures (or any object with phone_level_feature(input_ids, word2ph); `text_batch` takes a list of
    items through its phone_level_features_batch(ids_list, word2ph_list, group=))."""

    def __init__(self, out_dir, hubert=None, bert=None, voice=None):
        self.out_dir, self.hubert, self.bert, self.voice = out_dir, hubert, bert, voice
        self.bert_dir = os.path.join(out_dir, "3-bert")
        self.hubert_dir = os.path.join(out_dir, "4-cnhubert")
        self.wav_dir = os.path.join(out_dir, "5-wav32k")
        for d in (self.bert_dir, self.hubert_dir, self.wav_dir):
            os.makedirs(d, exist_ok=True)
        self._text_lines = []
        self._codes = {}                 # name -> semantic codes kept by ssl_batch(tokens=True) for write_semantic

    def ssl(self, name, audio32k) -> bool:
        """normalize.py:_name2go: False when the features came out non-finite (the reference then retries in fp32)"""
        from scipy.io import wavfile

        path = os.path.join(self.hubert_dir, name + ".pt")
        if os.path.exists(path):
            return True
        pair = rescale_clip(np.asarray(audio32k, dtype=np.float32))
        if pair is None:
            return True
        wav_int16, for_hubert = pair
        ssl = self.hubert(resample_half(for_hubert))
        if not bool(torch.isfinite(ssl).all()):
            return False
        wavfile.write(os.path.join(self.wav_dir, name), 32000, wav_int16)
        torch.save(ssl, path)
        return True

    def _front_rows(self, clips):
        """the device half of `ssl_batch` in front of the model: clips (1-D float32 arrays, 32 kHz) -> (peaks, the int16
        clips for 5-wav32k, the 16 kHz clips as zero-filled rows [B, N16] on the GPU, their lengths).  One upload, one
        hip/feat.py::clip_rescale_rows, one hip/audio.py::resample_pack (32000 -> 16000, float32, no gap: resample_half's
        operator), peaks and int16 rows back in one copy each."""
        from ..hip.audio import ingest_pcm, out_len, rate_ratio, resample_pack
        from ..hip.feat import clip_rescale_rows

        device = self.hubert.device
        files = [b for b, c in enumerate(clips) if isinstance(c, str)]
        if files:                                  # WAV files: headers first (a rate that is not served is an EvtError here)
            from ..audiokit import wav

            infos = [wav.probe(clips[b]) for b in files]
            of_file = {b: out_len(i.frames, *rate_ratio(i.rate, 32000)) for b, i in zip(files, infos)}
        lens = [of_file[b] if isinstance(c, str) else len(c) for b, c in enumerate(clips)]
        host = np.zeros((len(clips), max(lens)), dtype=np.float32)
        for b, c in enumerate(clips):
            if not isinstance(c, str):
                host[b, :lens[b]] = c
        x = torch.from_numpy(host).to(device)
        if files:                                  # their bytes uploaded once, decoded and resampled into their rows of x
            ingest_pcm(wav.stage([clips[b] for b in files], infos=infos), 32000, device, out=x.view(-1),
                       offsets=[b * x.size(1) for b in files])
        lens_dev = torch.tensor(lens, dtype=torch.int32).to(device)
        with torch.no_grad():
            f, q, peak = clip_rescale_rows(x, lens_dev)
            packed = resample_pack(f, lens, 1, 32000, 16000, "float32", interval=0.0, lens_dev=lens_dev)
            rows16 = torch.zeros(len(clips), max(max(packed.lengths), 1), dtype=torch.float32, device=device)
            for b in range(len(clips)):
                rows16[b, :packed.lengths[b]] = packed.row(b)
        q = q.cpu().numpy()
        return peak.cpu().tolist(), [q[b, :lens[b]] for b in range(len(clips))], rows16, list(packed.lengths)

    def ssl_batch(self, names, clips32k, tokens=False) -> list:
        """`ssl` for several clips with ONE pass of the model over the ragged batch (hubert: feature_extractor.CNHubert, or
        any object with its `device` and `batch((rows [B, N], lengths))`).  Per name what `ssl` returns: True for a name
        whose feature file exists (skipped before anything is uploaded) and for a clip the reference skips (peak above
        2.2, nothing written), False for a non-finite peak or non-finite features (nothing written), True after writing
        4-cnhubert/<name>.pt and 5-wav32k/<name>.  The int16 file is byte for byte `ssl`'s; the features differ from
        `ssl`'s within fp32 rounding (the resampler accumulates in fp32, resample_half in float64).
        An entry of clips32k may be the path of a WAV file (audiokit/wav.py: any served encoding, channel count and rate)
        in place of the array: it is read only when its name is not skipped, and decoded and resampled to 32 kHz on the GPU
        (hip/audio.py::ingest_pcm) -- the clip load_audio_batch([path], 32000) gives.
        tokens=True (needs `voice`, an object with SoVITSVoice.extract_latent_rows, and a hubert with
        last_hidden_state_batch; ValueError otherwise, before anything is uploaded): the features of the items that are
        written also go through voice.extract_latent_rows while they are on the device -- as the float32 values that are
        saved, so the codes are the codes of the file -- and are kept per name for `write_semantic`.  Items that are
        skipped or refused get no codes; the return value and the files are the same."""
        from scipy.io import wavfile

        if tokens and (self.voice is None or not hasattr(self.voice, "extract_latent_rows")
                       or not hasattr(self.hubert, "last_hidden_state_batch")):
            raise ValueError("ssl_batch(tokens=True) needs a voice with extract_latent_rows and a hubert with "
                             "last_hidden_state_batch")
        names = list(names)
        if len(names) != len(clips32k):
            raise ValueError(f"{len(names)} names for {len(clips32k)} clips")
        done = [True] * len(names)
        todo = [i for i, name in enumerate(names) if not os.path.exists(os.path.join(self.hubert_dir, name + ".pt"))]
        if not todo:
            return done
        clips = [os.fspath(clips32k[i]) if isinstance(clips32k[i], (str, os.PathLike))
                 else np.asarray(clips32k[i], dtype=np.float32).reshape(-1) for i in todo]
        peaks, wav16, rows16, lens16 = self._front_rows(clips)
        keep = []
        for j, i in enumerate(todo):
            if not np.isfinite(peaks[j]):
                done[i] = False
            elif not peaks[j] > 2.2:
                keep.append(j)
        if not keep:
            return done
        if len(keep) < len(todo):
            rows16 = rows16[torch.tensor(keep, device=rows16.device)]
        codes = None
        if tokens:
            from ..inference.semantic import codes_to_host
            from .cnhubert import rows_to_feats

            with torch.no_grad():
                hs, frame_lens = self.hubert.last_hidden_state_batch((rows16, [lens16[j] for j in keep]))
                hs = hs.float().contiguous()                                    # the values CNHubert.batch saves
                codes = codes_to_host(self.voice.extract_latent_rows(hs, frame_lens))
            feats = rows_to_feats(hs, frame_lens)                               # what CNHubert.batch returns
        else:
            feats = self.hubert.batch((rows16, [lens16[j] for j in keep]))
        for n, (j, ssl) in enumerate(zip(keep, feats)):
            i = todo[j]
            if not bool(torch.isfinite(ssl).all()):
                done[i] = False
                continue
            if codes is not None:
                self._codes[names[i]] = codes[n]
            wavfile.write(os.path.join(self.wav_dir, names[i]), 32000, wav16[j])
            torch.save(ssl, os.path.join(self.hubert_dir, names[i] + ".pt"))
        return done

    def text(self, name, phones, word2ph, norm_text, language="zh", input_ids=None):
        """normalize.py:_process_text: the BERT feature only for Chinese items that do not have one yet; always the text line"""
        path = os.path.join(self.bert_dir, name + ".pt")
        if not os.path.exists(path) and language == "zh":
            feat = self.bert.phone_level_feature(input_ids, word2ph)
            if feat.shape[-1] != len(phones):
                raise ValueError("bert_feature and phones not match")          # normalize.py:123-124
            torch.save(feat, path)
        self._text_lines.append("%s\t%s\t%s\t%s" % (name, " ".join(phones), word2ph, norm_text))

    def text_batch(self, items, group=16) -> None:
        """`text` for a list of (name, phones, word2ph, norm_text, language, input_ids): the items that `text` would send
        through BERT -- Chinese ones without a 3-bert/<name>.pt -- go through bert.phone_level_features_batch in groups
        of at most `group` (everything else is dropped before anything is uploaded; nothing is launched when none is left),
        every feature is checked against its item's phones and written as `text` writes it (float32 [1024, n] on the CPU),
        and the text lines of ALL items are appended in input order."""
        items = [tuple(it) for it in items]
        todo, seen = [], set()
        for i, (name, _phones, _word2ph, _norm_text, language, _ids) in enumerate(items):
            if language == "zh" and name not in seen and not os.path.exists(os.path.join(self.bert_dir, name + ".pt")):
                todo.append(i)
                seen.add(name)             # a name given twice is written once, as by two calls of `text`
        if todo:
            ids = [torch.as_tensor(items[i][5]).reshape(-1) for i in todo]
            feats = self.bert.phone_level_features_batch(ids, [list(items[i][2]) for i in todo], group=group)
            for i, feat in zip(todo, feats):
                if feat.shape[-1] != len(items[i][1]):
                    raise ValueError(f"bert_feature and phones not match (item {i}: {items[i][0]})")
            for i, feat in zip(todo, feats):
                torch.save(feat.float().clone(), os.path.join(self.bert_dir, items[i][0] + ".pt"))
        for name, phones, word2ph, norm_text, _language, _ids in items:
            self._text_lines.append("%s\t%s\t%s\t%s" % (name, " ".join(phones), word2ph, norm_text))

    def write_semantic(self, names, group=16) -> int:
        """the `token` step (normalize.py:181-211): 6-name2semantic.tsv in the order of `names`, in write_semantic_tsv's
        format.  A name whose codes `ssl_batch(tokens=True)` kept takes those; any other name with a 4-cnhubert/<name>.pt is
        tokenised from the file, in groups of at most `group` (inference/semantic.py::codes_of_files, needs `voice`); a name
        with neither is skipped.  -> the number of lines written."""
        from ..inference.semantic import codes_of_files, semantic_line

        names = list(names)
        path = lambda n: os.path.join(self.hubert_dir, n + ".pt")
        files = [n for n in dict.fromkeys(names) if n not in self._codes and os.path.exists(path(n))]
        got = dict(self._codes)
        if files:
            if self.voice is None:
                raise ValueError("write_semantic needs a voice to tokenise feature files")
            device = getattr(self.voice, "device", None) or getattr(self.hubert, "device", "cuda:0")
            got.update(zip(files, codes_of_files(self.voice.extract_latent_rows, [path(n) for n in files], group, device)))
        lines = [semantic_line(n, got[n]) for n in names if n in got]
        with open(os.path.join(self.out_dir, "6-name2semantic.tsv"), "w", encoding="utf8") as f:
            f.write("\n".join(["item_name\tsemantic_audio"] + lines) + "\n")
        return len(lines)

    def close(self):
        with open(os.path.join(self.out_dir, "2-name2text.txt"), "w", encoding="utf8") as f:
            f.write("\n".join(self._text_lines) + "\n")
