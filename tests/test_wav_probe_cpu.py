"""audiokit/wav.py on the host: probe() returns the fields a file was written with (tests/ingest_refs.py writes the files with
struct), for every encoding and header form and the irregular files people have; scipy.io.wavfile agrees where it reads the
file; stage() places each file's sample bytes at a 16-byte-aligned offset; everything not served is a ValueError naming the
path."""
import struct
import warnings

import numpy as np
import pytest

import ingest_refs as R

ENCODINGS = [R.U8, R.S16, R.S24, R.S32, R.F32, R.F64]


def _scipy_agrees(path, info):
    from scipy.io import wavfile

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rate, data = wavfile.read(path)
    assert rate == info.rate and data.shape[0] == info.frames
    assert (1 if data.ndim == 1 else data.shape[1]) == info.channels


@pytest.mark.parametrize("form", ["plain", "fmt18", "ext"])
@pytest.mark.parametrize("fmt", ENCODINGS, ids=R.NAMES)
def test_probe_returns_what_was_written(tmp_path, fmt, form):
    from easevoice_trainer_amd.audiokit import wav

    for channels, rate, frames in ((1, 32000, 7), (2, 44100, 5), (8, 96000, 3), (3, 8000, 0)):
        data = R.sample_bytes(R.samples_of(fmt, frames, channels, 1), fmt)
        path = str(tmp_path / f"{R.NAMES[fmt]}_{form}_{channels}.wav")
        pos = R.wav_file(path, data, fmt, channels, rate, form)
        info = wav.probe(path)
        assert info == wav.WavInfo(fmt, channels, rate, frames, pos, frames * channels * R.WIDTH[fmt])
        assert (wav.U8, wav.S16, wav.S24, wav.S32, wav.F32, wav.F64)[fmt] == fmt and wav.SAMPLE_BYTES[fmt] == R.WIDTH[fmt]
        if frames:
            _scipy_agrees(path, info)


def test_chunks_in_front_pad_bytes_and_irregular_data_sizes(tmp_path):
    from easevoice_trainer_amd.audiokit import wav

    x = R.ints(R.S16, 10, 2, 3)
    data = R.sample_bytes(x, R.S16)
    path = str(tmp_path / "a.wav")
    # LIST in front of data, and an odd-sized chunk with its pad byte
    before = R.chunk(b"LIST", b"INFOISFT\x04\0\0\0abc\0") + R.chunk(b"bext", b"x" * 7) + R.chunk(b"fact", struct.pack("<I", 10))
    assert len(R.chunk(b"bext", b"x" * 7)) == 16
    pos = R.wav_file(path, data, R.S16, 2, 48000, before=before)
    info = wav.probe(path)
    assert info == wav.WavInfo(R.S16, 2, 48000, 10, pos, 40)
    _scipy_agrees(path, info)
    with open(path, "rb") as f:
        f.seek(info.data_pos)
        assert f.read(info.data_bytes) == data
    # data size 0 and 0xFFFFFFFF: to the end of the file
    for size in (0, 0xFFFFFFFF):
        pos = R.wav_file(path, data, R.S16, 2, 48000, data_size=size)
        assert wav.probe(path) == wav.WavInfo(R.S16, 2, 48000, 10, pos, 40), size
    # a data size beyond the file: cut to the file
    pos = R.wav_file(path, data, R.S16, 2, 48000, data_size=4000)
    assert wav.probe(path) == wav.WavInfo(R.S16, 2, 48000, 10, pos, 40)
    # a trailing partial frame is dropped, in the chunk's own size and at the end of a cut file
    pos = R.wav_file(path, data + b"\x01\x02\x03", R.S16, 2, 48000)
    assert wav.probe(path) == wav.WavInfo(R.S16, 2, 48000, 10, pos, 40)
    pos = R.wav_file(path, data[:-1], R.S16, 2, 48000, data_size=0)
    assert wav.probe(path) == wav.WavInfo(R.S16, 2, 48000, 9, pos, 36)
    # a chunk behind the data does not count as samples
    pos = R.wav_file(path, data, R.S16, 2, 48000, after=R.chunk(b"LIST", b"INFO"))
    info = wav.probe(path)
    assert info == wav.WavInfo(R.S16, 2, 48000, 10, pos, 40)
    _scipy_agrees(path, info)


def test_stage_places_the_data_bytes_at_aligned_offsets(tmp_path):
    from easevoice_trainer_amd.audiokit import wav

    specs = [(R.S16, 2, 48000, 5), (R.S24, 1, 44100, 7), (R.U8, 3, 48000, 1), (R.F64, 1, 8000, 0), (R.F32, 2, 44100, 3)]
    paths, datas = [], []
    for k, (fmt, channels, rate, frames) in enumerate(specs):
        datas.append(R.sample_bytes(R.samples_of(fmt, frames, channels, k), fmt))
        paths.append(str(tmp_path / f"{k}.wav"))
        R.wav_file(paths[-1], datas[-1] + (b"\x07" if k == 1 else b""), fmt, channels, rate,
                   before=R.chunk(b"LIST", b"abc") if k % 2 else b"")
    nan = struct.pack("<f", float("nan"))
    for filler in (0, 0xFF, nan):
        batch = wav.stage(paths, filler=filler)
        raw = bytes(batch.raw.numpy())
        assert len(batch) == 5 and batch.raw.dtype.is_floating_point is False and batch.raw.dim() == 1
        assert batch.byte_off == [0, 32, 64, 80, 80] and len(raw) == 80 + len(datas[4])    # the last one ends the buffer
        live = np.zeros(len(raw), dtype=bool)
        for off, info, data in zip(batch.byte_off, batch.infos, datas):
            assert off % 16 == 0 and info.data_bytes == len(data) and raw[off:off + len(data)] == data
            live[off:off + len(data)] = True
        pattern = bytes([filler]) if isinstance(filler, int) else filler
        assert all(raw[i] == pattern[i % len(pattern)] for i in np.flatnonzero(~live))
        assert batch.by_rate == {48000: [0, 2], 44100: [1, 4], 8000: [3]}
    sub = batch.subset([4, 0])
    assert sub.raw is batch.raw and sub.byte_off == [80, 0] and sub.by_rate == {44100: [0], 48000: [1]}
    assert sub.infos == [batch.infos[4], batch.infos[0]]
    empty = wav.stage([])
    assert len(empty) == 0 and empty.raw.numel() == 0


def test_everything_else_is_a_value_error_naming_the_path(tmp_path):
    from easevoice_trainer_amd.audiokit import wav

    data = R.sample_bytes(R.ints(R.S16, 4, 2, 0), R.S16)
    path = str(tmp_path / "refused.wav")
    cases = [dict(magic=b"RIFX"), dict(magic=b"RF64"), dict(magic=b"FORM"),
             dict(tag=6, bits=8), dict(tag=7, bits=8), dict(tag=2, bits=4), dict(tag=0x11, bits=4),      # A-law, mu-law, ADPCM
             dict(form="ext", tag=6, bits=8),
             dict(block=5), dict(block=2), dict(rate=0), dict(channels=0), dict(channels=9),
             dict(bits=12), dict(tag=3, bits=16), dict(tag=1, bits=64)]
    for case in cases:
        kw = dict(case)
        channels, rate = kw.pop("channels", 2), kw.pop("rate", 32000)
        R.wav_file(path, data, R.S16, channels, rate, **kw)
        with pytest.raises(ValueError, match="refused.wav"):
            wav.probe(path)
    with open(path, "wb") as f:                                   # not RIFF at all, and a file that ends in the header
        f.write(b"ID3\x03" + b"\0" * 64)
    with pytest.raises(ValueError, match="refused.wav"):
        wav.probe(path)
    with open(path, "wb") as f:
        f.write(b"RIFF\x24\0\0\0WAVE" + R.fmt_chunk(R.S16, 1, 32000))
    with pytest.raises(ValueError, match="refused.wav"):
        wav.probe(path)
    with open(path, "wb") as f:                                   # data in front of fmt
        f.write(b"RIFF\x24\0\0\0WAVE" + R.chunk(b"data", data) + R.fmt_chunk(R.S16, 2, 32000))
    with pytest.raises(ValueError, match="refused.wav"):
        wav.probe(path)
    with pytest.raises(ValueError, match="refused.wav"):
        wav.stage([path])


def test_two_to_the_31_frames_are_refused_without_such_a_file(tmp_path):
    """a sparse file: the header of an 8-bit mono recording and 2^31 bytes of hole behind it"""
    from easevoice_trainer_amd.audiokit import wav

    path = str(tmp_path / "huge.wav")
    pos = R.wav_file(path, b"", R.U8, 1, 8000, data_size=0)
    with open(path, "r+b") as f:
        f.truncate(pos + 2 ** 31 - 1)
    assert wav.probe(path).frames == 2 ** 31 - 1
    with open(path, "r+b") as f:
        f.truncate(pos + 2 ** 31)
    with pytest.raises(ValueError, match="huge.wav"):
        wav.probe(path)


def test_read_wav_pcm16_files_decode_to_the_same_samples():
    """the numpy statement of the operator equals train/dataset.py::read_wav_pcm16's arithmetic for PCM16, C = 1 .. 8: the
    sequential float32 sum and numpy's mean(axis=1, dtype=float32) are the same bits"""
    for channels in range(1, 9):
        x = R.ints(R.S16, 4001, channels, channels)
        v = x.astype("<i2").astype(np.float32) * np.float32(1.0 / 32768.0)
        want = v.reshape(-1) if channels == 1 else v.reshape(-1, channels).mean(axis=1, dtype=np.float32)
        assert np.array_equal(R.mono(x, R.S16), want), channels
