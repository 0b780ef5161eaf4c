"""RIFF/WAVE files as the pipeline's input: `probe` reads a header, `stage` reads the sample bytes of several files into one
page-locked buffer that hip/audio.py::ingest_pcm uploads once and decodes, mixes down and resamples on the GPU
(csrc/pcm_ingest.hip; include/evt.h has the operator).  Host only: nothing here needs a device.

Served: unsigned 8-bit PCM, signed little-endian 16-, 24- (3 packed bytes) and 32-bit PCM, IEEE float32 and float64, with 1
to 8 channels at any rate, under format tag 1, 3 or WAVE_FORMAT_EXTENSIBLE.  Not served, a ValueError naming the file and
the reason: big-endian RIFX, RF64, A-law, mu-law, ADPCM and every other tag.  Compressed containers (mp3, flac, ogg) stay
out of scope: they need a decoder in front, as before.

train/dataset.py::read_wav_pcm16, the training reader of 5-wav32k, is a different function and stays as it is."""
import os
import struct
from dataclasses import dataclass
from typing import Dict, List, NamedTuple

U8, S16, S24, S32, F32, F64 = range(6)          # EVT_PCM_IN_* of include/evt.h
FORMAT_NAMES = ("u8", "s16", "s24", "s32", "f32", "f64")
SAMPLE_BYTES = (1, 2, 3, 4, 4, 8)
MAX_CHANNELS = 8                                  # EVT_PCM_IN_MAX_CHANNELS
ALIGN = 16                                        # a recording's first byte in the staged buffer
_PCM_BITS = {8: U8, 16: S16, 24: S24, 32: S32}
_FLOAT_BITS = {32: F32, 64: F64}
_REFUSED_TAGS = {2: "Microsoft ADPCM", 6: "A-law", 7: "mu-law", 0x11: "IMA ADPCM", 0x55: "MPEG layer 3"}


class WavInfo(NamedTuple):
    fmt: int             # U8 .. F64
    channels: int
    rate: int
    frames: int          # whole frames in the file
    data_pos: int        # position of the first sample byte in the file
    data_bytes: int      # frames * channels * SAMPLE_BYTES[fmt]: a trailing partial frame is not counted


def probe(path) -> WavInfo:
    """The header of a RIFF/WAVE file.  `fmt ` chunks of 16, 18 or 40 bytes; with WAVE_FORMAT_EXTENSIBLE (0xFFFE) the
    encoding is the first two bytes of the sub-format GUID.  Chunks in front of `data` (LIST, fact, bext, ...) are skipped,
    an odd-sized chunk carries a pad byte.  A `data` size of 0 or 0xFFFFFFFF (a streamed file whose writer never came back
    to the header) means "to the end of the file", a `data` chunk longer than the file is cut to the file, a trailing
    partial frame is dropped.  ValueError naming the path and the reason for everything the module does not serve."""
    path = os.fspath(path)

    def refuse(why):
        return ValueError(f"{path}: {why}")

    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if len(head) == 12 and head[:4] == b"RIFX":
            raise refuse("big-endian RIFX is not served")
        if len(head) == 12 and head[:4] == b"RF64":
            raise refuse("RF64 is not served")
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise refuse("not a RIFF/WAVE file")
        pos, fmt = 12, None
        while True:
            f.seek(pos)
            chunk = f.read(8)
            if len(chunk) < 8:
                raise refuse("missing fmt/data chunk")
            cid, csize = chunk[:4], struct.unpack("<I", chunk[4:])[0]
            if cid == b"data":
                break
            if cid == b"fmt ":
                fmt = f.read(min(csize, 40))
                if len(fmt) < 16:
                    raise refuse(f"fmt chunk of {csize} bytes")
            pos += 8 + csize + (csize & 1)
    if fmt is None:
        raise refuse("no fmt chunk in front of the data chunk")
    tag, channels, rate, _byte_rate, block, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == 0xFFFE:
        if len(fmt) < 40:
            raise refuse(f"WAVE_FORMAT_EXTENSIBLE with a fmt chunk of {len(fmt)} bytes")
        tag = struct.unpack_from("<H", fmt, 24)[0]
    if tag == 1 and bits in _PCM_BITS:
        code = _PCM_BITS[bits]
    elif tag == 3 and bits in _FLOAT_BITS:
        code = _FLOAT_BITS[bits]
    elif tag in _REFUSED_TAGS:
        raise refuse(f"{_REFUSED_TAGS[tag]} (format tag {tag}) is not served")
    else:
        raise refuse(f"format tag {tag} with {bits} bits per sample is not served")
    if not 1 <= channels <= MAX_CHANNELS:
        raise refuse(f"{channels} channels: 1 .. {MAX_CHANNELS} are served")
    if block != channels * SAMPLE_BYTES[code]:
        raise refuse(f"block align {block} is not channels * bytes per sample = {channels * SAMPLE_BYTES[code]}")
    if rate <= 0 or rate >= 1 << 31:
        raise refuse(f"sample rate {rate}")
    data_pos = pos + 8
    have = max(size - data_pos, 0)
    nbytes = have if csize in (0, 0xFFFFFFFF) else min(csize, have)
    frames = nbytes // block
    if frames >= 1 << 31:
        raise refuse(f"{frames} frames: 2^31 or more are not served")
    return WavInfo(code, channels, rate, frames, data_pos, frames * block)


@dataclass
class RawBatch:
    """raw: 1-D uint8 tensor (page-locked where the process has a GPU) with the recordings' sample bytes, recording r at
    raw[byte_off[r] : byte_off[r] + infos[r].data_bytes], every byte_off a multiple of 16 and the last recording ending at
    raw's end; by_rate: the recordings' indices grouped by the files' rate, in input order."""
    raw: object
    infos: List[WavInfo]
    byte_off: List[int]
    by_rate: Dict[int, List[int]]

    def __len__(self):
        return len(self.infos)

    def subset(self, rows):
        """the same buffer with the table cut to `rows` (indices into this batch), in that order"""
        rows = [int(r) for r in rows]
        by_rate = {}
        for k, r in enumerate(rows):
            by_rate.setdefault(self.infos[r].rate, []).append(k)
        return RawBatch(self.raw, [self.infos[r] for r in rows], [self.byte_off[r] for r in rows], by_rate)


def stage(paths, filler=0, infos=None) -> RawBatch:
    """The `data` bytes of all files back to back in one uint8 buffer, each start rounded up to 16 bytes, read straight into
    the buffer (readinto: no intermediate copy).  filler: the value of the at most 15 bytes between two recordings -- an int
    0 .. 255 or a bytes pattern that repeats from the buffer's byte 0; no consumer reads them.  infos: the files' probe()
    results where the caller has them."""
    import torch

    paths = [os.fspath(p) for p in paths]
    infos = [probe(p) for p in paths] if infos is None else list(infos)
    if len(infos) != len(paths):
        raise ValueError(f"{len(infos)} headers for {len(paths)} files")
    pattern = bytes([filler]) if isinstance(filler, int) else bytes(filler)
    if not pattern:
        raise ValueError("filler is an int 0 .. 255 or a non-empty bytes pattern")
    byte_off, end, by_rate = [], 0, {}
    for r, info in enumerate(infos):
        start = -(-end // ALIGN) * ALIGN
        byte_off.append(start)
        end = start + info.data_bytes
        by_rate.setdefault(info.rate, []).append(r)
    raw = torch.empty(end, dtype=torch.uint8, pin_memory=end > 0 and torch.cuda.is_available())
    view = memoryview(raw.numpy()) if end else memoryview(b"")
    at = 0
    for path, info, start in zip(paths, infos, byte_off):
        if start > at:
            view[at:start] = bytes(pattern[i % len(pattern)] for i in range(at, start))
        with open(path, "rb") as f:
            f.seek(info.data_pos)
            got = f.readinto(view[start:start + info.data_bytes]) if info.data_bytes else 0
        if got != info.data_bytes:
            raise ValueError(f"{path}: {got} of {info.data_bytes} sample bytes could be read")
        at = start + info.data_bytes
    return RawBatch(raw, infos, byte_off, by_rate)
