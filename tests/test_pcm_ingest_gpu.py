"""GPU: evt_pcm_ingest_rows (csrc/pcm_ingest.hip) -- the sample bytes of WAV files decoded, mixed down to mono and resampled
into one packed fp32 buffer -- and its binding hip/audio.py::ingest_pcm / load_audio_batch.

The files are written by tests/ingest_refs.py with struct, staged by audiokit/wav.py::stage and launched through the C entry
point on a buffer that holds 77 before the launch and has 8 elements behind sum(To).  The numpy statement of decode and
downmix (ingest_refs.mono) is the yardstick of the exact tests, the float64 oracle (tests/resample_oracle.py) on those fp32
values the yardstick of the resampling, with the bound tests/test_resample_pack_gpu.py derives for the same arithmetic:
|got - want| <= 2^-24 (Jm + 3) A[m] while 2 R + 1 <= 513."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import ingest_refs as R

pytestmark = pytest.mark.gpu
FILL, TAIL, EINVAL = 77.0, 8, 22
TILE = 2048
TOS = [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
PAIRS = [(8000, 32000), (16000, 32000), (22050, 32000), (44100, 32000), (48000, 32000), (96000, 32000), (44100, 16000),
         (48000, 16000)]
OTHERS = [(R.U8, 1), (R.S32, 2), (R.F32, 1), (R.F64, 2), (R.S24, 3)]      # each other encoding once, at 48000
_CACHE = {}


def _write(tmp, name, fmt, samples, rate, form="plain"):
    samples = np.asarray(samples)                      # [frames, C]
    path = str(tmp / f"{name}.wav")
    R.wav_file(path, R.sample_bytes(samples, fmt), fmt, samples.shape[1], rate, form)
    return path


def _launch(batch, out_rate, gpu, tab=None, over=None, shift=0):
    """the C entry point for a batch of ONE input rate -> (return code, buffer on the host, offsets, lengths).  tab: device
    table columns to replace; over: arguments to replace; shift: bytes put in front of the buffer (byte_off moves along)"""
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.hip import lib as L

    (rate,) = batch.by_rate
    up, down = R.ratio(rate, out_rate)
    lengths = [(i.frames * up) // down for i in batch.infos]
    offsets = [sum(lengths[:k]) for k in range(len(lengths))]
    cols = dict(byte_off=[o + shift for o in batch.byte_off], frames=[i.frames for i in batch.infos],
                fmt=[i.fmt for i in batch.infos], channels=[i.channels for i in batch.infos], off=offsets)
    cols.update(tab or {})
    raw = torch.cat([torch.full((shift,), 0xA5, dtype=torch.uint8), batch.raw]).to(gpu)
    dev = {k: torch.tensor(v, dtype=torch.int32 if k in ("fmt", "channels") else torch.int64).to(gpu) for k, v in cols.items()}
    out = torch.full((sum(lengths) + TAIL,), FILL, dtype=torch.float32, device=gpu)
    table, j_pad = (None, 0) if up == down else (audio.phase_table(up, down, gpu), audio.table_shape(up, down)[1])
    a = dict(raw=L.ptr(raw), raw_len=raw.numel(), byte_off=L.ptr(dev["byte_off"]), frames=L.ptr(dev["frames"]),
             fmt=L.ptr(dev["fmt"]), channels=L.ptr(dev["channels"]), nrec=len(batch), max_frames=max(max(cols["frames"]), 1),
             up=up, down=down, table=L.ptr(table), J=j_pad, out=L.ptr(out), out_elems=out.numel() - TAIL, off=L.ptr(dev["off"]))
    a.update(over or {})
    rc = L.lib().evt_pcm_ingest_rows(a["raw"], a["raw_len"], a["byte_off"], a["frames"], a["fmt"], a["channels"], a["nrec"],
                                     a["max_frames"], a["up"], a["down"], a["table"], a["J"], a["out"], a["out_elems"], a["off"],
                                     L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu(), offsets, lengths


def _rows(out, offsets, lengths):
    total = sum(lengths)
    assert int((out[:total] == FILL).sum()) == 0, "every element of the buffer is written"
    assert bool((out[total:] == FILL).all()), "nothing behind sum(To) is touched"
    return [out[o:o + n] for o, n in zip(offsets, lengths)]


def _same(got, want):
    """equal values, NaN where NaN"""
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _specials(fmt):
    f32 = [float("nan"), float("inf"), -float("inf"), 1e-45, -1e-40, -0.0, 3.4028234663852886e38, 1.0, -1.0]
    if fmt == R.F32:
        return f32
    # float64: values that round on the way to fp32 (to even, to a subnormal, to 0, to infinity)
    return f32 + [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 0.1, 1e-42, 1e-320, 1e300, -1e300, 3.4028235677973366e38]


def _decode_cases():
    """(name, fmt, samples [frames, C]): all six encodings at C = 1 and 2, s24 at C = 3 and 8; more than one tile"""
    cases = []
    for fmt in range(6):
        for channels in (1, 2) + ((3, 8) if fmt == R.S24 else ()):
            frames = TILE + 301 + fmt
            x = R.samples_of(fmt, frames, channels, 10 * fmt + channels)
            if fmt == R.S32:                # integers fp32 does not hold: ties to even both ways, and the largest
                x[1, 0], x[2, 0], x[3, 0], x[4, 0] = 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, -(2 ** 31) + 1
            if fmt >= R.F32:
                sp = _specials(fmt)
                x[5:5 + len(sp), 0] = sp
                x[40:40 + len(sp), -1] = sp[::-1]
            cases.append((f"{R.NAMES[fmt]}_{channels}", fmt, x))
    return cases


def test_decode_and_downmix_are_exact(gpu, tmp_path):
    """up == down == 1: torch.equal with the numpy statement (NaN where it has NaN; a mono float32 file bit for bit), all
    encodings and channel counts in one launch; PCM16 files equal read_wav_pcm16"""
    from easevoice_trainer_amd.audiokit import wav
    from easevoice_trainer_amd.train.dataset import read_wav_pcm16

    cases = _decode_cases()
    forms = ["plain", "fmt18", "ext"]
    paths = [_write(tmp_path, name, fmt, x, 32000, forms[k % 3]) for k, (name, fmt, x) in enumerate(cases)]
    batch = wav.stage(paths)
    rc, out, offsets, lengths = _launch(batch, 32000, gpu)
    assert rc == 0 and lengths == [len(x) for _n, _f, x in cases]
    for (name, fmt, x), path, got in zip(cases, paths, _rows(out, offsets, lengths)):
        want = R.mono(x, fmt)
        assert _same(got.numpy(), want), name
        if fmt == R.F32 and x.shape[1] == 1:
            assert np.array_equal(got.numpy().view(np.int32), x.astype("<f4").reshape(-1).view(np.int32)), "the value itself"
        if fmt == R.S16:
            assert torch.equal(got, torch.from_numpy(read_wav_pcm16(path, 32000))), name
    # the same bytes one byte off any alignment: the byte-wise loads
    rc, shifted, _o, _l = _launch(batch, 32000, gpu, shift=1)
    assert rc == 0 and _same(shifted.numpy(), out.numpy())


def _rate_batch(tmp, in_rate, out_rate):
    """s16 stereo recordings with To in TOS, one of 0 frames and one of 1 frame; at 48000 -> 32000 each other encoding"""
    from easevoice_trainer_amd.audiokit import wav

    key = (in_rate, out_rate)
    if key not in _CACHE:
        up, down = R.ratio(in_rate, out_rate)
        recs = [(R.S16, R.ints(R.S16, R.frames_for(to, up, down), 2, 100 + k)) for k, to in enumerate(TOS)]
        recs += [(R.S16, R.ints(R.S16, 0, 2, 0)), (R.S16, R.ints(R.S16, 1, 2, 7))]
        if key == (48000, 32000):
            recs += [(fmt, R.samples_of(fmt, R.frames_for(TILE + 1, up, down) + k, c, 200 + k)) for k, (fmt, c) in enumerate(OTHERS)]
        paths = [_write(tmp, f"r{in_rate}_{out_rate}_{k}", fmt, x, in_rate) for k, (fmt, x) in enumerate(recs)]
        monos = [R.mono(x, fmt) if len(x) else np.zeros(0, np.float32) for fmt, x in recs]
        oracle = [R.oracle(m, up, down) for m in monos]
        _CACHE[key] = (paths, monos, oracle, wav.stage(paths))
    return _CACHE[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ingest")


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_resampling_against_the_float64_oracle(gpu, tmp, in_rate, out_rate):
    up, down = R.ratio(in_rate, out_rate)
    paths, monos, oracle, batch = _rate_batch(tmp, in_rate, out_rate)
    rc, out, offsets, lengths = _launch(batch, out_rate, gpu)
    # the tile edges themselves, or where up > down skips one, the first length behind it
    assert rc == 0 and all(to <= n < to + -(-up // down) for to, n in zip(TOS, lengths)) and (down < up or lengths[:len(TOS)] == TOS)
    assert lengths[len(TOS):len(TOS) + 2] == [0, up // down]
    for k, got in enumerate(_rows(out, offsets, lengths)):
        want, bound = oracle[k]
        assert got.numel() == len(want)
        if not len(want):
            continue
        err = np.abs(got.double().numpy() - want)
        worst = int(np.argmax(err - bound))
        print(f"{in_rate} -> {out_rate} recording {k} (To = {len(want)}): max err {err.max():.3e}, at the tightest place err "
              f"{err[worst]:.3e} bound {bound[worst]:.3e}")
        assert (err <= bound).all(), (k, float(err[worst]), float(bound[worst]))


def test_row_alone_fillers_and_mixed_encodings(gpu, tmp):
    """the 48000 -> 32000 batch (six encodings, 1 .. 3 channels in one launch): every recording alone gives the bytes it
    has in the batch; the gaps between recordings may hold anything; the last recording ends the buffer"""
    from easevoice_trainer_amd.audiokit import wav

    paths, _m, _o, batch = _rate_batch(tmp, 48000, 32000)
    assert batch.byte_off[-1] + batch.infos[-1].data_bytes == batch.raw.numel() and batch.infos[-1].data_bytes % 16
    rc, out, offsets, lengths = _launch(batch, 32000, gpu)
    assert rc == 0
    rows = _rows(out, offsets, lengths)
    for filler in (0xFF, struct.pack("<f", float("nan"))):
        other = wav.stage(paths, filler=filler)
        assert other.byte_off == batch.byte_off and not torch.equal(other.raw, batch.raw)
        rc, again, _o2, _l2 = _launch(other, 32000, gpu)
        assert rc == 0 and torch.equal(again, out), filler
    for k, path in enumerate(paths):
        if lengths[k] == 0:
            continue                                   # no output (0 frames, or 1 frame at 2 / 3): nothing to launch on
        one = wav.stage([path], filler=0xFF)
        rc, alone, _o2, length = _launch(one, 32000, gpu)
        assert rc == 0 and length == [lengths[k]]
        assert torch.equal(_rows(alone, [0], length)[0], rows[k]), k


@pytest.mark.parametrize("in_rate", [48000, 44100])
def test_same_operator_as_resample_pack(gpu, tmp, in_rate):
    """a consistency check: evt_resample_pack_rows on the decoded rows gives the same bits"""
    from easevoice_trainer_amd.hip import audio

    _p, monos, _o, batch = _rate_batch(tmp, in_rate, 32000)
    rc, out, offsets, lengths = _launch(batch, 32000, gpu)
    assert rc == 0
    lens = [len(m) for m in monos]
    x = torch.zeros(len(monos), max(lens))
    for k, m in enumerate(monos):
        x[k, :lens[k]] = torch.from_numpy(m)
    pa = audio.resample_pack(x.to(gpu), lens, 1, in_rate, 32000, "float32")
    assert pa.lengths == lengths and pa.offsets == offsets
    assert torch.equal(pa.data.cpu(), out[:sum(lengths)])


def test_a_ratio_outside_lds_takes_the_direct_form(gpu, tmp):
    """2048000 -> 32000 Hz (1/64): the tile's span does not fit LDS, the frames are decoded from global memory per tap --
    same definition (the bound as tests/test_resample_pack_gpu.py uses it at this ratio), same row-alone identity, same bits
    as evt_resample_pack_rows"""
    from easevoice_trainer_amd.audiokit import wav
    from easevoice_trainer_amd.hip import audio

    recs = [(R.S16, R.ints(R.S16, 64 * 40 + 5, 2, 1)), (R.S24, R.ints(R.S24, 64 * 3, 1, 2)), (R.F64, R.floats(R.F64, 63, 2, 3))]
    paths = [_write(tmp, f"direct{k}", fmt, x, 2048000) for k, (fmt, x) in enumerate(recs)]
    batch = wav.stage(paths)
    rc, out, offsets, lengths = _launch(batch, 32000, gpu)
    assert rc == 0 and lengths == [40, 3, 0]
    rows = _rows(out, offsets, lengths)
    for k, (fmt, x) in enumerate(recs[:2]):
        m = R.mono(x, fmt)
        want, bound = R.oracle(m, 1, 64)
        assert (np.abs(rows[k].double().numpy() - want) <= bound).all(), k
        pa = audio.resample_pack(torch.from_numpy(m).to(gpu), [len(m)], 1, 2048000, 32000, "float32")
        assert torch.equal(pa.row(0).cpu(), rows[k]), k
        rc, alone, _o, length = _launch(wav.stage([paths[k]]), 32000, gpu)
        assert rc == 0 and torch.equal(_rows(alone, [0], length)[0], rows[k]), k


def test_argument_errors_and_bad_table_entries_launch_nothing(gpu, tmp):
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.hip import lib as L

    _p, _m, _o, batch = _rate_batch(tmp, 48000, 32000)
    rc, good, offsets, lengths = _launch(batch, 32000, gpu)
    assert rc == 0
    null = C.c_void_p(0)
    tp = audio.phase_table(2, 3, gpu).data_ptr()
    keep = torch.full((16,), FILL, dtype=torch.float32, device=gpu)
    bad = [dict(raw=null), dict(byte_off=null), dict(frames=null), dict(fmt=null), dict(channels=null), dict(out=null),
           dict(off=null), dict(table=null), dict(raw_len=0), dict(raw_len=-1), dict(nrec=0), dict(nrec=65536), dict(max_frames=0),
           dict(max_frames=2 ** 31), dict(out_elems=0), dict(up=0), dict(down=-3), dict(J=192), dict(J=195), dict(J=200),
           dict(table=C.c_void_p(tp + 4)), dict(out=C.c_void_p(keep.data_ptr() + 2))]
    for over in bad:
        rc, out, _o2, _l = _launch(batch, 32000, gpu, over=over)
        assert rc == EINVAL, over
        assert bool((out == FILL).all()), ("nothing was launched", over)
    assert bool((keep == FILL).all())
    # up == down == 1 needs no table
    rc, out, _o2, _l = _launch(batch, 48000, gpu, over=dict(table=null, J=0))
    assert rc == 0
    # a table entry outside the buffer, an unknown format, a channel count outside 1 .. 8: that recording is skipped, its
    # outputs are not written, the others are what they were
    n, k = len(batch), 3
    total = batch.raw.numel()
    for col, value in (("byte_off", total - 1), ("byte_off", -16), ("byte_off", total + 16), ("frames", 2 ** 31 - 1),
                       ("fmt", 6), ("fmt", -1), ("channels", 0), ("channels", 9)):
        column = {"byte_off": list(batch.byte_off), "frames": [i.frames for i in batch.infos],
                  "fmt": [i.fmt for i in batch.infos], "channels": [i.channels for i in batch.infos]}[col]
        column[k] = value
        rc, out, _o2, _l = _launch(batch, 32000, gpu, tab={col: column})
        assert rc == 0, (col, value)
        for r in range(n):
            got, want = out[offsets[r]:offsets[r] + lengths[r]], good[offsets[r]:offsets[r] + lengths[r]]
            assert bool((got == FILL).all()) if r == k else torch.equal(got, want), (col, value, r)
        assert bool((out[sum(lengths):] == FILL).all())
    # an offset table that points outside `out`: nothing is stored there
    rc, out, _o2, _l = _launch(batch, 32000, gpu, tab=dict(off=[o - 5 for o in offsets]))
    assert rc == 0 and bool((out[sum(lengths) - 5:] == FILL).all()) and torch.equal(out[:sum(lengths) - 5], good[5:sum(lengths)])


def test_binding_orders_rates_and_refuses_before_upload(gpu, tmp, tmp_path, monkeypatch):
    """hip.audio.ingest_pcm / load_audio_batch: files of three rates in one call, one launch per rate, rows in input order,
    each equal to the raw launch of its rate; a second rate from the same upload; a rate pair beyond MAX_FACTOR is an
    EvtError before anything is uploaded; empty input touches no device"""
    from easevoice_trainer_amd.audiokit import wav
    from easevoice_trainer_amd.hip import audio
    from easevoice_trainer_amd.hip import lib as L

    per_rate = {rate: _rate_batch(tmp, rate, 32000) for rate in (48000, 44100, 8000)}
    picks = [(48000, 4), (8000, 5), (44100, 3), (48000, 9), (44100, 7), (48000, 6)]
    paths = [per_rate[rate][0][k] for rate, k in picks]
    pa = audio.load_audio_batch(paths, 32000, gpu)
    assert pa.rate == 32000 and pa.gap == 0 and pa.data.dtype == torch.float32 and len(pa) == len(picks)
    assert pa.offsets == [sum(pa.lengths[:k]) for k in range(len(picks))] and pa.data.numel() == sum(pa.lengths)
    raw = {}
    for rate in per_rate:
        rc, out, offsets, lengths = _launch(per_rate[rate][3], 32000, gpu)
        raw[rate] = _rows(out, offsets, lengths)
    for b, (rate, k) in enumerate(picks):
        assert torch.equal(pa.row(b).cpu(), raw[rate][k]), (rate, k)
    # the same upload at a second rate
    batch = wav.stage(paths)
    raw_dev = audio.upload_raw(batch, gpu)
    a = audio.ingest_pcm(batch, 32000, gpu, raw_dev=raw_dev)
    b16 = audio.ingest_pcm(batch, 16000, gpu, raw_dev=raw_dev)
    assert torch.equal(a.data, pa.data) and b16.rate == 16000
    assert b16.lengths == [wav.probe(p).frames * 16000 // wav.probe(p).rate for p in paths]
    rc, out, offsets, lengths = _launch(per_rate[48000][3], 16000, gpu)
    assert rc == 0 and torch.equal(b16.row(0).cpu(), _rows(out, offsets, lengths)[4])
    # refused before upload
    odd = _write(tmp_path, "odd", R.S16, R.ints(R.S16, 100, 1, 0), 44101)
    monkeypatch.setattr(audio, "upload_raw", lambda *a, **k: pytest.fail("uploaded"))
    with pytest.raises(L.EvtError):
        audio.load_audio_batch([paths[0], odd], 32000, gpu)
    # nothing to do: no device is touched
    none = _write(tmp_path, "none", R.S16, R.ints(R.S16, 0, 2, 0), 48000)
    for empty in (audio.load_audio_batch([], 32000, gpu), audio.load_audio_batch([none, none], 32000, gpu)):
        assert empty.data.numel() == 0 and not empty.data.is_cuda and sum(empty.lengths) == 0
