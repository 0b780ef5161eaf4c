"""Bindings of the audio slicer's launches (csrc/slicer.hip; include/evt.h has the definitions): windowed RMS frames, span
peaks and the rescale-and-pack to int16 for recordings that lie in one packed fp32 device buffer.  The offsets and lengths
come from the host, which packed the buffer: they are checked against it here, before a pointer reaches a kernel, and
uploaded as one int64 table.  Inference only."""
import torch

from . import lib as L

MAX_WIN = 8192          # kRmsMaxWin of csrc/slicer.hip
MAX_SPANS = 65535       # spans of one launch (a grid's second dimension); longer tables go out in pieces


def _check_buffer(what, x):
    if (not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous()
            or x.numel() < 1):
        raise L.EvtError(f"{what}: a contiguous 1-D float32 buffer on the GPU expected")
    if torch.is_grad_enabled() and x.requires_grad:
        raise L.EvtError(f"{what} is inference only: run it under torch.no_grad()")


def _ints(what, name, seq, count=None):
    seq = [int(v) for v in (seq.tolist() if hasattr(seq, "tolist") else seq)]
    if count is not None and len(seq) != count:
        raise L.EvtError(f"{what}: {count} entries of {name} expected, got {len(seq)}")
    return seq


def frame_count(n, win, hop):
    """frames of get_rms for a recording of n samples: the signal padded by win // 2 on both sides, one frame per hop"""
    return (int(n) + 2 * (win // 2) - win) // hop + 1


def rms_frames_rows(x, offs, lens, win, hop):
    """x: packed fp32 recordings on the GPU, recording r = x[offs[r] : offs[r] + lens[r]] (host ints, 1 <= len < 2^31) ->
    (rms, frame_off): rms fp32 [frame_off[-1]] on the GPU, recording r's frames at rms[frame_off[r] : frame_off[r + 1]],
    each bit for bit the reference's get_rms(frame_length=win, hop_length=hop) of that recording alone (NumPy's pairwise
    float32 summation order; evt_rms_frames_rows).  One launch, no synchronisation."""
    _check_buffer("rms_frames_rows", x)
    offs = _ints("rms_frames_rows", "offs", offs)
    lens = _ints("rms_frames_rows", "lens", lens, len(offs))
    win, hop = int(win), int(hop)
    if not offs:
        raise L.EvtError("rms_frames_rows: no recordings")
    if not 1 <= win <= MAX_WIN or hop < 1:
        raise L.EvtError(f"rms_frames_rows: win = {win} (1 .. {MAX_WIN}) and hop = {hop} (>= 1) are not served")
    frame_off = [0]
    for o, n in zip(offs, lens):
        if not 1 <= n < 2 ** 31 or o < 0 or o + n > x.numel():
            raise L.EvtError(f"rms_frames_rows: recording [{o}, {o} + {n}) does not lie in a buffer of {x.numel()} samples "
                             "with 1 <= len < 2^31")
        frame_off.append(frame_off[-1] + frame_count(n, win, hop))
    nrec, total = len(offs), frame_off[-1]
    table = torch.tensor(offs + lens + frame_off, dtype=torch.int64).to(x.device)
    rms = torch.empty(total, dtype=torch.float32, device=x.device)
    L.check(L.lib().evt_rms_frames_rows(
        x.data_ptr(), x.numel(), table.data_ptr(), table[nrec:].data_ptr(), nrec, win, hop, rms.data_ptr(),
        table[2 * nrec:].data_ptr(), total, L.stream_ptr()), "evt_rms_frames_rows")
    return rms, frame_off


class Spans:
    """a checked table of spans of a packed buffer, on the host and (one int64 tensor [3, nspan]: source offset, length,
    destination offset) on the buffer's device: span s is x[src[s] : src[s] + n[s]] and goes to out[dst[s] : dst[s] + n[s]]
    (dst: the prefix sum of n unless given)"""

    def __init__(self, x, src, n, dst=None):
        _check_buffer("Spans", x)
        self.src = _ints("Spans", "src", src)
        self.n = _ints("Spans", "n", n, len(self.src))
        if dst is None:
            dst, pos = [], 0
            for v in self.n:
                dst.append(pos)
                pos += max(v, 0)
        self.dst = _ints("Spans", "dst", dst, len(self.src))
        if not self.src:
            raise L.EvtError("Spans: an empty table")
        for o, v, d in zip(self.src, self.n, self.dst):
            if v < 0 or o < 0 or o + v > x.numel() or d < 0:
                raise L.EvtError(f"Spans: span [{o}, {o} + {v}) -> {d} does not lie in a buffer of {x.numel()} samples")
        self.x_len = x.numel()
        self.max_n = max(self.n)
        self.out_len = max(d + v for d, v in zip(self.dst, self.n))
        self.table = torch.tensor([self.src, self.n, self.dst], dtype=torch.int64).to(x.device)

    def __len__(self):
        return len(self.src)


def _check_spans(what, x, spans):
    _check_buffer(what, x)
    if not isinstance(spans, Spans) or spans.x_len != x.numel() or spans.table.device != x.device:
        raise L.EvtError(f"{what}: a Spans table built for this buffer expected")


def span_peaks(x, spans):
    """-> peak fp32 [len(spans)] on the GPU: max |x| over every span, NaN where a span holds one (np.abs(x).max()), 0 for an
    empty span (evt_span_peak_rows).  One launch for up to 65535 spans."""
    _check_spans("span_peaks", x, spans)
    peak = torch.empty(len(spans), dtype=torch.float32, device=x.device)
    fn = L.lib().evt_span_peak_rows
    for s0 in range(0, len(spans), MAX_SPANS):
        ns = min(MAX_SPANS, len(spans) - s0)
        L.check(fn(x.data_ptr(), x.numel(), spans.table[0, s0:].data_ptr(), spans.table[1, s0:].data_ptr(), ns, spans.max_n,
                   peak[s0:].data_ptr(), L.stream_ptr()), "evt_span_peak_rows")
    return peak


def slice_pack(x, spans, peak, c1, c2):
    """-> int16 [spans.out_len] on the GPU: every span rescaled by its peak as AudioService.slicer rescales a chunk
    (audio.py:172-178) in numpy's float32 steps -- v / peak where peak > 1, then (v / peak) * c1 + c2 * v, times 32767,
    truncated -- and written at its destination offset (evt_slice_pack_rows).  A span whose peak is 0 (all zeros: the
    reference casts 0 / 0, which numpy leaves undefined) is written as zeros.  Elements of the output that no span covers
    are zeros.  One launch for up to 65535 spans."""
    _check_spans("slice_pack", x, spans)
    if (not torch.is_tensor(peak) or peak.dtype != torch.float32 or peak.device != x.device or peak.dim() != 1
            or peak.numel() != len(spans) or not peak.is_contiguous()):
        raise L.EvtError(f"slice_pack: peak must be a contiguous float32 [{len(spans)}] tensor on {x.device}")
    dense = spans.out_len == sum(spans.n)      # every element is written by the launch: no memset in front of it
    out = (torch.empty if dense else torch.zeros)(spans.out_len, dtype=torch.int16, device=x.device)
    if spans.out_len == 0:
        return out
    fn = L.lib().evt_slice_pack_rows
    for s0 in range(0, len(spans), MAX_SPANS):
        ns = min(MAX_SPANS, len(spans) - s0)
        L.check(fn(x.data_ptr(), x.numel(), spans.table[0, s0:].data_ptr(), spans.table[1, s0:].data_ptr(),
                   spans.table[2, s0:].data_ptr(), peak[s0:].data_ptr(), float(c1), float(c2), ns, spans.max_n,
                   out.data_ptr(), out.numel(), L.stream_ptr()), "evt_slice_pack_rows")
    return out
