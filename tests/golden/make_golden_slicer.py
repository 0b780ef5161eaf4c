"""Golden outputs of the REFERENCE's audio slicer (src/audiokit/slicer/slicer.py) and of the per-chunk arithmetic of its
service (src/service/audio.py:172-178), produced by importing Slicer read-only (oracle/refshim.py) and running it over the
closed-form recordings of tests/slicer_inputs.py.

Run in the build container only:   python tests/golden/make_golden_slicer.py
Writes tests/golden/slicer.json: per case the derived parameters, every frame's RMS as a uint32 bit pattern, the chunk
labels and lengths, each chunk's peak bits and the sha256 of the int16 bytes the service writes for it.  Data only.

The service's expression is applied here as the service applies it -- the same numpy statements on the chunk the Slicer
returned, in place -- since the service itself cannot run without ffmpeg and its models."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402

refshim.install()
import slicer_inputs as I  # noqa: E402

NORMALIZE_MAX, ALPHA_MIX = 0.9, 0.25       # the service's defaults


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def record(Slicer, x, params, chunks=True):
    s = Slicer(**params)
    out = {"params": params, "n": int(x.shape[0]),
           "derived": {"hop": s.hop_size, "win": s.win_size, "min_length": s.min_length, "min_interval": s.min_interval,
                       "max_sil_kept": s.max_sil_kept, "threshold": s.threshold},
           "rms": bits(Slicer.get_rms(y=x, frame_length=s.win_size, hop_length=s.hop_size).squeeze(0))}
    if not chunks:
        return out
    got = s.slice(x.copy())
    out["chunks"] = []
    if len(got) == 1 and isinstance(got[0], np.ndarray):     # at most min_length samples: handed back unsliced
        out["sliced"] = False
        return out
    out["sliced"] = True
    for chunk, start, end in got:
        nor_max = np.abs(chunk).max()
        peak = bits(nor_max)[0]
        if nor_max > 1:
            chunk /= nor_max
        chunk = (chunk / nor_max * (NORMALIZE_MAX * ALPHA_MIX)) + (1 - ALPHA_MIX) * chunk
        pcm = (chunk * 32767).astype(np.int16)
        out["chunks"].append({"start": int(start), "end": int(end), "n": int(pcm.shape[0]), "peak": peak,
                              "sha256": hashlib.sha256(pcm.astype("<i2").tobytes()).hexdigest()})
    return out


def main():
    from src.audiokit.slicer.slicer import Slicer

    assert np.__version__.split(".")[0] >= "2", "the goldens record NumPy 2's float32 comparison"
    out = {"numpy": np.__version__, "normalize_max": NORMALIZE_MAX, "alpha_mix": ALPHA_MIX,
           "A": record(Slicer, I.case_a(), I.PARAMS_A), "B": record(Slicer, I.case_b(), I.PARAMS_B),
           "C": record(Slicer, I.case_c(), I.PARAMS_C, chunks=False),
           "edges": [record(Slicer, x, I.PARAMS_A) for x in I.edges()]}
    with open(os.path.join(HERE, "slicer.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    for k in ("A", "B"):
        print(k, len(out[k]["rms"]), "frames", [(c["start"], c["end"], c["n"]) for c in out[k]["chunks"]])


if __name__ == "__main__":
    main()
