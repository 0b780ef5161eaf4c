"""Golden semantic codes of the REFERENCE's extract_latent (src/easevoice/module/models.py:1015-1018: ssl_proj + the
quantizer's forward, quantize.py:70-94, core_vq.py:172-228) on the planted inputs of tests/semantic_refs.py, produced by
importing ResidualVectorQuantizer read-only (oracle/refshim.py).

Run in the build container only:   python tests/golden/make_golden_semantic.py
Writes tests/golden/semantic_rows.pt: per case (generator, D, K) the codes of every row, packed, as int16, and the sha256 of
the inputs they belong to (tests/semantic_refs.py::checksum) -- the inputs themselves are regenerated from their seeds.
Data only.  The quantizer runs in eval mode on an initialised codebook, a row at a time in fp32, as the reference's `token`
step runs it (normalize.py:181-211); only the planted and close-pair inputs are recorded: their margins leave one answer."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402

refshim.install()
import semantic_refs as R  # noqa: E402

CASES = [(name, D, K) for name in ("planted", "close") for D, K in R.SHAPES]


def reference_codes(ResidualVectorQuantizer, inp):
    D, K = inp["embed"].size(1), inp["embed"].size(0)
    proj = torch.nn.Conv1d(D, D, 2, stride=2)
    quantizer = ResidualVectorQuantizer(dimension=D, n_q=1, bins=K)
    with torch.no_grad():
        proj.weight.copy_(inp["w"])
        proj.bias.copy_(inp["bias"])
        cb = quantizer.vq.layers[0]._codebook
        cb.embed.copy_(inp["embed"])
        cb.inited.fill_(1.0)
    quantizer.eval()
    out = []
    with torch.no_grad():
        for b, t in enumerate(inp["frames"]):
            if t < 2:
                continue
            _q, codes, _loss, _list = quantizer(proj(inp["x"][b, :t].t().unsqueeze(0)))
            out.append(codes.transpose(0, 1)[0, 0])
    return torch.cat(out)


def main():
    from src.easevoice.module.quantize import ResidualVectorQuantizer

    out = {}
    for name, D, K in CASES:
        inp = R.GENERATORS[name](D, K)
        codes = reference_codes(ResidualVectorQuantizer, inp)
        assert int(codes.max()) < 2 ** 15
        out[f"{name}_{D}_{K}"] = {"codes": codes.to(torch.int16), "sha256": R.checksum(inp)}
        print(name, D, K, codes.numel(), "codes")
    torch.save(out, os.path.join(HERE, "semantic_rows.pt"))


if __name__ == "__main__":
    main()
