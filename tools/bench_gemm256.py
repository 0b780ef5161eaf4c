"""Timing of csrc/gemm256.hip at the s1 layer shapes, next to the 128 x 128 kernels of conv_deep.hip (the composition the
layers run with EVT_NO_GEMM256 set; the switch is read per call).  HIP events over `--iters` launches each."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32768, 1536, 512), (32768, 512, 512), (32768, 2048, 512), (32768, 512, 2048), (16384, 1536, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.linear import LinearBank, gemm_fwd

    dev = torch.device("cuda:0")
    L.lib()
    for M, N, K in SHAPES:
        w = torch.nn.Parameter(torch.randn(N, K, device=dev) * K ** -0.5)
        b = torch.nn.Parameter(torch.randn(N, device=dev) * 0.1)
        x = torch.randn(M, K, device=dev).bfloat16()
        row = {}
        for name, off in (("gemm256", False), ("composed", True)):
            if off:
                os.environ["EVT_NO_GEMM256"] = "1"
            else:
                os.environ.pop("EVT_NO_GEMM256", None)
            bank = LinearBank([("t", w, b)], torch.bfloat16, dev)      # a fresh bank: a slot remembers which kernel covers it
            bank.prepare()
            slot = w._evt_slot
            fused = bool(slot.fused(M, False))
            for _ in range(3):
                gemm_fwd(slot, x)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                gemm_fwd(slot, x)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.iters
            row[name] = dict(fused=fused, us=round(us, 1), tflops=round(2.0 * M * N * K / us / 1e6, 1))
        os.environ.pop("EVT_NO_GEMM256", None)
        print(f"{M}x{N}x{K}", json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
