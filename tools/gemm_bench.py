#!/usr/bin/env python3
"""Timing of the verified-GEMM kernels (profiles/r04_gemmtest.md).

Per size: warm-up launches, then >= 20 iterations each timed with its own
event pair; mean and best are reported. Operands are generator data
(gemm_fill), not zeros. One JSON line per measurement.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from k3samd import ops  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sum(ms) / len(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096, 8192])
    ap.add_argument("--gold-size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    for s in args.sizes:
        a = torch.empty((s, s), dtype=torch.bfloat16, device=dev)
        bt = torch.empty((s, s), dtype=torch.bfloat16, device=dev)
        ops.gemm_fill(a, 0, 1, s, s)
        ops.gemm_fill(bt, 1, 1, s, s)
        c = torch.empty((s, s), dtype=torch.float32, device=dev)
        mean, best = timed(lambda: ops.gemm_bf16_nt(a, bt, out=c),
                           args.warmup, args.iters)
        flops = 2.0 * s ** 3
        print(json.dumps({"kernel": "gemm_bf16_nt", "size": s,
                          "mean_ms": round(mean, 4), "best_ms": round(best, 4),
                          "mean_tflops": round(flops / mean / 1e9, 1),
                          "best_tflops": round(flops / best / 1e9, 1)}))
        gold = c.clone()
        report = ops.mem_report_new(dev)
        mean, best = timed(lambda: ops.buf_compare(c, gold, report),
                           args.warmup, args.iters)
        nbytes = 2.0 * c.numel() * 4
        print(json.dumps({"kernel": "buf_compare", "size": s,
                          "mean_ms": round(mean, 4), "best_ms": round(best, 4),
                          "mean_gbps": round(nbytes / mean / 1e6, 1),
                          "best_gbps": round(nbytes / best / 1e6, 1),
                          "clean": ops.mem_report_read(report).clean}))
        if s == args.gold_size:
            mean, best = timed(lambda: ops.gemm_ref_int(a, bt, out=gold), 1, 5)
            print(json.dumps({"kernel": "gemm_ref_int", "size": s,
                              "mean_ms": round(mean, 3),
                              "best_ms": round(best, 3)}))


if __name__ == "__main__":
    main()
