#!/usr/bin/env python3
"""Time stats.batched.mmd_chains (ey_kernel_pair_sums: no [n, n] matrix) against the obvious torch formulation on the same
device: torch.cdist -> kernel function -> sum, which materialises [C, n, n], [C, m, m] and [C, n, m].  f64, IsoSEKernel(),
x2 one [m, p] sample shared by all chains (a direct sample of the target), the whole run (no prefixes).

    python tools/bench_mmd.py [--repeats 20] [--out profiles/mmd_bench.txt]

Per shape: clocks warmed by untimed calls of both, then `repeats` rounds alternating the two, each call between device events;
medians (and minima) are printed, with the largest difference between the two squared statistics.  A record, not a test."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd.kernels import IsoSEKernel  # noqa: E402
from eeyore_amd.stats import batched  # noqa: E402

SHAPES = [(256, 512, 512, 2), (256, 512, 512, 64), (4096, 256, 256, 2), (1, 4096, 4096, 2)]   # (C, n, m, p)


def torch_form(x, y, ker):
    """x [C, n, p], y [m, p] -> squared mmd [C] (biased)"""
    n, m = x.shape[1], y.shape[0]
    k11 = ker.of_sqdist(torch.cdist(x, x).pow(2)).sum((1, 2))
    k22 = ker.of_sqdist(torch.cdist(y[None], y[None]).pow(2)).sum((1, 2))
    k12 = ker.of_sqdist(torch.cdist(x, y[None].expand(x.shape[0], m, y.shape[1])).pow(2)).sum((1, 2))
    return k11 / (n * n) + k22 / (m * m) - 2 * k12 / (n * m)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mmd: needs the ROCm device")
    dev, ker, lines = torch.device("cuda", 0), IsoSEKernel(), []
    for C, n, m, p in SHAPES:
        g = torch.Generator(device=dev).manual_seed(C + n + p)
        x = torch.randn(C, n, p, dtype=torch.float64, device=dev, generator=g)
        y = 0.4 + 1.25 * torch.randn(m, p, dtype=torch.float64, device=dev, generator=g)
        ours = lambda: batched.mmd_chains(x, y, ker, layout="cnp", squared=True)  # noqa: E731
        theirs = lambda: torch_form(x, y, ker)  # noqa: E731
        for _ in range(5):
            ours(), theirs()
        torch.cuda.synchronize()
        t_o, t_t = [], []
        for _ in range(args.repeats):
            to, a = timed(ours)
            tt, b = timed(theirs)
            t_o.append(to)
            t_t.append(tt)
        diff = (a - b).abs().max().item()
        pairs = C * (n * n + n * m) + m * m
        line = (f"C={C} n={n} m={m} p={p} f64: mmd_chains median {statistics.median(t_o):.3f} ms (min {min(t_o):.3f}), "
                f"torch cdist form median {statistics.median(t_t):.3f} ms (min {min(t_t):.3f}), ratio torch/ours "
                f"{statistics.median(t_t) / statistics.median(t_o):.2f}, {pairs / statistics.median(t_o) * 1e-6:.1f} G pairs/s, "
                f"max |difference| {diff:.2e}")
        print(line, flush=True)
        lines.append(line)
        del x, y, a, b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/bench_mmd.py --repeats {args.repeats} on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
