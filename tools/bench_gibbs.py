#!/usr/bin/env python3
"""Gibbs throughput: ey_gibbs_run (ms per draw and per sub-step) beside ey_mh_run per draw on the same plan FORCED ONTO THE
GENERIC KERNEL (a sub-step is one MH draw's evaluation without MH's full-state write, so sub-step / generic-MH draw is
the figure to read) and beside a torch-composed loop (S plan.log_target calls per draw: what a user writes without
ey_gibbs_*).  One block per node, whole nodes.  One JSON line per (model, dtype, chains):

    python tools/bench_gibbs.py [--chains 4096] [--dtypes f32,f64] [--iters 50] [--cases mlp433,...]

Whole launches are timed between device synchronisations after a warm-up launch of the same size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd import _lib as L  # noqa: E402
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"
CASES = {  # dims, activations, likelihood, rows
    "mlp433": ([4, 3, 3], [1, 0], 1, 150),
    "mlp2321": ([2, 3, 2, 1], [1, 2, 1], 0, 256),
    "mlp483": ([4, 8, 3], [1, 0], 1, 150),
    "mlp432323": ([4, 32, 32, 3], [1, 1, 0], 1, 150),
}


def node_blocks(dims):
    out, start = [], 0
    for l in range(len(dims) - 1):
        din, dout = dims[l], dims[l + 1]
        out += [[start + n * din + i for i in range(din)] + [start + din * dout + n] for n in range(dout)]
        start += (din + 1) * dout
    return out


def plan_for(name, dtype):
    dims, acts, lik, N = CASES[name]
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, dims[0]))
    y = (rng.random((N, 1)) < 0.5).astype(np.float64) if lik == 0 else np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    pl = Plan(dims, [1] * (len(dims) - 1), acts, lik, dtype, DEV)
    pl.set_data(torch.tensor(x, dtype=dtype, device=DEV), torch.tensor(y, dtype=dtype, device=DEV))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    return pl


def timed(fn, reps):
    fn()  # warm-up: first launch, LDS attributes, clocks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def start(pl, C):
    th = 0.1 * torch.randn(C, pl.P, dtype=pl.dtype, device=DEV)
    lik, prior = pl.log_target(th)
    return th, (lik + prior).contiguous()


def torch_gibbs_draw(pl, th, tv, blocks, scale):
    C = th.shape[0]
    prop = th.clone()
    for idx in blocks:
        prop[:, idx] += scale * torch.randn(C, len(idx), dtype=pl.dtype, device=DEV)
        lik, prior = pl.log_target(prop)
        tp = lik + prior
        acc = torch.log(torch.rand(C, dtype=pl.dtype, device=DEV)) < tp - tv
        th[:, idx] = torch.where(acc[:, None], prop[:, idx], th[:, idx])
        prop[:, idx] = th[:, idx]
        tv.copy_(torch.where(acc, tp, tv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="4096")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--torch-iters", type=int, default=2)
    args = ap.parse_args()
    for name in args.cases.split(","):
        blocks = node_blocks(CASES[name][0])
        blocks = [[int(i) for i in b] for b in blocks]
        S = len(blocks)
        for dt in args.dtypes.split(","):
            dtype = torch.float32 if dt == "f32" else torch.float64
            pl = plan_for(name, dtype)
            tb = pl.gibbs_table(blocks, [0.1] * S)
            for C in [int(c) for c in args.chains.split(",")]:
                K = max(2, args.iters // max(1, S // 8))  # the wide model has 67 sub-steps per draw
                th, tv = start(pl, C)
                gibbs = timed(lambda: pl.gibbs_run(th, tv, tb, K, seed=1), 3) / K
                th, tv = start(pl, C)
                Km = args.iters
                mh = timed(lambda: pl.mh_run(th, tv, 0.1, Km, seed=1, flags=L.EY_FORCE_GENERIC), 3) / Km
                th, tv = start(pl, C)
                tr = timed(lambda: torch_gibbs_draw(pl, th, tv, blocks, 0.1), args.torch_iters)
                print(json.dumps(dict(
                    case=name, P=pl.P, S=S, dtype=dt, chains=C, kernel_family_plan=pl.kernel,
                    gibbs_ms_per_draw=gibbs * 1e3, gibbs_ms_per_substep=gibbs * 1e3 / S,
                    generic_mh_ms_per_draw=mh * 1e3, torch_gibbs_ms_per_draw=tr * 1e3,
                    substep_over_generic_mh_draw=gibbs / S / mh, torch_over_gibbs=tr / gibbs,
                    gibbs_substeps_per_s_x_chains=C * S / gibbs)), flush=True)


if __name__ == "__main__":
    main()
