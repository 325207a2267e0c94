#!/usr/bin/env python3
"""RAM throughput: ey_ram_run against ey_mh_run on the same model (the cost of adaptation) and against a torch-composed
RAM loop (bmm proposal, plan.log_target, accept, batched torch.linalg.cholesky of S (I + beta w w^T) S^T: what a user
writes without ey_ram_*).  One JSON line per (model, dtype, chains):

    python tools/bench_ram.py [--chains 1,256,4096] [--dtypes f32,f64] [--iters 100] [--cases lr5,mlp433,...]

ms per iteration and draws/s x chains for each path; the torch loop runs fewer iterations (it is host-driven)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"
CASES = {  # dims, activations, likelihood, rows
    "lr5": ([4, 1], [1], 0, 200),
    "mlp433": ([4, 3, 3], [1, 0], 1, 150),
    "mlp483": ([4, 8, 3], [1, 0], 1, 150),
    "mlp6142": ([6, 14, 2], [2, 0], 1, 150),
}


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
    fn()  # warm-up (first launch, LDS attributes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def start(pl, C):
    th = 0.1 * torch.randn(C, pl.P, dtype=pl.dtype, device=DEV)
    lik, prior = pl.log_target(th)
    chol = (0.1 * torch.eye(pl.P, dtype=pl.dtype, device=DEV)).expand(C, pl.P, pl.P).contiguous()
    return th, (lik + prior).contiguous(), chol


def torch_ram_iteration(pl, th, tv, chol, n, a=0.234, g=0.7):
    C, P = th.shape
    z = torch.randn(C, P, dtype=pl.dtype, device=DEV)
    prop = th + torch.bmm(chol, z[:, :, None])[:, :, 0]
    lik, prior = pl.log_target(prop)
    tp = lik + prior
    log_rate = tp - tv
    acc = torch.log(torch.rand(C, dtype=pl.dtype, device=DEV)) < log_rate
    th.copy_(torch.where(acc[:, None], prop, th))
    tv.copy_(torch.where(acc, tp, tv))
    alpha = torch.nan_to_num(torch.exp(log_rate), nan=1.0).clamp(max=1.0)
    beta = min(1.0, P * n ** (-g)) * (alpha - a)
    w = z / z.norm(dim=1, keepdim=True)
    M = torch.eye(P, dtype=pl.dtype, device=DEV) + beta[:, None, None] * w[:, :, None] * w[:, None, :]
    chol.copy_(torch.linalg.cholesky(chol @ M @ chol.transpose(1, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1,256,4096")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--torch-iters", type=int, default=5)
    args = ap.parse_args()
    for name in args.cases.split(","):
        for dt in args.dtypes.split(","):
            dtype = torch.float32 if dt == "f32" else torch.float64
            pl = plan_for(name, dtype)
            for C in [int(c) for c in args.chains.split(",")]:
                K = args.iters
                th, tv, chol = start(pl, C)
                ram = timed(lambda: pl.ram_run(th, tv, chol, 1, K, seed=1), 3) / K
                th, tv, _ = start(pl, C)
                mh = timed(lambda: pl.mh_run(th, tv, 0.1, K, seed=1), 3) / K
                th, tv, chol = start(pl, C)
                try:
                    tr = timed(lambda: torch_ram_iteration(pl, th, tv, chol, 10), args.torch_iters)
                    terr = None
                except RuntimeError as e:  # a ROCm torch build without a batched Cholesky on the device
                    tr, terr = float("nan"), str(e).splitlines()[0][:200]
                line = dict(case=name, P=pl.P, dtype=dt, chains=C, kernel_family_mh=pl.kernel,
                            ram_ms_per_iter=ram * 1e3, mh_ms_per_iter=mh * 1e3, torch_ram_ms_per_iter=tr * 1e3,
                            ram_draws_per_s_x_chains=C / ram, mh_draws_per_s_x_chains=C / mh,
                            torch_ram_draws_per_s_x_chains=C / tr, ram_over_mh=ram / mh, torch_over_ram=tr / ram)
                if terr:
                    line["torch_error"] = terr
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
