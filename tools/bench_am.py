#!/usr/bin/env python3
"""AM throughput: ey_am_run against ey_ram_run and ey_mh_run on the same plan (what the in-wave factorisation and the
covariance rebuild cost) and against a torch-composed AM loop (plan.log_target plus a batched torch.linalg.cholesky: what
a user writes without ey_am_*).  One JSON line per (model, dtype, chains), also appended to --out:

    python tools/bench_am.py [--chains 4096] [--dtypes f32,f64] [--iters 100] [--cases lr5,mlp433,...] [--out FILE]

ms per iteration and draws/s x chains for each path; the torch loop runs fewer iterations (it is host-driven).  The AM
run starts at idx = t0, so every timed draw adapts, and l = 0.05: 95 % of the draws factorise."""
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
CASES = {  # dims, activations, likelihood, rows (the cases of tools/bench_ram.py)
    "lr5": ([4, 1], [1], 0, 200),
    "mlp433": ([4, 3, 3], [1, 0], 1, 150),
    "mlp483": ([4, 8, 3], [1, 0], 1, 150),
    "mlp6142": ([6, 14, 2], [2, 0], 1, 150),
}
L_MIX, C_ISO, T0, EPS = 0.05, 0.1, 2, 1e-4


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
    return th, (lik + prior).contiguous()


def am_state(pl, C):
    P, kw = pl.P, dict(dtype=pl.dtype, device=DEV)
    cov0 = (0.01 * torch.eye(P, **kw)).contiguous()
    return (torch.zeros(C, P, **kw), torch.zeros(C, P, P, **kw), cov0.expand(C, P, P).contiguous(),
            torch.zeros(C, dtype=torch.int32, device=DEV), cov0)


def torch_am_iteration(pl, th, tv, mean, cov_sum, cov, n, b):
    C, P = th.shape
    kw = dict(dtype=pl.dtype, device=DEV)
    z = torch.randn(C, P, **kw)
    iso = torch.rand(C, **kw) < L_MIX
    fac = torch.linalg.cholesky(cov)
    prop = th + torch.where(iso[:, None], C_ISO * z, torch.bmm(b * fac, z[:, :, None])[:, :, 0])
    lik, prior = pl.log_target(prop)
    tp = lik + prior
    acc = torch.log(torch.rand(C, **kw)) < tp - tv
    th.copy_(torch.where(acc[:, None], prop, th))
    tv.copy_(torch.where(acc, tp, tv))
    mean.copy_(((n - 1) * mean + th) / n)
    cov_sum.add_(th[:, :, None] * th[:, None, :])
    cov.copy_((cov_sum - n * mean[:, :, None] * mean[:, None, :]) / (n - 1) + EPS * torch.eye(P, **kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="4096")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    for name in args.cases.split(","):
        for dt in args.dtypes.split(","):
            dtype = torch.float32 if dt == "f32" else torch.float64
            pl = plan_for(name, dtype)
            b = 2.38 / np.sqrt(pl.P)
            for C in [int(c) for c in args.chains.split(",")]:
                K = args.iters
                th, tv = start(pl, C)
                st = am_state(pl, C)
                bd = torch.zeros(C, dtype=torch.int32, device=DEV)
                # P + 2 draws first: the empirical covariance has full rank before anything is timed
                pl.am_run(th, tv, *st, 0, pl.P + 2, l=L_MIX, b=b, c=C_ISO, eps=EPS, t0=T0, seed=1, breakdowns=bd)
                i0 = pl.P + 2
                am = timed(lambda: pl.am_run(th, tv, *st, i0, K, l=L_MIX, b=b, c=C_ISO, eps=EPS, t0=T0, seed=1, it=i0,
                                             breakdowns=bd), 3) / K
                th, tv = start(pl, C)
                chol = (0.1 * torch.eye(pl.P, dtype=dtype, device=DEV)).expand(C, pl.P, pl.P).contiguous()
                ram = timed(lambda: pl.ram_run(th, tv, chol, 1, K, seed=1), 3) / K
                th, tv = start(pl, C)
                mh = timed(lambda: pl.mh_run(th, tv, 0.1, K, seed=1), 3) / K
                th, tv = start(pl, C)
                mean, cov_sum, cov, _, _ = am_state(pl, C)
                try:
                    for n in range(1, pl.P + 3):  # as above: a full-rank covariance first
                        torch_am_iteration(pl, th, tv, mean, cov_sum, cov, max(n, 2), b)
                    tr = timed(lambda: torch_am_iteration(pl, th, tv, mean, cov_sum, cov, pl.P + 3, b), args.torch_iters)
                    terr = None
                except RuntimeError as e:  # a ROCm torch build without a batched Cholesky on the device
                    tr, terr = float("nan"), str(e).splitlines()[0][:200]
                line = dict(case=name, P=pl.P, dtype=dt, chains=C, kernel_family_mh=pl.kernel,
                            am_ms_per_iter=am * 1e3, ram_ms_per_iter=ram * 1e3, mh_ms_per_iter=mh * 1e3,
                            torch_am_ms_per_iter=tr * 1e3, am_draws_per_s_x_chains=C / am, am_over_ram=am / ram,
                            am_over_mh=am / mh, torch_over_am=tr / am, breakdowns=int(bd.sum()))
                if terr:
                    line["torch_error"] = terr
                text = json.dumps(line)
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(text + "\n")


if __name__ == "__main__":
    main()
