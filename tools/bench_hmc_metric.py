#!/usr/bin/env python3
"""HMC with a fixed metric: what the metric costs per draw, and what it buys on a badly scaled target.

(i)  draws/s x chains of ey_hmc_metric_run (k_hmc_metric) with a diagonal and with a dense metric (one
     shared entry, and for dense also one factor per chain) beside ey_hmc_run with identity mass on the SAME generic plan: the
     Gaussian-mixture plans of tools/bench_dist.py at P = 2 / 32 / 128, f32 and f64.  The paths alternate within one process:
     every round times one whole launch of each with device events, after a warm-up launch of each, until every path has
     a window of at least --window seconds.  The chains restart from the same state before every launch, so every launch
     of a path does the same work.
(ii) the minimum effective sample size per second (worst coordinate, summed over the chains) of
     examples/mvn_hmc_dense_metric.py's target -- N(0, Sigma) in 32 dimensions, condition number 1e4 -- under identity mass,
     a diagonal and a dense metric, the metrics taken from the true covariance, each at a step its own geometry allows and
     the same number of leapfrog steps (13); wall time of the recorded run, which ends in a device synchronise.

One JSON line per measurement, also appended to --out:

    python tools/bench_hmc_metric.py [--chains 4096] [--dtypes f32,f64] [--iters 50] [--shapes 2x4,32x4,128x4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
from bench_dist import mixture  # noqa: E402
from bench_mala_tril import alternate, factors  # noqa: E402
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def cost_per_draw(args):
    C, n, L = args.chains, args.iters, args.num_steps
    for shape in args.shapes.split(","):
        P, M = (int(v) for v in shape.split("x"))
        for dn in args.dtypes.split(","):
            dtype = dict(f32=torch.float32, f64=torch.float64)[dn]
            c, mean, prec = mixture(P, M)
            pl = Plan.mixture(c, mean, prec, dtype, DEV)
            th0 = torch.tensor(mean[0], dtype=dtype, device=DEV).repeat(C, 1).contiguous()
            t0, g0 = (v.contiguous() for v in pl.log_target_grad(th0))
            th, t, g = th0.clone(), t0.clone(), g0.clone()
            step = args.step
            ones = torch.ones(P, dtype=dtype, device=DEV)
            shared = torch.tensor(factors(1, P, 1.0)[0], dtype=dtype, device=DEV).contiguous()
            # per chain: 64 distinct factors tiled over the chains (the kernel reads C separate [P, P] blocks either way)
            per_chain = torch.tensor(factors(64, P, 1.0), dtype=dtype, device=DEV).repeat((C + 63) // 64, 1, 1)[:C].contiguous()

            def restart():
                th.copy_(th0), t.copy_(t0), g.copy_(g0)

            def path(fn):
                def call():
                    restart()
                    fn()
                return call, n

            sec = alternate({
                "hmc": path(lambda: pl.hmc_run(th, t, g, step, L, n, seed=1)),
                "diag": path(lambda: pl.hmc_metric_run(th, t, g, step, L, ones, "diag", n, seed=1)),
                "dense_shared": path(lambda: pl.hmc_metric_run(th, t, g, step, L, shared, "dense", n, seed=1)),
                "dense_per_chain": path(lambda: pl.hmc_metric_run(th, t, g, step, L, per_chain, "dense", n, seed=1)),
            }, args.window)
            rec = dict(what="cost_per_draw", P=P, M=M, dtype=dn, chains=C, iters_per_launch=n, num_steps=L, step=step,
                       window_s=args.window, kernel=pl.kernel)
            for k, v in sec.items():
                rec[f"{k}_ms_per_draw"] = 1e3 * v
                rec[f"{k}_draws_per_s_x_chains"] = C / v
            for k in ("diag", "dense_shared", "dense_per_chain"):
                rec[f"{k}_over_hmc"] = sec[k] / sec["hmc"]
            emit(rec, args.out)


def ess_per_second(args):
    from torch.utils.data import DataLoader
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.models import DistributionModel, MultivariateNormal
    from eeyore_amd.samplers import HMC, DenseMetric, DiagMetric
    from mvn_hmc_dense_metric import P, covariance
    cov, eig = covariance()
    C, L = args.ess_chains, 13
    model = DistributionModel(MultivariateNormal(torch.zeros(P, dtype=torch.float64), cov), P, dtype=torch.float64,
                              device=DEV)
    # start in the target: a direct draw per chain
    gen = torch.Generator().manual_seed(3)
    Lf = torch.linalg.cholesky(cov)
    th0 = (torch.randn(C, P, generator=gen, dtype=torch.float64) @ Lf.T).to(DEV)
    # steps: identity and diag at 0.6 of the stability limit 2 sigma_min of their geometry (the narrowest direction of the
    # covariance; of the covariance rescaled by the marginal scales), where one direction is near the limit; dense at 0.35
    # of it, where the whitened target is a standard normal and all 32 directions are equally near
    sd = cov.diagonal().sqrt()
    corr = cov / sd[:, None] / sd[None, :]
    cases = (("identity", None, 1.2 * float(eig.min().sqrt())),
             ("diag", DiagMetric(sd), 1.2 * float(torch.linalg.eigvalsh(corr).min().sqrt())),
             ("dense", DenseMetric(Lf), 0.7))
    for name, metric, step in cases:
        for rep in range(2):  # the first run warms the kernels up and is not reported
            s = HMC(model, theta0=th0, dataloader=DataLoader(EmptyXYDataset()), step=step, num_steps=L, seed=1, metric=metric,
                    chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.run(num_epochs=args.ess_draws, num_burnin_epochs=0)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
        chain = s.get_chain()
        ess = chain.ess()
        worst = ess.min(1).values
        emit(dict(what="min_ess_per_s", target="N(0, Sigma), P = 32, condition 1e4", metric=name, step=step, num_steps=L,
                  chains=C, draws=args.ess_draws, seconds=seconds, acceptance=chain.acceptance_rate().mean().item(),
                  min_ess_median_over_chains=worst.median().item(), min_ess_per_s_summed_over_chains=worst.sum().item() / seconds,
                  draws_per_s_x_chains=C * args.ess_draws / seconds), args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--num-steps", type=int, default=4)
    ap.add_argument("--shapes", default="2x4,32x4,128x4")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--ess-chains", type=int, default=512)
    ap.add_argument("--ess-draws", type=int, default=2000)
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: cost, ess")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hmc_metric: no GPU -- nothing is measured without one")
    skip = set(args.skip.split(","))
    if "cost" not in skip:
        cost_per_draw(args)
    if "ess" not in skip:
        ess_per_second(args)


if __name__ == "__main__":
    main()
