#!/usr/bin/env python3
"""DistributionModel throughput: ey_hmc_run (L = 5) and ey_mh_run on Gaussian-mixture plans (mix_target)
against the same draw composed from batched torch ops on the device (what a user writes without the kernels: an einsum
for Lambda_k d, logsumexp, the closed-form gradient, the accept step with torch.where).  One JSON line per
(P, M, dtype), also appended to --out:

    python tools/bench_dist.py [--chains 4096] [--dtypes f32,f64] [--iters 100] [--shapes 2x1,2x4,...] [--out FILE]

ms per draw and draws/s x chains for each path; the torch loop runs fewer iterations (it is host-driven)."""
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
L_HMC = 5


def mixture(P, M, seed=0):
    rng = np.random.default_rng(seed)
    means = 2.0 * rng.standard_normal((M, P))
    prec = np.empty((M, P, P))
    c = np.log(0.5 + rng.random(M))
    for k in range(M):
        A = rng.standard_normal((P, P)) / np.sqrt(P)
        S = A @ A.T + np.eye(P)
        inv = np.linalg.inv(S)
        prec[k] = (inv + inv.T) / 2
        c[k] -= 0.5 * (P * np.log(2 * np.pi) + np.linalg.slogdet(S)[1])
    return c, means, prec


def timed(fn, reps):
    fn()  # warm-up (first launch, LDS attributes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def torch_target(c, mean, prec):
    def vg(th):
        d = th[:, None, :] - mean
        v = torch.einsum('kij,ckj->cki', prec, d)
        a = c - 0.5 * (d * v).sum(-1)
        val = torch.logsumexp(a, -1)
        w = torch.exp(a - val[:, None])
        return val, -(w[:, :, None] * v).sum(1)
    return vg


def torch_hmc(vg, th, t, g, step):
    p = torch.randn_like(th)
    h0 = -t + 0.5 * (p * p).sum(-1)
    q, p = th, p + 0.5 * step * g
    for k in range(1, L_HMC + 1):
        q = q + step * p
        tq, gq = vg(q)
        p = p + (step if k < L_HMC else 0.5 * step) * gq
    acc = torch.rand_like(t) < torch.exp(h0 - (-tq + 0.5 * (p * p).sum(-1)))
    return torch.where(acc[:, None], q, th), torch.where(acc, tq, t), torch.where(acc[:, None], gq, g)


def torch_mh(vg, th, t, scale):
    q = th + scale * torch.randn_like(th)
    tq = vg(q)[0]
    acc = torch.log(torch.rand_like(t)) < tq - t
    return torch.where(acc[:, None], q, th), torch.where(acc, tq, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--shapes", default="2x1,2x4,32x1,32x4,128x1,128x4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    C = args.chains
    for shape in args.shapes.split(","):
        P, M = (int(v) for v in shape.split("x"))
        for dn in args.dtypes.split(","):
            dtype = dict(f32=torch.float32, f64=torch.float64)[dn]
            c, mean, prec = mixture(P, M)
            pl = Plan.mixture(c, mean, prec, dtype, DEV)
            step, scale = 0.3 / P ** 0.25, 1.0 / P ** 0.5
            th = torch.tensor(mean[0], dtype=dtype, device=DEV).repeat(C, 1).contiguous()
            t, g = pl.log_target_grad(th)
            n = args.iters
            hmc = timed(lambda: pl.hmc_run(th, t, g, step, L_HMC, n, seed=1), 3) / n
            mh = timed(lambda: pl.mh_run(th, t, scale, n, seed=1), 3) / n
            vg = torch_target(*(torch.tensor(a, dtype=dtype, device=DEV) for a in (c, mean, prec)))
            st = [th.clone(), *vg(th)]
            nt = max(5, n // 10)

            def loop_hmc():
                for _ in range(nt):
                    st[:] = torch_hmc(vg, *st, step)

            def loop_mh():
                for _ in range(nt):
                    st[:2] = torch_mh(vg, st[0], st[1], scale)
            thmc = timed(loop_hmc, 2) / nt
            tmh = timed(loop_mh, 2) / nt
            rec = dict(P=P, M=M, dtype=dn, chains=C, kernel=pl.kernel, hmc_L=L_HMC, hmc_ms_per_draw=1e3 * hmc,
                       mh_ms_per_draw=1e3 * mh, torch_hmc_ms_per_draw=1e3 * thmc, torch_mh_ms_per_draw=1e3 * tmh,
                       hmc_draws_per_s_x_chains=C / hmc, mh_draws_per_s_x_chains=C / mh, torch_over_hmc=thmc / hmc,
                       torch_over_mh=tmh / mh)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
