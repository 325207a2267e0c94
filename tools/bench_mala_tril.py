#!/usr/bin/env python3
"""MALA with a fixed proposal factor: draws/s x chains of ey_mala_tril_run (k_mala_tril) with one shared
factor and with one factor per chain, on the Gaussian-mixture plans of tools/bench_dist.py, beside

  (i)  ey_mala_run with its scalar proposal scale on the same plan (what the factor and its two solves cost), and
  (ii) the same draw composed from batched torch ops plus ey_log_target_grad (what a user writes without the kernel: a
       matrix product for L z, two triangular solves for the proposal densities, the accept step with torch.where).

The paths alternate within one process: every round times one whole launch of each with device events, after a warm-up
launch of each, until every path has a window of at least --window seconds.  One JSON line per (P, M, dtype), also appended
to --out:

    python tools/bench_mala_tril.py [--chains 4096] [--dtypes f32,f64] [--iters 100] [--shapes 2x4,32x4,128x4] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dist import mixture  # noqa: E402
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"


def factors(G, P, scale, seed=1):
    rng = np.random.default_rng(seed)
    out = np.empty((G, P, P))
    for g in range(G):
        A = rng.standard_normal((P, P)) / np.sqrt(P)
        out[g] = scale * np.linalg.cholesky(A @ A.T + 0.5 * np.eye(P))
    return out


def alternate(paths, window):
    """paths: {name: (fn, draws per call)} -> {name: seconds per draw}; device events around whole calls."""
    for fn, _ in paths.values():
        fn()  # warm-up (first launch, LDS attributes)
    torch.cuda.synchronize()
    total = {k: 0.0 for k in paths}
    calls = {k: 0 for k in paths}
    while min(total.values()) < window:
        for name, (fn, _) in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            total[name] += 1e-3 * a.elapsed_time(b)
            calls[name] += 1
    return {k: total[k] / (calls[k] * paths[k][1]) for k in paths}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--shapes", default="2x4,32x4,128x4")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    C, n, step = args.chains, args.iters, args.step
    for shape in args.shapes.split(","):
        P, M = (int(v) for v in shape.split("x"))
        for dn in args.dtypes.split(","):
            dtype = dict(f32=torch.float32, f64=torch.float64)[dn]
            c, mean, prec = mixture(P, M)
            pl = Plan.mixture(c, mean, prec, dtype, DEV)
            scale = 1.0 / P ** 0.5
            th = torch.tensor(mean[0], dtype=dtype, device=DEV).repeat(C, 1).contiguous()
            t, g = (v.contiguous() for v in pl.log_target_grad(th))
            shared = torch.tensor(factors(1, P, scale)[0], dtype=dtype, device=DEV).contiguous()
            # per chain: 64 distinct factors tiled over the chains (4096 Cholesky factorisations of 128 x 128 on the host
            # would dominate the script; the kernel reads C separate [P, P] blocks either way)
            per_chain = torch.tensor(factors(64, P, scale), dtype=dtype, device=DEV).repeat((C + 63) // 64, 1, 1)[:C].contiguous()
            st = [th.clone(), t.clone(), g.clone()]

            def half_sq(d):  # |L^-1 d|^2 / 2 of every chain
                y = torch.linalg.solve_triangular(shared, d.T, upper=False)
                return 0.5 * (y * y).sum(0)

            def torch_draw():
                loc = st[0] + 0.5 * step * st[2]
                q = loc + torch.randn_like(loc) @ shared.T
                tq, gq = pl.log_target_grad(q)
                loc2 = q + 0.5 * step * gq
                log_rate = tq - st[1] + half_sq(q - loc) - half_sq(st[0] - loc2)
                acc = torch.log(torch.rand_like(tq)) < log_rate
                st[0], st[1] = torch.where(acc[:, None], q, st[0]), torch.where(acc, tq, st[1])
                st[2] = torch.where(acc[:, None], gq, st[2])

            sec = alternate({
                "mala_tril_shared": (lambda: pl.mala_tril_run(th, t, g, step, shared, n, seed=1), n),
                "mala_tril_per_chain": (lambda: pl.mala_tril_run(th, t, g, step, per_chain, n, seed=1), n),
                "mala": (lambda: pl.mala_run(th, t, g, step, n, seed=1), n),
                "torch": (torch_draw, 1),
            }, args.window)
            rec = dict(P=P, M=M, dtype=dn, chains=C, iters_per_launch=n, step=step, window_s=args.window)
            for k, v in sec.items():
                rec[f"{k}_ms_per_draw"] = 1e3 * v
                rec[f"{k}_draws_per_s_x_chains"] = C / v
            rec["tril_shared_over_mala"] = sec["mala_tril_shared"] / sec["mala"]
            rec["tril_per_chain_over_mala"] = sec["mala_tril_per_chain"] / sec["mala"]
            rec["torch_over_tril_shared"] = sec["torch"] / sec["mala_tril_shared"]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
