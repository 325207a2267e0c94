#!/usr/bin/env python3
"""What a regression plan costs beside a classification plan of the same shape: draws/s x chains of HMC (ey_hmc_step, one
call per draw, whatever family serves the plan) on

    MLP(8-64-1), f32, N = 512, 4096 chains, L = 10

under the Gaussian likelihood with an identity output (EY_LIK_GAUSS_SUM: the layerwise family's separate launches, DESIGN.md
4.19) against BCE-sum with a sigmoid output (the same family with its fused last-layer kernel k_tail).  The two plans
alternate within one process: after a warm-up of each, every repeat times --iters draws of each with device events; the
median over the repeats and their spread (min .. max) are reported.  One JSON line, also appended to --out.

    python tools/bench_regression.py [--chains 4096] [--iters 20] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd import _lib as L  # noqa: E402
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"
DIMS, N, STEPS, EPS = [8, 64, 1], 512, 10, 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regression: no GPU visible; nothing is measured without one")
    C, n = args.chains, args.iters
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, DIMS[0]))
    f = np.tanh(x @ rng.standard_normal(DIMS[0]))
    ys = {"gauss": (f + 0.3 * rng.standard_normal(N))[:, None], "bce": (rng.random(N) < 1 / (1 + np.exp(-2 * f)))[:, None]}
    plans = {}
    for name, code, act_out in (("gauss", L.EY_LIK_GAUSS_SUM, 0), ("bce", L.EY_LIK_BCE_SUM, 1)):
        pl = Plan(DIMS, [1, 1], [2, act_out], code, torch.float32, DEV)
        pl.set_data(torch.tensor(x, dtype=torch.float32, device=DEV),
                    torch.tensor(ys[name].astype(np.float64), dtype=torch.float32, device=DEV))
        pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
        if name == "gauss":
            pl.set_lik_scale(0.3)
        th = torch.tensor(0.1 * np.random.default_rng(1).standard_normal((C, pl.P)), dtype=torch.float32, device=DEV)
        t, g = (v.contiguous() for v in pl.log_target_grad(th))
        plans[name] = (pl, th, t, g)

    def draws(name, it0):
        pl, th, t, g = plans[name]
        for it in range(n):
            out = pl.hmc_step(th, t, g, EPS, STEPS, seed=1, it=it0 + it)
        return out

    acc = {name: float(draws(name, 0)["accepted"].float().mean()) for name in plans}  # warm-up
    torch.cuda.synchronize()
    times = {name: [] for name in plans}
    for r in range(args.repeats):
        for name in plans:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            draws(name, (r + 1) * n)
            b.record()
            b.synchronize()
            times[name].append(1e-3 * a.elapsed_time(b))
    rec = dict(model="mlp_8_64_1", dtype="f32", rows=N, chains=C, draws_per_repeat=n, num_steps=STEPS, step=EPS,
               repeats=args.repeats, kernels={name: plans[name][0].kernel for name in plans})
    for name, ts in times.items():
        rate = sorted(C * n / s for s in ts)
        rec[f"{name}_draws_per_s_x_chains"] = float(np.median(rate))
        rec[f"{name}_min"], rec[f"{name}_max"] = rate[0], rate[-1]
        rec[f"{name}_last_acceptance"] = acc[name]
    rec["gauss_time_over_bce"] = rec["bce_draws_per_s_x_chains"] / rec["gauss_draws_per_s_x_chains"]
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
