#!/usr/bin/env python3
"""What a prior family costs in the generic HMC kernel: draws/s x chains of ey_hmc_run (k_hmc, ey_generic.hip) under a
Normal prior (forced to the generic kernels with EY_FORCE_GENERIC), a Laplace prior and a Student-t prior (one log1p and
one division per parameter and evaluation), on

    MLP(4-8-3),      N = 150, L = 10
    MLP(4-32-32-3),  N = 150, L = 20

in f32 and f64.  The three priors alternate within one process: after a warm-up launch of each, every repeat times one whole
launch of each with device events; the median over the repeats and their spread (min .. max) are reported.  One JSON line
per (model, dtype), also appended to --out.  With --normal-only only the forced-generic Normal case runs: the same command
on the commit before the prior families existed gives the figure the Normal case must stay within.

    python tools/bench_prior.py [--chains 4096] [--iters 50] [--repeats 7] [--dtypes f32,f64] [--normal-only] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd import _lib as L  # noqa: E402
from eeyore_amd.datasets import synthetic  # noqa: E402
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"
MODELS = {"mlp483": ([4, 8, 3], [1, 0], 10, 0.02), "mlp432323": ([4, 32, 32, 3], [1, 1, 0], 20, 0.01)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--models", default="mlp483,mlp432323")
    ap.add_argument("--normal-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prior: no GPU visible; nothing is measured without one")
    C, n = args.chains, args.iters
    xs, ys = synthetic.iris_shaped_arrays(seed=0)  # 150 rows
    for name in args.models.split(","):
        dims, acts, steps, eps = MODELS[name]
        for dn in args.dtypes.split(","):
            dtype = dict(f32=torch.float32, f64=torch.float64)[dn]
            rng = np.random.default_rng(0)
            plans = {}
            for fam in ("normal",) if args.normal_only else ("normal", "laplace", "studentt"):
                pl = Plan(dims, [1] * len(acts), acts, 1, dtype, DEV)
                pl.set_data(torch.tensor(xs, dtype=dtype, device=DEV), torch.tensor(ys, dtype=dtype, device=DEV))
                loc = torch.zeros(pl.P)
                scale = torch.tensor(1.0 + rng.random(pl.P))
                if fam == "normal":
                    pl.set_prior(loc, scale)
                elif fam == "laplace":
                    pl.set_prior_family(L.EY_PRIOR_LAPLACE, loc, scale)
                else:
                    pl.set_prior_family(L.EY_PRIOR_STUDENT_T, loc, scale, torch.tensor(2.0 + 5.0 * rng.random(pl.P)))
                th = torch.tensor(0.1 * np.random.default_rng(1).standard_normal((C, pl.P)), dtype=dtype, device=DEV)
                t, g = (v.contiguous() for v in pl.log_target_grad(th))
                plans[fam] = (pl, th, t, g)

            def launch(fam):
                pl, th, t, g = plans[fam]
                return pl.hmc_run(th, t, g, eps, steps, n, seed=1, flags=L.EY_FORCE_GENERIC)

            acc = {}
            for fam in plans:  # warm-up: first launch, LDS attributes
                acc[fam] = float(launch(fam)["accepted"].float().mean())
            torch.cuda.synchronize()
            times = {fam: [] for fam in plans}
            for _ in range(args.repeats):
                for fam in plans:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    launch(fam)
                    b.record()
                    b.synchronize()
                    times[fam].append(1e-3 * a.elapsed_time(b))
            rec = dict(model=name, dtype=dn, chains=C, iters_per_launch=n, num_steps=steps, step=eps, repeats=args.repeats,
                       rows=int(xs.shape[0]))
            for fam, ts in times.items():
                rate = sorted(C * n / s for s in ts)
                rec[f"{fam}_draws_per_s_x_chains"] = float(np.median(rate))
                rec[f"{fam}_min"], rec[f"{fam}_max"] = rate[0], rate[-1]
                rec[f"{fam}_last_acceptance"] = acc[fam]
            if not args.normal_only:
                for fam in ("laplace", "studentt"):
                    rec[f"{fam}_time_over_normal"] = rec["normal_draws_per_s_x_chains"] / rec[f"{fam}_draws_per_s_x_chains"]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
