#!/usr/bin/env python3
"""What the exponential-tilt target costs beside a Gaussian one: draws/s x chains of ey_mala_run (k_mala, ey_generic.hip) on a
plan of ey_plan_create_exptilt (tilt_target: one exp per coordinate and evaluation) and on a
MultivariateNormal plan of ey_plan_create_mixture of the same P (mix_target: a P x P product per evaluation), at

    P = 1, 32, 128

in f32 and f64.  The two targets alternate within one process: after a warm-up launch of each, every repeat times one whole
launch of each with device events; the median over the repeats and their spread (min .. max) are reported.  One JSON line
per (P, dtype), also appended to --out.  A record, not a gate: there is no threshold.

    python tools/bench_exptilt.py [--chains 4096] [--iters 5000] [--repeats 7] [--dtypes f32,f64] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd.plan import Plan  # noqa: E402

DEV = "cuda:0"
SIZES = {1: 0.5, 32: 0.08, 128: 0.03}  # P: MALA step


def tilt_tables(P, rng):
    """Mixed signs of s, |s| in [0.5, 2], a / s in [0.5, 4], b in [0.3, 3]."""
    s = (0.5 + 1.5 * rng.random(P)) * np.where(rng.random(P) < 0.5, -1.0, 1.0)
    return rng.standard_normal(P), (0.5 + 3.5 * rng.random(P)) * s, 0.3 + 2.7 * rng.random(P), s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--sizes", default="1,32,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_exptilt: no GPU visible; nothing is measured without one")
    C, n = args.chains, args.iters
    for P in (int(v) for v in args.sizes.split(",")):
        step = SIZES[P]
        for dn in args.dtypes.split(","):
            dtype = dict(f32=torch.float32, f64=torch.float64)[dn]
            rng = np.random.default_rng(P)
            c, a, b, s = tilt_tables(P, rng)
            A = rng.standard_normal((P, P)) / np.sqrt(P)
            prec = A @ A.T + 0.75 * np.eye(P)
            prec = (prec + prec.T) / 2
            starts = {"exptilt": np.log(a / (b * s)) / s, "normal": np.zeros(P)}
            plans = {}
            for name in ("exptilt", "normal"):
                pl = Plan.exp_tilt(c, a, b, s, dtype, DEV) if name == "exptilt" else \
                    Plan.mixture(np.zeros(1), np.zeros((1, P)), prec[None], dtype, DEV)
                z = np.random.default_rng(1).standard_normal((C, P))
                th = torch.tensor(starts[name] + 0.3 * z, dtype=dtype, device=DEV)
                t, g = (v.contiguous() for v in pl.log_target_grad(th))
                plans[name] = (pl, th, t, g)

            def launch(name):
                pl, th, t, g = plans[name]
                return pl.mala_run(th, t, g, step, n, seed=1)

            acc = {}
            for name in plans:  # warm-up: first launch, LDS attributes
                acc[name] = float(launch(name)["accepted"].float().mean())
            torch.cuda.synchronize()
            times = {name: [] for name in plans}
            for _ in range(args.repeats):
                for name in plans:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch(name)
                    e1.record()
                    e1.synchronize()
                    times[name].append(1e-3 * e0.elapsed_time(e1))
            rec = dict(P=P, dtype=dn, chains=C, iters_per_launch=n, step=step, repeats=args.repeats)
            for name, ts in times.items():
                rate = sorted(C * n / t for t in ts)
                rec[f"{name}_draws_per_s_x_chains"] = float(np.median(rate))
                rec[f"{name}_min"], rec[f"{name}_max"] = rate[0], rate[-1]
                rec[f"{name}_last_acceptance"] = acc[name]
            rec["exptilt_time_over_normal"] = rec["normal_draws_per_s_x_chains"] / rec["exptilt_draws_per_s_x_chains"]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
