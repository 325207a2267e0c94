#!/usr/bin/env python3
"""AM with the softabs transform: what the in-wave eigen-decomposition costs and what it saves.  Per (model, dtype, chains)
three paths on the same plan, draws/s x chains each:

  fused     ey_am_softabs_run: softabs inside the kernel, blocks of iterations per launch
  callable  what ``AM`` does with the same ``SoftAbs`` object when it cannot fuse: ey_am_step without a transform, then the
            object on every chain's covariance in a Python loop (``AM._retransform``), one draw per launch; timed on
            --callable-chains chains (its cost per chain does not depend on how many there are)
  ridge     ey_am_run with cov + eps I: the kernel without an eigen-decomposition

One JSON line per case, also appended to --out:

    python tools/bench_am_softabs.py [--chains 4096] [--dtypes f32,f64] [--iters 20] [--cases lr2,mlp433,...] [--out FILE]

The cases are P = 2, 27, 65 and the widest logistic regression whose softabs instantiation fits the dtype.  Every run
starts at idx = t0 = 2 after P + 2 draws, so every timed draw adapts and transforms, and l = 0.05: 95 % of the draws
factorise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd.plan import Plan  # noqa: E402
from eeyore_amd.samplers import SoftAbs  # noqa: E402
from eeyore_amd.stats import batched  # noqa: E402

DEV = "cuda:0"
CASES = {  # dims, activations, likelihood, rows; "largest" is found with ey_am_softabs_fits
    "lr2": ([1, 1], [1], 0, 200),
    "mlp433": ([4, 3, 3], [1, 0], 1, 150),
    "lr65": ([64, 1], [1], 0, 16),
    "largest": None,
}
L_MIX, C_ISO, T0, EPS, A = 0.05, 0.1, 2, 1e-4, 1000.0


def plan_of(dims, acts, lik, N, dtype):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, dims[0])) / max(1.0, np.sqrt(dims[0] / 16))
    y = (rng.random((N, 1)) < 0.5).astype(np.float64) if lik == 0 else np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    pl = Plan(dims, [1] * (len(dims) - 1), acts, lik, dtype, DEV)
    pl.set_data(torch.tensor(x, dtype=dtype, device=DEV), torch.tensor(y, dtype=dtype, device=DEV))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    return pl


def plan_for(name, dtype):
    if name != "largest":
        return plan_of(*CASES[name], dtype)
    for d in range(127, 0, -1):  # the widest logistic regression the softabs instantiation has room for
        pl = plan_of([d, 1], [1], 0, 16, dtype)
        if pl.am_softabs_fits():
            return pl
    raise SystemExit("no logistic regression fits")


def timed(fn, reps):
    fn()  # warm-up (first launch, LDS attributes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def state(pl, C, transform):
    P, kw = pl.P, dict(dtype=pl.dtype, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(0)
    th = (0.1 * torch.randn(C, P, generator=g, dtype=torch.float64)).to(**kw)
    lik, prior = pl.log_target(th)
    cov0 = transform(0.01 * torch.eye(P, **kw)).contiguous()
    return dict(args=[th, (lik + prior).contiguous(), torch.zeros(C, P, **kw), torch.zeros(C, P, P, **kw),
                      cov0.expand(C, P, P).contiguous().clone(), torch.zeros(C, dtype=torch.int32, device=DEV), cov0],
                bd=torch.zeros(C, dtype=torch.int32, device=DEV))


def callable_draw(pl, st, tr, idx, b):
    """AM.draw on the callable path: the kernel without a transform, then the object chain by chain."""
    pl.am_step(*st["args"], idx, l=L_MIX, b=b, c=C_ISO, eps=0.0, t0=T0, seed=1, it=idx, breakdowns=st["bd"])
    cov, nacc = st["args"][4], st["args"][5]
    for c in (nacc > 0).nonzero().flatten().tolist():
        lo = torch.tril(cov[c])
        cov[c] = tr(lo + torch.tril(cov[c], -1).mT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="4096")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--callable-iters", type=int, default=1)
    ap.add_argument("--callable-chains", type=int, default=256)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    tr = SoftAbs(A)
    for name in args.cases.split(","):
        for dt in args.dtypes.split(","):
            dtype = torch.float32 if dt == "f32" else torch.float64
            pl = plan_for(name, dtype)
            b, K, i0 = 2.38 / np.sqrt(pl.P), args.iters, pl.P + 2
            par = dict(l=L_MIX, b=b, c=C_ISO, t0=T0, seed=1)
            for C in [int(c) for c in args.chains.split(",")]:
                st = state(pl, C, tr)
                pl.am_run(*st["args"], 0, i0, softabs_a=A, breakdowns=st["bd"], **par)
                fused = timed(lambda: pl.am_run(*st["args"], i0, K, softabs_a=A, it=i0, breakdowns=st["bd"], **par), 2) / K
                # the sweeps of the next draw's transform: softabs of the raw covariance the state holds
                n = i0 + K
                mean, cs = st["args"][2].double(), st["args"][3].double()
                raw = (torch.tril(cs) - n * torch.tril(mean[:, :, None] * mean[:, None, :])) / (n - 1)
                sweeps = torch.zeros(C, dtype=torch.int32, device=DEV)
                batched.softabs(raw.to(dtype).contiguous(), A, sweeps=sweeps)
                fused_bd = int(st["bd"].sum())
                Cc = min(C, args.callable_chains)
                st = state(pl, Cc, tr)
                pl.am_run(*st["args"], 0, i0, softabs_a=A, breakdowns=st["bd"], **par)  # the same start as the fused path
                call = timed(lambda: callable_draw(pl, st, tr, i0, b), args.callable_iters)
                st = state(pl, C, lambda m: m + EPS * torch.eye(pl.P, dtype=dtype, device=DEV))
                pl.am_run(*st["args"], 0, i0, eps=EPS, breakdowns=st["bd"], **par)
                ridge = timed(lambda: pl.am_run(*st["args"], i0, K, eps=EPS, it=i0, breakdowns=st["bd"], **par), 2) / K
                line = dict(case=name, P=pl.P, dtype=dt, chains=C, fused_ms_per_iter=fused * 1e3,
                            callable_chains=Cc, callable_ms_per_iter=call * 1e3, ridge_ms_per_iter=ridge * 1e3,
                            fused_draws_per_s_x_chains=C / fused, callable_draws_per_s_x_chains=Cc / call,
                            ridge_draws_per_s_x_chains=C / ridge, callable_over_fused=(call / Cc) / (fused / C),
                            fused_over_ridge=fused / ridge, sweeps_mean=float(sweeps.float().mean()),
                            sweeps_max=int(sweeps.max()), breakdowns_fused=fused_bd, breakdowns_ridge=int(st["bd"].sum()))
                text = json.dumps(line)
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(text + "\n")


if __name__ == "__main__":
    main()
