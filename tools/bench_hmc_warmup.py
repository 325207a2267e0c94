#!/usr/bin/env python3
"""The windowed warm-up of HMC under a metric: what adapting inside the kernel costs per draw, and what a whole warm-up
takes against the draw-by-draw way.

(i)  draws/s x chains, on the Gaussian-mixture plans of tools/bench_dist.py at P = 2 / 32 / 128, f32 and f64, of
     ey_hmc_metric_run, and of ey_hmc_metric_warmup with nothing attached, with dual averaging, with dual averaging and
     diagonal moments, and with dual averaging and dense moments (the metric of the moments' form, one shared entry).  The
     paths alternate within one process: every round times one whole launch of each with device events, after a warm-up
     launch of each, until every path has a window of at least --window seconds.  The chains, the steps and the dual-averaging
     state restart from the same values before every launch, so every launch of a path does the same work.
(ii) seconds for a 300-draw warm-up of examples/mvn_hmc_dense_metric.py's target (N(0, Sigma), P = 32, condition 1e4, f64,
     dense metric from the identity) through HMC(tuner=WindowedAdaptation), against the same adaptation without the two
     entry points: PerChainDATuner adapting draw by draw (one launch and one host read-back per draw), the draws of a window
     recorded and DenseMetric.from_samples taken at the same window ends.  Wall time ending in a device synchronise; the
     first run of each way warms the kernels up and is not reported.

One JSON line per measurement, also appended to --out:

    python tools/bench_hmc_warmup.py [--chains 4096] [--dtypes f32,f64] [--iters 50] [--shapes 2x4,32x4,128x4] [--out FILE]
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
from bench_mala_tril import alternate  # noqa: E402
from eeyore_amd.plan import Plan  # noqa: E402
from eeyore_amd.tuners import PerChainDATuner, WindowedAdaptation  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def cost_per_draw(args):
    C, n, L = args.chains, args.iters, args.num_steps
    sched = WindowedAdaptation(num_steps=L)
    for shape in args.shapes.split(","):
        P, M = (int(v) for v in shape.split("x"))
        for dn in args.dtypes.split(","):
            dtype = dict(f32=torch.float32, f64=F64)[dn]
            c, mean, prec = mixture(P, M)
            pl = Plan.mixture(c, mean, prec, dtype, DEV)
            th0 = torch.tensor(mean[0], dtype=dtype, device=DEV).repeat(C, 1).contiguous()
            t0, g0 = (v.contiguous() for v in pl.log_target_grad(th0))
            th, t, g = th0.clone(), t0.clone(), g0.clone()
            step0 = torch.full((C,), args.step, dtype=dtype, device=DEV)
            step, state0 = step0.clone(), sched.restart(step0)
            state, table = state0.clone(), sched.table(1, n, DEV)
            metric = dict(diag=torch.ones(P, dtype=dtype, device=DEV), dense=torch.eye(P, dtype=dtype, device=DEV))
            mom = dict(diag=(torch.zeros(C, P, dtype=F64, device=DEV), torch.zeros(C, P, dtype=F64, device=DEV)),
                       dense=(torch.zeros(C, P, dtype=F64, device=DEV), torch.zeros(C, P, P, dtype=F64, device=DEV)))

            def path(fn):
                def call():
                    th.copy_(th0), t.copy_(t0), g.copy_(g0), step.copy_(step0), state.copy_(state0)
                    fn()
                return call, n

            def warm(form, da, moments):
                kw = dict(da_state=state, da_table=table, d=0.8) if da else {}
                if moments:  # (the accumulators run on: an update costs the same whatever they hold)
                    kw.update(mean=mom[form][0], M2=mom[form][1], count=0)
                return lambda: pl.hmc_metric_warmup(th, t, g, 0.0, L, metric[form], form, n, step_vec=step, seed=1, **kw)

            paths = {}
            for form in ("diag", "dense"):
                paths[f"{form}_run"] = path(lambda form=form: pl.hmc_metric_run(th, t, g, 0.0, L, metric[form], form, n,
                                                                                step_vec=step, seed=1))
                paths[f"{form}_warmup_plain"] = path(warm(form, False, False))
                paths[f"{form}_warmup_da"] = path(warm(form, True, False))
                paths[f"{form}_warmup_da_moments"] = path(warm(form, True, True))
            sec = alternate(paths, args.window)
            rec = dict(what="cost_per_draw", P=P, M=M, dtype=dn, chains=C, iters_per_launch=n, num_steps=L, step=args.step,
                       window_s=args.window, kernel=pl.kernel)
            for k, v in sec.items():
                rec[f"{k}_draws_per_s_x_chains"] = C / v
            for form in ("diag", "dense"):
                for k in ("warmup_plain", "warmup_da", "warmup_da_moments"):
                    rec[f"{form}_{k}_over_run"] = sec[f"{form}_{k}"] / sec[f"{form}_run"]
            emit(rec, args.out)
            del mom, pl
            torch.cuda.empty_cache()


def end_to_end(args):
    from torch.utils.data import DataLoader
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.models import DistributionModel, MultivariateNormal
    from eeyore_amd.samplers import HMC, DenseMetric
    from mvn_hmc_dense_metric import P, covariance
    cov, _ = covariance()
    C, L, n = args.e2e_chains, 13, args.e2e_draws
    model = DistributionModel(MultivariateNormal(torch.zeros(P, dtype=F64), cov), P, dtype=F64, device=DEV)
    gen = torch.Generator().manual_seed(3)
    th0 = (0.1 * torch.randn(C, P, generator=gen, dtype=F64)).to(DEV)
    loader = DataLoader(EmptyXYDataset())

    def whitened_condition(tril):
        Li = torch.linalg.inv(tril.double().cpu())
        return float(torch.linalg.cond(Li @ cov @ Li.T))

    def windowed():
        s = HMC(model, theta0=th0, dataloader=loader, seed=1, metric='dense', tuner=WindowedAdaptation(num_steps=L),
                chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
        s.run(num_epochs=n, num_burnin_epochs=n)
        return s._metric, s.step

    def draw_by_draw():
        sched = WindowedAdaptation(num_steps=L)
        metric, theta = DenseMetric.identity(P, dtype=F64, device=DEV), th0
        for start, end, adapts in sched.phases(n):
            s = HMC(model, theta0=theta, dataloader=loader, seed=1, metric=metric, num_steps=L,
                    chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
            s._iter = start
            s.tuner = PerChainDATuner(s.init_step_per_chain(theta), num_steps=L, d=0.8)
            s.step = s.tuner.step
            s.counter.set_epoch_info(end - start, end - start)
            x, y = next(iter(loader))
            for _ in range(end - start):
                s.draw(x, y, savestate=adapts)
                s.counter.increment_idx()
            if adapts:
                metric = DenseMetric.from_samples(s.get_chain())
            theta = s._theta
        return metric.scale_tril, s.step

    for name, fn in (("windowed", windowed), ("draw_by_draw", draw_by_draw)):
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tril, step = fn()
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
        emit(dict(what="warm_up_seconds", way=name, target="N(0, Sigma), P = 32, condition 1e4", chains=C, draws=n, num_steps=L,
                  seconds=seconds, whitened_condition=whitened_condition(tril), step_min=float(step.min()),
                  step_max=float(step.max())), args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--num-steps", type=int, default=4)
    ap.add_argument("--shapes", default="2x4,32x4,128x4")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--e2e-chains", type=int, default=4096)
    ap.add_argument("--e2e-draws", type=int, default=300)
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: cost, e2e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hmc_warmup: no GPU -- nothing is measured without one")
    skip = set(args.skip.split(","))
    if "cost" not in skip:
        cost_per_draw(args)
    if "e2e" not in skip:
        end_to_end(args)


if __name__ == "__main__":
    main()
