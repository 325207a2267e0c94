"""Minimum ESS per second and per gradient: ``NUTS(metric='dense')`` against ``HMC(metric='dense')`` with the hand-set
trajectory length of examples/mvn_hmc_windowed_warmup.py (13 leapfrog steps), after the same windowed warm-up, on
N(0, Sigma) with condition number 1e4 at P = 2 / 32 / 128 in f64.

    python tools/bench_nuts.py [--chains 512] [--draws 1000] [--warmup 300] > profiles/nuts_bench.txt

Gradients: HMC makes num_steps per draw; for NUTS the count is ESTIMATED as the mean ``n_leapfrog`` of the last draw over
the chains times the number of draws (the run records no per-draw count).  Times are wall-clock around the sampling phase's
``run`` after a synchronise, one run each: read them as one sample, not a distribution."""
import argparse
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd.chains import ChainBuffer
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.models import DistributionModel
from eeyore_amd.models.targets import MultivariateNormal
from eeyore_amd.samplers import HMC, NUTS
from eeyore_amd.tuners import WindowedAdaptation
from examples.mvn_hmc_dense_metric import DEVICE, covariance

HMC_STEPS = 13


def one(kind, P, chains, draws, warmup):
    cov, _ = covariance(P=P)
    model = DistributionModel(MultivariateNormal(torch.zeros(P, dtype=torch.float64), cov), P, dtype=torch.float64,
                              device=DEVICE)
    gen = torch.Generator().manual_seed(3)
    theta0 = (0.1 * torch.randn(chains, P, generator=gen, dtype=torch.float64)).to(DEVICE)
    kw = dict(theta0=theta0, dataloader=DataLoader(EmptyXYDataset()), metric='dense', seed=1,
              tuner=WindowedAdaptation(num_steps=HMC_STEPS), chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    s = NUTS(model, **kw) if kind == 'nuts' else HMC(model, num_steps=HMC_STEPS, **kw)
    s.run(num_epochs=warmup, num_burnin_epochs=warmup)  # the warm-up alone
    torch.cuda.synchronize()
    s.counter.reset()
    t0 = time.perf_counter()
    s.run(num_epochs=draws, num_burnin_epochs=0)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    ess = s.get_chain().ess().min(1).values.sum().item()
    if kind == 'nuts':
        grads = float(s.last['n_leapfrog'].double().mean()) * draws * chains
        note = "gradients estimated from the last draw's mean n_leapfrog"
    else:
        grads, note = float(HMC_STEPS * draws * chains), "gradients = num_steps x draws x chains"
    return ess, seconds, grads, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=512)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    a = ap.parse_args()
    print(f"# N(0, Sigma), cond 1e4, f64, dense metric, {a.chains} chains, {a.warmup} warm-up draws, {a.draws} draws; "
          f"{torch.cuda.get_device_name(0)}")
    print("# P  sampler  min-ESS(sum over chains)  seconds  min-ESS/s  min-ESS/gradient  (note)")
    for P in (2, 32, 128):
        for kind in ("hmc", "nuts"):
            ess, sec, grads, note = one(kind, P, a.chains, a.draws, a.warmup)
            print(f"{P:4d} {kind:5s} {ess:12.4e} {sec:8.3f} {ess / sec:12.4e} {ess / grads:10.4e}  ({note})")


if __name__ == '__main__':
    main()
