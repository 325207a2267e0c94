"""HMC with its step sizes and diagonal metric found on the device, on the matrix cores: MLP(4-32-32-3) on Iris, 4096 chains.

``HMC(metric='diag', tuner=WindowedAdaptation(...), metric_kernel='fused')`` makes the burn-in Stan's diag_e warm-up (DESIGN.md
4.23): dual averaging of every chain's step inside the launches, the metric re-estimated at the end of doubling windows from
moments kept inside the kernel.  ``metric_kernel='fused'`` runs every draw of it, and of the sampling phase after it, on the
kernel of the matrix cores (``k_hmc_metric_mfma``) for the plans whose ``plan.kernel`` is 'mfma32' -- this one
is; without it the same draws run on the generic kernel, about thirty times slower per leapfrog step.  The script prints which
kernel served, the adapted steps and scales, and the acceptance.  The chains start from draws of the prior scaled down.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.chains import ChainBuffer
from eeyore_amd.constants import loss_functions
from eeyore_amd.datasets import XYDataset
from eeyore_amd.models import mlp
from eeyore_amd.samplers import HMC
from eeyore_amd.tuners import WindowedAdaptation

DEVICE = 'cuda:0'
NUM_STEPS = 10


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 200))
    warmup = max(20, epochs // 2)
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=torch.float32, device=DEVICE)
    loader = DataLoader(iris, batch_size=len(iris), shuffle=False)
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                                activations=[torch.sigmoid, torch.sigmoid, None]),
                    dtype=torch.float32, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEVICE), torch.full((P,), 3.0, device=DEVICE).sqrt())

    torch.manual_seed(1)
    tuner = WindowedAdaptation(num_steps=NUM_STEPS)
    sampler = HMC(model, theta0=0.1 * model.prior.sample((num_chains,)), dataloader=loader, metric='diag', tuner=tuner,
                  rng='philox', seed=1, metric_kernel='fused', chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    t0 = time.perf_counter()
    sampler.run(num_epochs=warmup + epochs, num_burnin_epochs=warmup)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    plan = model._plan(*next(iter(loader)))
    chain = sampler.get_chain()
    ends = ", ".join(str(h['draw']) for h in tuner.history) or "none"
    print(f"metric_kernel='fused': HMC runs on the {plan.hmc_metric_kernel(sampler._metric_flags(plan))} kernel")
    print(f"{num_chains} chains, {P} parameters, {NUM_STEPS} leapfrog steps a draw, {warmup} warm-up draws and {epochs} stored: "
          f"{seconds:.2f} s")
    print(f"windowed warm-up: the metric re-estimated after draws {ends}; steps {sampler.step.min().item():.4f} ... "
          f"{sampler.step.max().item():.4f}; scales {sampler.metric.scale.min().item():.3f} ... "
          f"{sampler.metric.scale.max().item():.3f}")
    print(f"Acceptance rate of the stored draws: {chain.acceptance_rate().mean().item():.4f}; mean log-target of the last "
          f"draw: {chain.get_target_vals()[-1].mean().item():.2f}")


if __name__ == '__main__':
    main()
