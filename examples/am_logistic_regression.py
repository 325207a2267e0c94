"""Adaptive Metropolis (Haario et al.) over logistic-regression coefficients, many chains at once on one MI355X.

The reference's AM workflow (its examples/samplers/logistic_regression/banknotes/am.py: four standardised features,
LogisticRegression without bias, N(0, 1) prior) on synthetic banknote-shaped data, with the textbook proposal: scale
b = 2.38 / sqrt(P) on the factor of the empirical covariance plus a ridge, ``transform=Ridge(eps)``, which the kernel
applies itself.  ``theta0`` of shape [C, P] runs C chains, each adapting its own covariance, in one launch per block of
iterations.  EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import numpy as np
import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.constants import loss_functions
from eeyore_amd.datasets import XYDataset
from eeyore_amd.models import logistic_regression
from eeyore_amd.samplers import AM, Ridge

DEVICE = 'cuda:0'
DTYPE = torch.float32


def banknote_shaped(n=1372, seed=0):
    """Two classes of four features each, standardised as the reference standardises the banknotes."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.45).astype(np.float64)
    x = rng.standard_normal((n, 4)) * np.array([2.0, 5.0, 4.0, 2.0]) + np.outer(y, [-4.0, -3.0, 1.5, 0.0])
    x = (x - x.mean(0)) / x.std(0)
    return XYDataset(torch.tensor(x, dtype=DTYPE, device=DEVICE), torch.tensor(y[:, None], dtype=DTYPE, device=DEVICE))


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 64))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 400))
    data = banknote_shaped()
    dataloader = DataLoader(data, batch_size=len(data))
    model = logistic_regression.LogisticRegression(
        loss=loss_functions['binary_classification'],
        hparams=logistic_regression.Hyperparameters(input_size=4, bias=False), dtype=DTYPE, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, dtype=DTYPE, device=DEVICE), torch.ones(P, dtype=DTYPE, device=DEVICE))

    theta0 = model.prior.sample((num_chains,))
    eps = 1e-5
    sampler = AM(model, theta0=theta0, dataloader=dataloader, l=0.05, b=2.38 / np.sqrt(P), c=0.1, t0=20,
                 transform=Ridge(eps), seed=1)
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=0)  # every state is recorded: the covariance is built from all
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"Time taken: {seconds:.2f} s  ->  {num_chains * epochs / seconds:.3e} draws/sec x chains")

    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    rate = chain.acceptance_rate()
    print(f"Stored samples per chain: {len(chain)}")
    print(f"Acceptance rate: mean {rate.mean().item():.3f}, chains {rate.min().item():.3f} .. {rate.max().item():.3f}")
    print(f"Breakdowns of the factorisation: {int(sampler.breakdowns.sum())}")
    second_half = chain.get_samples()[epochs // 2:].double()  # pooled over the chains, after the transient
    pooled = torch.cov(second_half.reshape(-1, P).T)
    adapted = sampler.cov.double().mean(0)
    gap = (torch.linalg.norm(adapted - pooled) / torch.linalg.norm(pooled)).item()
    print(f"Adapted cov (mean over chains) against the pooled sample covariance of the second half: "
          f"relative Frobenius distance {gap:.3f}")
    print(f"Adapted cov of chain 0:\n{sampler.cov[0].cpu()}")


if __name__ == '__main__':
    main()
