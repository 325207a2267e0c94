"""MALA on an unnormalised Gamma(shape 2, scale 1) density, sampled on the log scale, for thousands of chains at once
(examples/samplers/distributions/gamma/mala_unnormalized_target.py of the reference).

The reference samples theta = log x on the whole real line with the Jacobian in its closure,
log p(theta) = (shape - 1) theta - exp(theta) / scale + theta, with MALA at step 0.25 from theta0 = -1, and reports the
chain's acceptance rate, mean and Monte Carlo standard error.  Here the same density is ``LogGamma(2, 1, normalized=False)``,
a member of the exponential-tilt family the generic HIP kernels evaluate in closed form, and every chain
runs inside one kernel.  exp(theta) is the Gamma variable itself, whose mean is shape * scale.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.models import DistributionModel, LogGamma
from eeyore_amd.samplers import MALA

DEVICE = 'cuda:0'
SHAPE, SCALE = 2.0, 1.0
NORMALIZED = False


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 11000))
    burnin = epochs // 11
    dtype = torch.float64
    model = DistributionModel(LogGamma(SHAPE, SCALE, normalized=NORMALIZED), 1, dtype=dtype, device=DEVICE)
    sampler = MALA(model, theta0=torch.full((num_chains, 1), -1.0, dtype=dtype, device=DEVICE),
                   dataloader=DataLoader(EmptyXYDataset()), step=0.25, seed=1)
    print(f"kernel family: {model._plan().kernel}")
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=burnin)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"Time taken: {seconds:.2f} s  ->  {num_chains * epochs / seconds:.3e} draws/sec x chains")

    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    print(f"Stored samples per chain: {len(chain)}")
    print(f"Acceptance rate (mean over chains): {chain.acceptance_rate().mean().item():.3f}")
    print(f"Monte Carlo mean of theta over all chains: {chain.mean().mean().item():.4f}")
    print(f"Monte Carlo standard error of theta (median over chains): {chain.mc_se().median().item():.4f}")
    x = chain.get_samples().exp()
    print(f"Monte Carlo mean of exp(theta) over all chains: {x.mean().item():.4f} (true mean shape * scale = {SHAPE * SCALE})")


if __name__ == '__main__':
    main()
