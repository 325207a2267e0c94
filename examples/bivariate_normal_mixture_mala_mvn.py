"""MALA with a MultivariateNormalKernel proposal on the reference's bivariate normal mixture,
log(exp(-|theta - m_0|^2 / 2) + exp(-|theta - m_1|^2 / 2)) with m_0 = (-2, -2) and m_1 = (2, 2)
(examples/samplers/distributions/bivariate_normal_mixture/mala.py there), for thousands of chains at once.

The reference runs MALA with step 2.5 and its default proposal N(theta + step/2 grad, step I) and reports the chain's
acceptance rate, mean, Monte Carlo standard error and multivariate ESS.  Its MALA also takes ``kernel=``: with a
``MultivariateNormalKernel(loc, scale_tril = L)`` the proposal is theta + step/2 grad + L z, a dense fixed covariance L L^T
around the Langevin mean (the step enters the mean only).  This script does that with every chain inside one HIP kernel
(``ey_mala_tril_run``) and adds the chains' MMD against direct draws of the mixture.  EEYORE_EXAMPLE_SCALE_TRIL (default
``1.5,0,0.5,1.3``: a dense factor) gives another lower-triangular factor, row by row; EEYORE_EXAMPLE_STEP another step.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.kernels import IsoSEKernel, MultivariateNormalKernel
from eeyore_amd.models import DistributionModel, NormalMixture
from eeyore_amd.samplers import MALA
from eeyore_amd.stats import batched

DEVICE = 'cuda:0'


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 11000))
    burnin = epochs // 11
    dtype = torch.float32
    means = torch.tensor([[-2., -2.], [2., 2.]])
    target = NormalMixture([1., 1.], means, torch.eye(2).expand(2, 2, 2), normalized=False)
    model = DistributionModel(target, 2, dtype=dtype, device=DEVICE)
    entries = [float(v) for v in os.environ.get('EEYORE_EXAMPLE_SCALE_TRIL', '1.5,0,0.5,1.3').split(',')]
    scale_tril = torch.tensor(entries, dtype=dtype).view(2, 2)

    kernel = MultivariateNormalKernel(torch.zeros(2, dtype=dtype), scale_tril)
    step = float(os.environ.get('EEYORE_EXAMPLE_STEP', 2.5))
    sampler = MALA(model, theta0=torch.zeros(num_chains, 2, dtype=dtype, device=DEVICE),
                   dataloader=DataLoader(EmptyXYDataset()), step=step, kernel=kernel, seed=1)
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=burnin)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"Time taken: {seconds:.2f} s  ->  {num_chains * epochs / seconds:.3e} draws/sec x chains")

    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    n = len(chain)
    print(f"Stored samples per chain: {n}")
    print(f"Acceptance rate (mean over chains): {chain.acceptance_rate().mean().item():.3f}")
    print(f"Monte Carlo mean over all chains: {chain.mean().mean(0).tolist()} (the mixture's mean is [0, 0])")
    print(f"Monte Carlo standard error (median over chains): {chain.mc_se().median(0).values.tolist()}")
    print(f"Multivariate ESS (median over chains): {batched.multi_ess_device(chain.get_samples()).median().item():.1f}")

    # n direct draws of the target: a component at random, then a standard normal around its mean
    gen = torch.Generator().manual_seed(2)
    direct = (means[torch.randint(2, (n,), generator=gen)] + torch.randn(n, 2, generator=gen)).to(device=DEVICE, dtype=dtype)
    lengths = sorted({max(2, n * i // 10) for i in range(1, 11)})
    curve = chain.mmd(direct, kernel=IsoSEKernel(), lengths=lengths, lengths2=lengths)   # [len(lengths), C]
    print("     n   mean MMD over chains   worst chain")
    for m, row in zip(lengths, curve):
        print(f"{m:6d}   {row.mean().item():.4f}                 {row.max().item():.4f}")


if __name__ == '__main__':
    main()
