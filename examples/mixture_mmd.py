"""Metropolis-Hastings on the reference's bivariate normal mixture, judged the way the reference's distribution examples
judge a sampler (examples/samplers/distributions/bivariate_normal*/metropolis_hastings.py there): the maximum mean discrepancy
between the chain's first n draws and n direct draws of the target under IsoSEKernel, against n.

The reference computes one such curve for one chain with a Python call per pair of points and stops at n = 100; here every
chain's curve comes out of one pass of a HIP kernel (``chain.mmd`` -> ``stats.batched.mmd_chains``), and the curve printed is
the mean over thousands of chains.  A chain stuck in one mode keeps a large MMD however good its R-hat and ESS look.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.kernels import IsoSEKernel
from eeyore_amd.models import DistributionModel, NormalMixture
from eeyore_amd.samplers import MetropolisHastings

DEVICE = 'cuda:0'


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 1100))
    burnin = epochs // 11
    dtype = torch.float32
    means = torch.tensor([[-2., -2.], [2., 2.]])
    target = NormalMixture([1., 1.], means, torch.eye(2).expand(2, 2, 2), normalized=False)
    model = DistributionModel(target, 2, dtype=dtype, device=DEVICE)

    sampler = MetropolisHastings(model, theta0=torch.zeros(num_chains, 2, dtype=dtype, device=DEVICE),
                                 dataloader=DataLoader(EmptyXYDataset()), seed=1)
    sampler.run(num_epochs=epochs, num_burnin_epochs=burnin)
    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    n = len(chain)
    print(f"Stored samples per chain: {n}; mean acceptance rate: {chain.acceptance_rate().mean().item():.3f}")

    # n direct draws of the target: a component at random, then a standard normal around its mean
    gen = torch.Generator().manual_seed(2)
    direct = (means[torch.randint(2, (n,), generator=gen)] + torch.randn(n, 2, generator=gen)).to(device=DEVICE, dtype=dtype)
    lengths = sorted({max(2, n * i // 10) for i in range(1, 11)})

    t0 = time.perf_counter()
    curve = chain.mmd(direct, kernel=IsoSEKernel(), lengths=lengths, lengths2=lengths)   # [len(lengths), C]
    torch.cuda.synchronize()
    print(f"MMD curves of {num_chains} chains at {len(lengths)} lengths: {time.perf_counter() - t0:.3f} s")
    print("     n   mean MMD over chains   worst chain")
    for m, row in zip(lengths, curve):
        print(f"{m:6d}   {row.mean().item():.4f}                 {row.max().item():.4f}")
    one_mode = (chain.get_samples().sum(-1) > 0).double().mean(0)   # share of each chain's draws near (2, 2)
    stuck = ((one_mode < 0.05) | (one_mode > 0.95))
    if bool(stuck.any()) and not bool(stuck.all()):
        print(f"chains that stayed in one mode: {int(stuck.sum())}; their final MMD {curve[-1][stuck].mean().item():.4f} "
              f"against {curve[-1][~stuck].mean().item():.4f} for the rest")


if __name__ == '__main__':
    main()
