"""HMC on the reference's bivariate normal mixture, log(exp(-|theta - m_0|^2 / 2) + exp(-|theta - m_1|^2 / 2)) with
m_0 = (-2, -2) and m_1 = (2, 2) (examples/samplers/distributions/bivariate_normal_mixture/hmc.py there), for thousands of
chains at once.

The reference's ``DistributionModel`` takes a Python closure; here the density is a ``NormalMixture`` target object, whose
value and gradient a HIP kernel evaluates.  EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.distributed import ChainStats
from eeyore_amd.models import DistributionModel, NormalMixture
from eeyore_amd.samplers import HMC

DEVICE = 'cuda:0'
NUM_STEPS, STEP = 5, 0.5


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 11000))
    dtype = torch.float32
    means = torch.tensor([[-2., -2.], [2., 2.]])
    target = NormalMixture([1., 1.], means, torch.eye(2).expand(2, 2, 2), normalized=False)
    model = DistributionModel(target, 2, dtype=dtype, device=DEVICE)
    loader = DataLoader(EmptyXYDataset())
    print(f"kernel family: {model._plan().kernel}")

    sampler = HMC(model, theta0=torch.zeros(num_chains, 2, dtype=dtype, device=DEVICE), dataloader=loader, step=STEP,
                  num_steps=NUM_STEPS, seed=1)
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=epochs // 11)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"Time taken: {seconds:.2f} s  ->  {num_chains * epochs / seconds:.3e} draws/sec x chains")

    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    print(f"Stored samples per chain: {len(chain)}")
    print(f"Mean acceptance rate: {chain.acceptance_rate().mean().item():.3f}")
    stats = ChainStats(num_chains, 2, DEVICE)
    for i in range(len(chain)):
        stats.update(chain.get_samples()[i].contiguous(), chain.get_accepted()[i].contiguous())
    print(f"max R-hat over parameters: {stats.summary()['rhat'].max().item():.3f}")
    samples = chain.get_samples()
    print(f"Monte Carlo mean over all chains: {samples.mean((0, 1)).tolist()} (the mixture's mean is [0, 0])")
    print(f"share of draws near the mode at (2, 2): {(samples.sum(-1) > 0).double().mean().item():.3f}")


if __name__ == '__main__':
    main()
