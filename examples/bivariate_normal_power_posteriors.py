"""Power posteriors on a bivariate normal (examples/samplers/distributions/bivariate_normal/power_posteriors.py of the
reference): a ladder of tempered copies of the density, MALA within each, state exchanges between them -- for R ladders at
once, with the between-chain move and whole runs on the device.

EEYORE_EXAMPLE_CHAINS (the number of ladders) / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.models import DistributionModel, MultivariateNormal
from eeyore_amd.samplers import PowerPosteriorSampler

DEVICE = 'cuda:0'
NUM_POWER_POSTERIORS = 10


def main():
    ladders = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 256))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 11000))
    dtype = torch.float64
    mean, cov = torch.tensor([1., -1.], dtype=dtype), torch.tensor([[1., 0.5], [0.5, 2.]], dtype=dtype)
    model = DistributionModel(MultivariateNormal(mean, cov), 2, dtype=dtype, device=DEVICE)
    print(f"kernel family: {model._plan().kernel}")
    per_chain = [['MALA', {'step': 0.8}] for _ in range(NUM_POWER_POSTERIORS)]
    sampler = PowerPosteriorSampler(model, DataLoader(EmptyXYDataset()), per_chain,
                                    theta0=torch.zeros(ladders, 2, dtype=dtype, device=DEVICE), between_step=10,
                                    keys=['sample', 'target_val', 'accepted'], between='device', seed=1)
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=epochs // 11)
    torch.cuda.synchronize()
    print(f"Time taken: {time.perf_counter() - t0:.2f} s for {ladders} ladders of {NUM_POWER_POSTERIORS} temperatures")
    chain = sampler.get_chain()  # the chain at temperature one
    samples = chain.get_samples()
    print(f"Acceptance rate at temperature one: {chain.get_accepted().double().mean().item():.3f}")
    flat = samples.reshape(-1, 2)
    print(f"Monte Carlo mean: {flat.mean(0).tolist()} (true mean {mean.tolist()})")
    print(f"Monte Carlo covariance: {torch.cov(flat.T).tolist()} (true covariance {cov.tolist()})")


if __name__ == '__main__':
    main()
