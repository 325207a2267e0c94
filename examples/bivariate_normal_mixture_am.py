"""Adaptive Metropolis on the reference's bivariate normal mixture,
log(exp(-|theta - m_0|^2 / 2) + exp(-|theta - m_1|^2 / 2)) with m_0 = (-2, -2) and m_1 = (2, 2)
(examples/samplers/distributions/bivariate_normal_mixture/am.py there), first as one chain, then as thousands at once.

The reference hands the sampler ``transform=lambda h: softabs(h.to(torch.float64), 1000.).to(model.dtype)``: the running
covariance of the first draws is rank deficient, a Cholesky of it fails, and softabs lifts the null space to 1 / a -- in
f64, because f32 eigenvalues are not good enough.  Here ``transform=SoftAbs(1000.)`` says the same, and the sampler's
kernel runs the eigen-decomposition itself, in f64 inside an f32 run, every draw, for every chain: ``run`` goes through
``ey_am_softabs_run`` in blocks of iterations.  l = 0.01, b = 2, c = 2 and theta0 = 0 as there.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.models import DistributionModel, NormalMixture
from eeyore_amd.samplers import AM, SoftAbs

DEVICE = 'cuda:0'
DTYPE = torch.float32


def run(theta0, epochs, burnin, seed=1):
    means = torch.tensor([[-2., -2.], [2., 2.]])
    target = NormalMixture([1., 1.], means, torch.eye(2).expand(2, 2, 2), normalized=False)
    model = DistributionModel(target, 2, dtype=DTYPE, device=DEVICE)
    sampler = AM(model, theta0=theta0, dataloader=DataLoader(EmptyXYDataset()), l=0.01, b=2., c=2.,
                 transform=SoftAbs(1000.), seed=seed)
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=burnin)
    torch.cuda.synchronize()
    return sampler, time.perf_counter() - t0


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 11000))
    burnin = epochs // 11

    # ---- the reference's single chain (torch's generator draws z and the uniforms, in the reference's order)
    torch.manual_seed(0)
    sampler, seconds = run(torch.zeros(2, dtype=DTYPE, device=DEVICE), epochs, burnin)
    chain = sampler.get_chain()
    print(f"One chain: {seconds:.2f} s, acceptance rate {chain.acceptance_rate():.3f}, "
          f"Monte Carlo mean {[round(float(v), 3) for v in chain.mean()]} (the mixture's mean is [0, 0]), "
          f"breakdowns of the factorisation: {sampler.breakdowns}")

    # ---- many chains, each adapting its own covariance, on the in-kernel random streams
    sampler, seconds = run(torch.zeros(num_chains, 2, dtype=DTYPE, device=DEVICE), epochs, burnin)
    print(f"{num_chains} chains: {seconds:.2f} s  ->  {num_chains * epochs / seconds:.3e} draws/sec x chains")
    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    samples = chain.get_samples()
    print(f"Stored samples per chain: {len(chain)}")
    print(f"Acceptance rate (mean over chains): {chain.acceptance_rate().mean().item():.3f}")
    print(f"Pooled mean over all chains: {samples.double().mean((0, 1)).tolist()} (the mixture's mean is [0, 0])")
    in_first = (samples.sum(-1) < 0).double().mean(0)  # per chain: the fraction of its draws around m_0
    print(f"Chains that visited both modes: {int(((in_first > 0.05) & (in_first < 0.95)).sum())} of {num_chains}")
    print(f"Breakdowns of the factorisation: {int(sampler.breakdowns.sum())}")
    print(f"Adapted cov of chain 0 (the mixture's covariance is [[5, 4], [4, 5]]):\n{sampler.cov[0].cpu()}")


if __name__ == '__main__':
    main()
