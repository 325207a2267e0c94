"""HMC with a dense metric on a badly scaled target: a 32-dimensional multivariate normal whose covariance has condition
number 1e4 (eigenvalues 1e-2 ... 1e2 in a random basis), for hundreds of chains at once.

With identity mass HMC must take its step from the narrowest direction (standard deviation 0.1) and its trajectory length
from the widest (10): at a step the narrow direction allows, a few leapfrog steps hardly move the wide ones.  The script

  1. runs a short warm-up with identity mass,
  2. estimates the covariance from the warm-up draws of all chains (``DenseMetric.from_samples``: Stan's regularised
     estimate, its Cholesky factor taken on the device), and
  3. runs again under that metric, one ``ey_hmc_metric_run`` launch per block of draws, from where the warm-up ended,

and prints both runs' acceptance and effective sample sizes (``chain.ess()``, per chain and coordinate).  In the whitened
coordinates the target is close to a standard normal, so the second run takes steps of order one.

The chains start close together (0.1 z around the mode) on purpose.  A fixed trajectory length leaves any direction whose
period divides it almost unmoved, so a warm-up can fail to mix one direction; started under-dispersed, such a direction
comes out of the estimate too narrow, which only costs efficiency.  Started over-dispersed it comes out too wide, and a
metric that overstates a variance fourfold makes the leapfrog step of order one unstable: every proposal is rejected.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.chains import ChainBuffer
from eeyore_amd.datasets import EmptyXYDataset
from eeyore_amd.models import DistributionModel
from eeyore_amd.models.targets import MultivariateNormal
from eeyore_amd.samplers import HMC, DenseMetric

DEVICE = 'cuda:0'
P, CONDITION = 32, 1e4


def covariance(P=P, condition=CONDITION, seed=0):
    """A covariance with eigenvalues log-spaced over ``condition`` around 1, in a random orthogonal basis."""
    gen = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(P, P, generator=gen, dtype=torch.float64))
    half = 0.5 * torch.log10(torch.tensor(condition, dtype=torch.float64))
    eig = torch.logspace(-half, half, P, dtype=torch.float64)
    cov = (q * eig) @ q.T
    return (cov + cov.T) / 2, eig


def run(model, theta0, step, num_steps, epochs, burnin, metric=None, seed=1):
    sampler = HMC(model, theta0=theta0, dataloader=DataLoader(EmptyXYDataset()), step=step, num_steps=num_steps, seed=seed,
                  metric=metric, chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=burnin)
    torch.cuda.synchronize()
    return sampler, time.perf_counter() - t0


def report(name, sampler, seconds):
    chain = sampler.get_chain()
    ess = chain.ess()  # [C, P]
    n = len(chain)
    print(f"{name}: {n} stored draws per chain in {seconds:.2f} s")
    print(f"  acceptance rate (mean over chains): {chain.acceptance_rate().mean().item():.3f}")
    print(f"  ESS per chain, median over chains: worst coordinate {ess.min(1).values.median().item():.1f}, "
          f"median coordinate {ess.median(1).values.median().item():.1f} (of {n} draws)")
    print(f"  minimum ESS per second, summed over chains: {ess.min(1).values.sum().item() / seconds:.3e}")
    return ess


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 512))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 2000))
    warmup = max(40, epochs // 4)
    dtype = torch.float64
    cov, eig = covariance()
    model = DistributionModel(MultivariateNormal(torch.zeros(P, dtype=torch.float64), cov), P, dtype=dtype, device=DEVICE)
    gen = torch.Generator().manual_seed(3)
    theta0 = (0.1 * torch.randn(num_chains, P, generator=gen, dtype=dtype)).to(DEVICE)
    print(f"target: N(0, Sigma) in {P} dimensions, standard deviations {eig.min().sqrt().item():.2f} ... "
          f"{eig.max().sqrt().item():.1f}; {num_chains} chains")

    # 1. identity mass: the step is bounded by the narrowest direction
    num_steps = 13
    plain, seconds = run(model, theta0, 0.12, num_steps, warmup + epochs, warmup)
    report("identity mass, step 0.12", plain, seconds)

    # 2. the metric from a short identity-mass warm-up of all chains, pooled
    warm, _ = run(model, theta0, 0.12, num_steps, 2 * warmup, warmup, seed=2)
    metric = DenseMetric.from_samples(warm.get_chain())
    est = metric.scale_tril @ metric.scale_tril.T
    err = (torch.linalg.eigvalsh(est).log10() - torch.linalg.eigvalsh(cov.to(est)).log10()).abs().max().item()
    print(f"metric: Cholesky factor of the regularised covariance of {len(warm.get_chain())} x {num_chains} warm-up draws "
          f"(largest error of an eigenvalue: a factor {10 ** err:.2f})")

    # 3. the same number of leapfrog steps under the metric, from where the warm-up ended
    dense, seconds = run(model, warm._theta.clone(), 0.7, num_steps, warmup + epochs, warmup, metric=metric)
    report("dense metric, step 0.7", dense, seconds)


if __name__ == '__main__':
    main()
