"""NUTS warmed up on the device: the target of ``mvn_hmc_dense_metric.py`` -- a 32-dimensional multivariate normal whose
covariance has condition number 1e4, for hundreds of chains at once -- sampled without a trajectory length anywhere.

``NUTS(metric='dense', tuner=WindowedAdaptation(...))`` makes the burn-in the windowed warm-up of
``mvn_hmc_windowed_warmup.py`` -- every chain's step adapts by dual averaging on the draw's mean accept statistic, the dense
metric is re-estimated at the end of doubling windows from moments kept inside the kernel -- and every draw, warm-up or not,
ends its own trajectory: the tree doubles until it turns back on itself (``ey_nuts_warmup`` / ``ey_nuts_run``).  One wave
is one chain, so chains whose trees differ in depth run side by side.  The script prints the adapted steps, the tree depths
of the sampling phase, divergences, and the effective sample sizes.  The chains start close together on purpose.
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
from eeyore_amd.samplers import NUTS
from eeyore_amd.tuners import WindowedAdaptation
from examples.mvn_hmc_dense_metric import DEVICE, P, covariance, report


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 512))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 2000))
    warmup = max(150, epochs // 2)
    dtype = torch.float64
    cov, eig = covariance()
    model = DistributionModel(MultivariateNormal(torch.zeros(P, dtype=torch.float64), cov), P, dtype=dtype, device=DEVICE)
    gen = torch.Generator().manual_seed(3)
    theta0 = (0.1 * torch.randn(num_chains, P, generator=gen, dtype=dtype)).to(DEVICE)
    print(f"target: N(0, Sigma) in {P} dimensions, standard deviations {eig.min().sqrt().item():.2f} ... "
          f"{eig.max().sqrt().item():.1f}; {num_chains} chains")

    tuner = WindowedAdaptation(num_steps=1)  # (the tuner's num_steps is not used by NUTS)
    sampler = NUTS(model, theta0=theta0, dataloader=DataLoader(EmptyXYDataset()), metric='dense', tuner=tuner, seed=1,
                   chain=ChainBuffer(keys=['sample', 'target_val', 'accepted', 'depth', 'divergent']))
    t0 = time.perf_counter()
    sampler.run(num_epochs=warmup + epochs, num_burnin_epochs=warmup)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    est = sampler.metric.scale_tril.double() @ sampler.metric.scale_tril.double().T
    err = (torch.linalg.eigvalsh(est).log10() - torch.linalg.eigvalsh(cov.to(est)).log10()).abs().max().item()
    ends = ", ".join(str(h['draw']) for h in tuner.history)
    print(f"windowed warm-up: {warmup} draws, the metric re-estimated after draws {ends} (largest error of an eigenvalue: a "
          f"factor {10 ** err:.2f}); steps {sampler.step.min().item():.3f} ... {sampler.step.max().item():.3f}")
    depth = sampler.get_chain().bufs['depth'][:len(sampler.get_chain())]
    div = sampler.get_chain().bufs['divergent'][:len(sampler.get_chain())]
    hist = torch.bincount(depth.flatten().long(), minlength=11).tolist()
    print(f"tree depths of the stored draws (0 ... 10): {hist}; divergent draws: {int(div.sum())}")
    report("NUTS, dense metric, warmed up in the same run", sampler, seconds)


if __name__ == '__main__':
    main()
