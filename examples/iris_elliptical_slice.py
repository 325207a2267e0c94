"""Elliptical slice sampling of MLP(4-32-32-3) on Iris: 4096 chains over 1315 weights with nothing tuned.

The model of the README under its elementwise Normal prior.  ``EllipticalSlice`` has no step, no metric and no warm-up: a draw
takes a point nu of the prior, and shrinks an angle bracket on the ellipse through the state and nu until a point lies above
the slice height -- value-only evaluations of the log-likelihood, one wave per chain, so chains that need different numbers of
evaluations run side by side (``ey_eslice_run``).  The script prints the mean evaluations per draw, R-hat
and the effective sample sizes.  The chains start from draws of the prior.  EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS
shrink the run.
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
from eeyore_amd.distributed import ChainStats
from eeyore_amd.models import mlp
from eeyore_amd.samplers import EllipticalSlice
from eeyore_amd.stats import batched

DEVICE = 'cuda:0'


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 4096))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 300))
    burnin = epochs // 3
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=torch.float32, device=DEVICE)
    loader = DataLoader(iris, batch_size=len(iris), shuffle=False)
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                                activations=[torch.sigmoid, torch.sigmoid, None]),
                    dtype=torch.float32, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEVICE), torch.full((P,), 3.0, device=DEVICE).sqrt())

    torch.manual_seed(1)
    sampler = EllipticalSlice(model, theta0=model.prior.sample((num_chains,)), dataloader=loader, seed=1,
                              chain=ChainBuffer(keys=['sample', 'target_val', 'accepted', 'n_evals']))
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=burnin)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    chain = sampler.get_chain()
    evals = chain.bufs['n_evals'][:len(chain)].double()
    print(f"{num_chains} chains, {P} parameters, {epochs} draws ({burnin} of them burn-in): {seconds:.2f} s  ->  "
          f"{num_chains * epochs / seconds:.3e} draws/sec x chains")
    print(f"evaluations per stored draw: mean {evals.mean().item():.2f}, largest {int(evals.max().item())}; "
          f"share of draws that moved: {chain.acceptance_rate().mean().item():.4f}")
    stats = ChainStats(num_chains, P, DEVICE)
    for i in range(len(chain)):
        stats.update(chain.get_samples()[i].contiguous(), chain.get_accepted()[i].contiguous())
    print(f"max R-hat over parameters: {stats.summary()['rhat'].max().item():.3f}")
    ess = batched.ess(chain.get_samples()[:, :min(num_chains, 256)].contiguous())   # [chains, P], of the first 256 chains
    print(f"ESS per chain of {len(chain)} stored draws, median over chains: worst parameter "
          f"{ess.min(1).values.median().item():.1f}, median parameter {ess.median(1).values.median().item():.1f}")


if __name__ == '__main__':
    main()
