"""The No-U-Turn sampler on MLP(4-32-32-3) on Iris: 1315 weights, no trajectory length, step and metric adapted on the device.

The model of the README under its elementwise Normal prior.  ``NUTS(tree='device', metric='diag', tuner=WindowedAdaptation(...))``:
the burn-in is the windowed warm-up of ``mvn_nuts_windowed_warmup.py`` -- every chain's step adapts by dual averaging on the
draw's mean accept statistic, the diagonal metric is re-estimated at the end of doubling windows from moments kept inside the
kernel -- and every draw ends its own trajectory.  The tree of a chain -- 12 + 2 max_depth vectors of 1315 weights -- does not
fit LDS beside the evaluation, so ``tree='device'`` keeps it in a workspace in device memory; the evaluation
itself stays in LDS, one wave per chain.  The script prints the adapted steps, the tree depths of the stored draws, the
divergent draws and the acceptance.  The chains start from draws of the prior scaled down.  EEYORE_EXAMPLE_CHAINS /
EEYORE_EXAMPLE_EPOCHS shrink the run.

``--tree fused`` runs the same sampler with every leapfrog step on the matrix cores (``NUTS(tree='fused')``):
the same draw and the same workspace, for the plans whose ``plan.kernel`` is 'mfma32' -- this one is.  The default is
``--tree device``.
"""
import argparse
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
from eeyore_amd.models import mlp
from eeyore_amd.samplers import NUTS
from eeyore_amd.tuners import WindowedAdaptation

DEVICE = 'cuda:0'
MAX_DEPTH = 7


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument('--tree', choices=['device', 'fused'], default='device',
                    help="where a leaf is evaluated: the generic kernel (device) or the matrix cores (fused)")
    args = ap.parse_args()
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 1024))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 200))
    warmup = max(20, epochs // 2)
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=torch.float32, device=DEVICE)
    loader = DataLoader(iris, batch_size=len(iris), shuffle=False)
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                                activations=[torch.sigmoid, torch.sigmoid, None]),
                    dtype=torch.float32, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEVICE), torch.full((P,), 3.0, device=DEVICE).sqrt())

    torch.manual_seed(1)
    tuner = WindowedAdaptation(num_steps=1)  # (the tuner's num_steps is not used by NUTS)
    sampler = NUTS(model, theta0=0.1 * model.prior.sample((num_chains,)), dataloader=loader, tree=args.tree, metric='diag',
                   max_depth=MAX_DEPTH, tuner=tuner, seed=1,
                   chain=ChainBuffer(keys=['sample', 'target_val', 'accepted', 'depth', 'divergent']))
    t0 = time.perf_counter()
    sampler.run(num_epochs=warmup + epochs, num_burnin_epochs=warmup)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    plan = model._plan(*next(iter(loader)))
    chain = sampler.get_chain()
    depth = chain.bufs['depth'][:len(chain)]
    div = chain.bufs['divergent'][:len(chain)]
    ends = ", ".join(str(h['draw']) for h in tuner.history) or "none"
    print(f"tree='{args.tree}': NUTS runs on the {plan.nuts_kernel(sampler._flags(plan))} kernel")
    print(f"{num_chains} chains, {P} parameters, {warmup} warm-up draws and {epochs} stored: {seconds:.2f} s; the tree's "
          f"workspace holds {plan.nuts_tree_bytes(num_chains, MAX_DEPTH) / 2 ** 20:.1f} MiB")
    print(f"windowed warm-up: the metric re-estimated after draws {ends}; steps {sampler.step.min().item():.4f} ... "
          f"{sampler.step.max().item():.4f}; scales {sampler.metric.scale.min().item():.3f} ... "
          f"{sampler.metric.scale.max().item():.3f}")
    hist = torch.bincount(depth.flatten().long(), minlength=MAX_DEPTH + 1).tolist()
    print(f"tree depths of the stored draws (0 ... {MAX_DEPTH}): {hist}; divergent draws: {int(div.sum())}")
    print(f"Acceptance rate (share of draws that moved): {chain.acceptance_rate().mean().item():.4f}; mean accept statistic "
          f"of the last draw: {sampler.last['accept_stat'].mean().item():.3f}")


if __name__ == '__main__':
    main()
