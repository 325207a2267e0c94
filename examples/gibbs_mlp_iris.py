"""Node-blocked Metropolis within Gibbs over the weights of MLP(4-3-3) on iris-shaped data, many chains at once on one
MI355X.

The reference's Gibbs sampler visits the nodes of an MLP one at a time: the incoming weights and the bias of a node are
one parameter block with its own Normal random-walk proposal and its own accept/reject decision.  Here the five
parameters of every hidden node are cut into sub-blocks (``node_subblock_size``), the output nodes stay whole, and all
sub-steps of a draw run inside one kernel; ``theta0`` of shape [C, P] runs C chains in one launch per block of draws.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.constants import loss_functions
from eeyore_amd.datasets import synthetic
from eeyore_amd.models import mlp
from eeyore_amd.samplers import Gibbs

DEVICE = 'cuda:0'
DTYPE = torch.float32


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 1024))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 5500))
    data = synthetic.iris_shaped(dtype=DTYPE, device=DEVICE)
    dataloader = DataLoader(data, batch_size=len(data))
    hparams = mlp.Hyperparameters(dims=[4, 3, 3], activations=[torch.sigmoid, None])
    model = mlp.MLP(loss=loss_functions['multiclass_classification'], hparams=hparams, dtype=DTYPE, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, dtype=DTYPE, device=DEVICE),
                         torch.full((P,), 3.0 ** 0.5, dtype=DTYPE, device=DEVICE))

    theta0 = model.prior.sample((num_chains,))
    sampler = Gibbs(model, theta0=theta0, dataloader=dataloader, scales=[0.6, 0.6, 0.6, 0.9, 0.9, 0.9],
                    node_subblock_size=[2, 2, 2, None, None, None], seed=1)
    print(f"Parameter blocks (one per node): {model.num_par_blocks()}, sub-steps per draw: {sampler.num_substeps}")
    print(f"Sub-blocks: {sampler.get_blocks()}")
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=max(1, epochs // 11))
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"Time taken: {seconds:.2f} s  ->  {num_chains * epochs / seconds:.3e} draws/sec x chains "
          f"({num_chains * epochs * sampler.num_substeps / seconds:.3e} sub-steps/sec x chains)")

    chain = sampler.get_chain()  # ChainBuffer: sample [iters, C, P], accepted [iters, C, S] on the device
    rate = chain.acceptance_rate()  # [C, S]
    print(f"Stored samples per chain: {len(chain)}")
    print(f"Acceptance rate per sub-step (mean over chains): {[round(r, 3) for r in rate.mean(0).tolist()]}")
    print(f"Monte Carlo mean (chain 0): {chain.mean()[0].tolist()}")
    print(f"Posterior mean over all chains: {chain.get_samples().mean(dim=(0, 1)).tolist()}")


if __name__ == '__main__':
    main()
