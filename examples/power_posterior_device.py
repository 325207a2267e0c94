"""Parallel tempering with the between-chain moves on the device: 8 temperatures x 512 replicas of the ladder, MALA over
the weights of MLP(2-3-2-1) on the XOR data.

``between='device'`` makes every between-chain move one HIP launch (``ey_pt_between``: partners and accept variates from
the in-kernel Philox stream) and lets ``run`` issue the within-chain draws between two moves as one launch; the 8 x 512
chains record into one device buffer of which ``get_chain(i)`` is the view of temperature i.  The default,
``between='host'``, walks the temperatures on the host with torch's generator.  EEYORE_EXAMPLE_REPLICAS /
EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys
import time

import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.constants import loss_functions
from eeyore_amd.datasets import XYDataset
from eeyore_amd.models import mlp
from eeyore_amd.samplers import PowerPosteriorSampler

DEVICE = 'cuda:0'
NUM_TEMPERATURES = 8


def main():
    replicas = int(os.environ.get('EEYORE_EXAMPLE_REPLICAS', 512))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 2200))
    xor = XYDataset.from_eeyore('xor', dtype=torch.float32, device=DEVICE)
    loader = DataLoader(xor, batch_size=len(xor), shuffle=False)
    model = mlp.MLP(loss=loss_functions['binary_classification'],
                    hparams=mlp.Hyperparameters(dims=[2, 3, 2, 1], bias=3 * [True], activations=3 * [torch.sigmoid]),
                    dtype=torch.float32, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEVICE), torch.full((P,), 10.0, device=DEVICE).sqrt())

    sampler = PowerPosteriorSampler(model, loader, [['MALA', {'step': 0.1}] for _ in range(NUM_TEMPERATURES)],
                                    theta0=0.5 * torch.randn(replicas, P, device=DEVICE), between_step=10, seed=1,
                                    keys=['sample', 'target_val', 'accepted'], between='device')
    t0 = time.perf_counter()
    sampler.run(num_epochs=epochs, num_burnin_epochs=epochs // 11)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"Time taken: {seconds:.2f} s for {epochs} draws of {NUM_TEMPERATURES} x {replicas} chains")

    cold = sampler.get_chain()  # the t = 1 chain: a view [iters, R, P] of the one record buffer
    print(f"Stored samples per chain: {len(cold)}")
    for k in (0, NUM_TEMPERATURES - 1):
        chain = sampler.get_chain(k)
        print(f"temperature {sampler.temperature[k]:.4f}: mean acceptance {chain.acceptance_rate().mean().item():.3f}, "
              f"mean tempered log-target {chain.get_target_vals().mean().item():.2f}")
    swaps = torch.stack([swap for _, swap, _ in sampler.last_swaps]).float().mean(1)
    print("exchange rate per temperature in the last move:", [round(v, 2) for v in swaps.tolist()])


if __name__ == '__main__':
    main()
