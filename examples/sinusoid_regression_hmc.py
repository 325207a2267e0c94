"""A Bayesian neural network on a continuous response: HMC over the weights of MLP(1-16-1) (tanh, identity output) on 64
rows of y = sin(3x) + noise, 256 chains at once on one MI355X.

``loss_functions['regression']`` is the Gaussian likelihood with noise scale 1 (``gaussian_loss(scale)`` for another scale;
'robust_regression' / ``laplace_loss`` and 'count_regression' / ``poisson_loss`` are the Laplace and Poisson forms), i.e. the
reference's ``loss = lambda out, y: -Normal(out, s).log_prob(y).sum()``.  ``predict_batched`` returns the posterior predictive
mean and standard deviation of the network output on a grid, from the outputs of every stored sample in one device pass.
EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys

import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.constants import gaussian_loss
from eeyore_amd.datasets import XYDataset
from eeyore_amd.models import mlp
from eeyore_amd.samplers import HMC

DEVICE = 'cuda:0'
NOISE, NUM_STEPS, STEP = 0.2, 10, 0.004


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 256))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 1000))
    gen = torch.Generator().manual_seed(0)
    x = 2 * torch.rand(64, 1, generator=gen) - 1
    y = torch.sin(3 * x) + NOISE * torch.randn(64, 1, generator=gen)
    data = XYDataset(x.to(DEVICE), y.to(DEVICE))
    loader = DataLoader(data, batch_size=len(data), shuffle=False)
    model = mlp.MLP(loss=gaussian_loss(NOISE),
                    hparams=mlp.Hyperparameters(dims=[1, 16, 1], bias=2 * [True], activations=[torch.tanh, None]),
                    dtype=torch.float32, device=DEVICE)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEVICE), torch.full((P,), 3.0, device=DEVICE))
    sampler = HMC(model, theta0=0.1 * torch.randn(num_chains, P, generator=gen).to(DEVICE), dataloader=loader, step=STEP,
                  num_steps=NUM_STEPS, seed=1)
    sampler.run(num_epochs=epochs, num_burnin_epochs=epochs // 2)
    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    print(f"Gaussian likelihood, scale {NOISE} ({model._plan(data.x, data.y).kernel} kernels): "
          f"mean acceptance rate {chain.acceptance_rate().mean().item():.3f}")
    samples = chain.get_samples()[-1]  # the last state of every chain: num_chains draws
    grid = torch.linspace(-1, 1, 9, device=DEVICE).reshape(-1, 1)
    mean, sd, dropped = model.predict_batched(samples, grid)
    print("      x   sin(3x)   predictive mean       sd")
    for xi, mi, si in zip(grid[:, 0].tolist(), mean[:, 0].tolist(), sd[:, 0].tolist()):
        print(f"{xi:7.2f} {torch.sin(torch.tensor(3 * xi)).item():9.3f} {mi:17.3f} {si:8.3f}")
    print(f"samples dropped for a non-finite output: {int(dropped.sum().item())}")


if __name__ == '__main__':
    main()
