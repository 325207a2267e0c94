"""HMC over the weights of MLP(4-8-3) on Iris under a Laplace (sparsity) prior, 256 chains at once on one MI355X.

``model.prior`` takes an elementwise ``torch.distributions`` Normal, Laplace, StudentT or Cauchy object, as in the
reference; with one of the last three the generic HIP kernels evaluate the prior and its gradient inside every leapfrog
step (the gradient of |theta| at 0 is taken as 0, what autograd gives).  A Laplace prior pulls the weights the data do not
need towards zero: the script prints the acceptance and the share of posterior means that end up near zero, beside the same
share under a Normal prior of the same variance.  EEYORE_EXAMPLE_CHAINS / EEYORE_EXAMPLE_EPOCHS shrink the run.
"""
import os
import sys

import torch
from torch.distributions import Laplace, Normal
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from eeyore_amd.constants import loss_functions
from eeyore_amd.datasets import XYDataset
from eeyore_amd.models import mlp
from eeyore_amd.samplers import HMC

DEVICE = 'cuda:0'
NUM_STEPS, STEP, NEAR_ZERO = 10, 0.02, 0.1


def posterior_means(prior_of, num_chains, epochs, loader):
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 8, 3], bias=2 * [True], activations=[torch.sigmoid, None]),
                    dtype=torch.float32, device=DEVICE)
    P = model.num_params()
    model.prior = prior_of(P)
    torch.manual_seed(0)
    sampler = HMC(model, theta0=0.1 * torch.randn(num_chains, P, device=DEVICE), dataloader=loader, step=STEP,
                  num_steps=NUM_STEPS, seed=1)
    sampler.run(num_epochs=epochs, num_burnin_epochs=epochs // 4)
    chain = sampler.get_chain()  # ChainBuffer: [iters, C, P] on the device
    x, y = next(iter(loader))
    return chain.get_samples().mean(0), chain.acceptance_rate().mean().item(), model._plan(x, y).kernel  # [C, P]


def main():
    num_chains = int(os.environ.get('EEYORE_EXAMPLE_CHAINS', 256))
    epochs = int(os.environ.get('EEYORE_EXAMPLE_EPOCHS', 2000))
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=torch.float32, device=DEVICE)
    loader = DataLoader(iris, batch_size=len(iris), shuffle=False)
    b = 0.5  # Laplace(0, b) has variance 2 b^2: the Normal prior beside it has the same
    priors = {
        'Laplace': lambda P: Laplace(torch.zeros(P, device=DEVICE), torch.full((P,), b, device=DEVICE)),
        'Normal': lambda P: Normal(torch.zeros(P, device=DEVICE), torch.full((P,), b * 2 ** 0.5, device=DEVICE)),
    }
    for name, prior_of in priors.items():
        means, acceptance, kernel = posterior_means(prior_of, num_chains, epochs, loader)
        near = (means.abs() < NEAR_ZERO).float().mean().item()
        print(f"{name} prior ({kernel} kernels): mean acceptance rate {acceptance:.3f}, "
              f"share of posterior means with |mean| < {NEAR_ZERO}: {near:.3f}")


if __name__ == '__main__':
    main()
