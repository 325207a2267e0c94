#!/usr/bin/env python3
"""Generate tests/golden/g11_ram_traces.npz by running the REFERENCE's robust adaptive Metropolis sampler
(eeyore/samplers/ram.py) in the build container.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ram.py

It takes make_golden.py's approach and its helpers (the `kanga` stand-in, the recorder that wraps torch.randn /
torch.rand): a trace is then a pure function of the recorded (z, u) streams.  Every group stores the target's spec, the
inputs, the adaptation index n of every draw, the recorded z [n_iter, P] / u [n_iter], the state after every draw and
the factor chol_cov after every 10th draw and after the last.

  a  LogisticRegression(4, bias), BCE, f64, 40 synthetic rows, 300 iterations with the defaults
  b  MLP(2-3-2-1) sigmoid / tanh / sigmoid, BCE, f64, xor, cov0 = 0.1 I, 300 iterations
  c  MLP(4-3-3) sigmoid / none, CE, f64, iris, a = 0.3, g = 0.6, 200 iterations
  d  the model of (a), 40 direct draw(x, y, offset=5) calls with the counter at 10, 11, ...
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)

import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.constants import loss_functions  # noqa: E402
from eeyore.datasets import XYDataset  # noqa: E402
from eeyore.models import logistic_regression, mlp  # noqa: E402
from eeyore.samplers import RAM  # noqa: E402

ACT = {None: 0, torch.sigmoid: 1, torch.tanh: 2}
LIK = {"binary_classification": 0, "multiclass_classification": 1}


def lr_data(n=40, d=4, seed=11):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    logit = x @ np.array([1.0, -0.5, 0.25, 0.8]) + 0.3
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float64)[:, None]
    return XYDataset(torch.tensor(x), torch.tensor(y))


def trace(sampler, data, dims, acts, lik, n_iter, offset=0, idx0=0):
    loader = DataLoader(data, batch_size=len(data))
    x, y = next(iter(loader))
    sampler.counter.idx = idx0
    rec = dict(n=[], sample=[], target_val=[], accepted=[], chol=[], chol_it=[])
    with mg.Recorder() as r:
        for it in range(n_iter):
            rec["n"].append(sampler.counter.idx + 1 - offset)
            sampler.draw(x, y, offset=offset)
            rec["sample"].append(mg.tnp(sampler.current["sample"]))
            rec["target_val"].append(float(sampler.current["target_val"].detach()))
            rec["accepted"].append(int(sampler.current["accepted"]))
            if (it + 1) % 10 == 0 or it == n_iter - 1:
                rec["chol"].append(mg.tnp(sampler.chol_cov))
                rec["chol_it"].append(it)
            sampler.counter.increment_idx()
    assert len(r.z) == len(r.u) == n_iter
    P = sampler.model.num_params()
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(z=np.stack(r.z).reshape(n_iter, P), u=np.array([v.item() for v in r.u]),
               dims=np.array(dims), acts=np.array([ACT[a] for a in acts]), lik=np.array(LIK[lik]),
               x=data.x.numpy(), y=data.y.numpy(), prior_mu=np.zeros(P), prior_sigma=np.ones(P),
               a=np.array(sampler.a), g=np.array(sampler.g), offset=np.array(offset))
    print(f"g11 P={P} iterations={n_iter} acceptance {out['accepted'].mean():.3f}")
    return out


def lr_model():
    hp = logistic_regression.Hyperparameters(input_size=4, bias=True)
    return logistic_regression.LogisticRegression(loss=loss_functions["binary_classification"], hparams=hp,
                                                  dtype=torch.float64)


def group(name, model, data, dims, acts, lik, n_iter, cov0=None, a=0.234, g=0.7, offset=0, idx0=0):
    torch.manual_seed(1000 + ord(name))
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, dtype=torch.float64), torch.ones(P, dtype=torch.float64))
    theta0 = model.prior.sample()
    loader = DataLoader(data, batch_size=len(data))
    s = RAM(model, theta0=theta0.clone(), dataloader=loader, cov0=cov0, a=a, g=g)
    init_t = float(s.current["target_val"].detach())
    out = trace(s, data, dims, acts, lik, n_iter, offset=offset, idx0=idx0)
    out.update(theta0=mg.tnp(theta0), init_target=np.array(init_t), cov0=mg.tnp(s.cov0))
    return {f"{name}/{k}": v for k, v in out.items()}


def main():
    torch.set_num_threads(1)
    d = mg.datasets(torch.float64)
    out = {}
    out.update(group("a", lr_model(), lr_data(), [4, 1], [torch.sigmoid], "binary_classification", 300))
    hp = mlp.Hyperparameters(dims=[2, 3, 2, 1], bias=[True] * 3, activations=[torch.sigmoid, torch.tanh, torch.sigmoid])
    m = mlp.MLP(loss=loss_functions["binary_classification"], hparams=hp, dtype=torch.float64)
    out.update(group("b", m, d["xor"], [2, 3, 2, 1], hp.activations, "binary_classification", 300,
                     cov0=0.1 * torch.eye(m.num_params(), dtype=torch.float64)))
    hp = mlp.Hyperparameters(dims=[4, 3, 3], bias=[True] * 2, activations=[torch.sigmoid, None])
    m = mlp.MLP(loss=loss_functions["multiclass_classification"], hparams=hp, dtype=torch.float64)
    out.update(group("c", m, d["iris"], [4, 3, 3], hp.activations, "multiclass_classification", 200, a=0.3, g=0.6))
    out.update(group("d", lr_model(), lr_data(), [4, 1], [torch.sigmoid], "binary_classification", 40, offset=5,
                     idx0=10))
    path = os.path.join(mg.HERE, "g11_ram_traces.npz")
    np.savez_compressed(path, **out)
    print("g11", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
