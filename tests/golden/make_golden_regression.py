#!/usr/bin/env python3
"""Generate tests/golden/g19_regression_traces.npz by running the REFERENCE (eeyore/models/bayesian_model.py:
log_lik = -loss(forward(x), y) with ``loss`` any callable) in f64 under the three regression losses.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_regression.py

It takes make_golden.py's helpers (the `kanga` stand-in, the recorder that wraps torch.randn / torch.rand / torch.normal),
so a trace is a pure function of the recorded (z, u).  The losses:

  gauss     lambda out, y: -Normal(out, 0.6).log_prob(y).sum()
  laplace   lambda out, y: -Laplace(out, 0.8).log_prob(y).sum()
  poisson   nn.PoissonNLLLoss(log_input=True, full=False, reduction='sum')

  values/<loss>/<model>   log_lik, log_prior, log_target and the gradient at 4 theta, for each loss and each model in
                            mlp231   MLP(2-3-1) tanh / none, P = 13
                            mlp432   MLP(4-3-2) sigmoid / none (two outputs), P = 23
  trace/gauss             HMC (L = 5) on mlp231, 60 draws
  trace/laplace           MALA on mlp432, 60 draws
  trace/poisson           MetropolisHastings (NormalKernel) on mlp231, 60 draws

Every model has 40 synthetic rows, stored here: data/<model>/x, data/<model>/y (continuous responses) and
data/<model>/counts (the responses of the Poisson loss).  The prior is N(0, 1.5^2) on every parameter.  `meta` is a JSON
string: the models (dims, activation codes), the scales, the prior's sigma and, per trace, its model, sampler and step
(`par`: the step of HMC / MALA, the proposal scale of MH).  A values group stores theta [4, P], parts [4, 3] (log_lik,
log_prior, log_target) and grad [4, P]; a trace theta0, the initial target and gradient, the recorded z [n, P] / u [n] and
the state after every draw.  The script prints each trace's acceptance rate and its smallest |log u - log rate|: the seeds
and steps are chosen so that it stays above 1e-9 and both decisions occur.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)

import torch  # noqa: E402
from torch.distributions import Laplace, Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.datasets import XYDataset  # noqa: E402
from eeyore.models import mlp  # noqa: E402
from eeyore.samplers import HMC, MALA, MetropolisHastings  # noqa: E402

N_ITER, N_ROWS, SIGMA = 60, 40, 1.5
F64 = torch.float64
SCALES = {"gauss": 0.6, "laplace": 0.8, "poisson": None}
LOSSES = {
    "gauss": lambda out, y: -Normal(out, SCALES["gauss"]).log_prob(y).sum(),
    "laplace": lambda out, y: -Laplace(out, SCALES["laplace"]).log_prob(y).sum(),
    "poisson": torch.nn.PoissonNLLLoss(log_input=True, full=False, reduction='sum'),
}
ACT = {None: 0, torch.sigmoid: 1, torch.tanh: 2}
MODELS = {"mlp231": ([2, 3, 1], [torch.tanh, None]), "mlp432": ([4, 3, 2], [torch.sigmoid, None])}


def rows(name):
    """x [40, d0], y [40, dK] continuous, counts [40, dK]: smooth functions of x plus noise, and Poisson draws."""
    dims, _ = MODELS[name]
    rng = np.random.default_rng(1900 + dims[0])
    x = rng.standard_normal((N_ROWS, dims[0]))
    f = np.stack([np.sin(x @ rng.standard_normal(dims[0])) for _ in range(dims[-1])], 1)
    return x, f + 0.3 * rng.standard_normal(f.shape), rng.poisson(np.exp(0.5 + 0.8 * f)).astype(np.float64)


def model_and_data(name, loss):
    dims, acts = MODELS[name]
    hp = mlp.Hyperparameters(dims=dims, bias=[True] * (len(dims) - 1), activations=acts)
    m = mlp.MLP(loss=LOSSES[loss], hparams=hp, dtype=F64)
    P = m.num_params()
    m.prior = Normal(torch.zeros(P, dtype=F64), SIGMA * torch.ones(P, dtype=F64))
    x, y, counts = rows(name)
    return m, XYDataset(torch.tensor(x), torch.tensor(counts if loss == "poisson" else y))


def values(name, loss, seed):
    m, data = model_and_data(name, loss)
    P = m.num_params()
    torch.manual_seed(seed)
    thetas = 0.7 * torch.randn(4, P, dtype=F64)
    lls, lps, lts, gs = [], [], [], []
    for th in thetas:
        lt, g = m.upto_grad_log_target(th.clone(), data.x, data.y)
        lts.append(mg.tnp(lt)); gs.append(mg.tnp(g))
        lls.append(mg.tnp(m.log_lik(data.x, data.y))); lps.append(mg.tnp(m.log_prior()))
    assert np.isfinite(np.array(lts)).all() and np.isfinite(np.array(gs)).all()
    return dict(theta=mg.tnp(thetas), parts=np.stack([np.array(lls), np.array(lps), np.array(lts)], 1), grad=np.array(gs))


def trace(name, loss, kind, seed, par):
    m, data = model_and_data(name, loss)
    P = m.num_params()
    loader = DataLoader(data, batch_size=len(data), shuffle=False)
    x, y = data.x, data.y
    torch.manual_seed(seed)
    th0 = 0.3 * torch.randn(P, dtype=F64)
    if kind == "hmc":
        s = HMC(m, theta0=th0.clone(), dataloader=loader, step=par, num_steps=5, chain=ChainList())
    elif kind == "mala":
        s = MALA(m, theta0=th0.clone(), dataloader=loader, step=par, chain=ChainList())
    else:
        s = MetropolisHastings(m, theta0=th0.clone(), dataloader=loader, chain=ChainList())
        s.kernel.set_density_params(th0.clone(), scale=torch.full([P], par, dtype=F64))
    init_t = mg.tnp(s.current["target_val"])
    init_g = mg.tnp(s.current["grad_val"]) if kind != "mh" else np.zeros(P)
    out = dict(sample=[], target_val=[], accepted=[])
    zs, us, margins = [], [], []
    s.counter.set_epoch_info(N_ITER, 0)
    for _ in range(N_ITER):
        th = s.current["sample"].detach().clone()
        t = float(s.current["target_val"].detach())
        g = s.current["grad_val"].detach().clone() if kind != "mh" else None
        with mg.Recorder() as r:
            s.draw(x, y, savestate=True)
        assert len(r.z) == 1 and len(r.u) == 1
        z = torch.tensor(r.z[0].reshape(-1), dtype=F64)
        u = float(r.u[0].reshape(-1)[0])
        zs.append(z.numpy()); us.append(u)
        # the margin of the decision, from the proposal rebuilt out of the recorded z
        if kind == "hmc":
            thp, pp, tp, _ = s.leapfrog(th.clone(), z.clone(), x, y)
            log_rate = float((-t + 0.5 * torch.sum(z ** 2)) - (-tp.detach() + 0.5 * torch.sum(pp.detach() ** 2)))
        elif kind == "mala":
            sd = torch.full([P], float(np.sqrt(par)), dtype=F64)
            mean = th + 0.5 * par * g
            thp = mean + sd * z
            tp, gp = m.upto_grad_log_target(thp.clone().detach(), x, y)
            log_rate = (float(tp.detach()) - t - float(Normal(mean, sd).log_prob(thp).sum())
                        + float(Normal(thp + 0.5 * par * gp.detach(), sd).log_prob(th).sum()))
        else:
            thp = th + par * z
            log_rate = float(m.log_target(thp.clone().detach(), x, y).detach()) - t
        m.set_params(s.current["sample"].clone().detach())
        if s.current["accepted"]:
            assert torch.allclose(s.current["sample"].detach(), thp.detach(), rtol=0, atol=1e-14)
        margins.append(abs(np.log(u) - log_rate))
        assert bool(s.current["accepted"]) == (np.log(u) < log_rate)
        out["sample"].append(mg.tnp(s.current["sample"]))
        out["target_val"].append(float(s.current["target_val"].detach()))
        out["accepted"].append(int(s.current["accepted"]))
        s.counter.increment_idx()
    rec = {k: np.array(v) for k, v in out.items()}
    rec.update(z=np.array(zs), u=np.array(us), theta0=mg.tnp(th0), init_target=init_t, init_grad=init_g)
    print(f"g19 trace {loss} {kind} on {name} P={P} acceptance {rec['accepted'].mean():.3f} "
          f"smallest |log u - log rate| {min(margins):.3e}")
    assert min(margins) > 1e-9 and 0 < rec["accepted"].sum() < N_ITER
    assert np.isfinite(rec["sample"]).all() and np.isfinite(rec["target_val"]).all()
    return rec


def main():
    torch.set_num_threads(1)
    out = {}
    meta = dict(models={name: dict(dims=dims, acts=[ACT[a] for a in acts]) for name, (dims, acts) in MODELS.items()},
                scales={k: (1.0 if v is None else v) for k, v in SCALES.items()}, sigma=SIGMA, traces={})
    for name in MODELS:
        out[f"data/{name}/x"], out[f"data/{name}/y"], out[f"data/{name}/counts"] = rows(name)
    for li, loss in enumerate(LOSSES):
        for mi, name in enumerate(MODELS):
            rec = values(name, loss, 1900 + 10 * li + mi)
            out.update({f"values/{loss}/{name}/{k}": np.asarray(v) for k, v in rec.items()})
    for loss, name, kind, seed, par in (("gauss", "mlp231", "hmc", 1951, 0.09),
                                        ("laplace", "mlp432", "mala", 1952, 0.012),
                                        ("poisson", "mlp231", "mh", 1953, 0.12)):
        rec = trace(name, loss, kind, seed, par)
        out.update({f"trace/{loss}/{k}": np.asarray(v) for k, v in rec.items()})
        meta["traces"][loss] = dict(model=name, sampler=kind, par=par, **({"L": 5} if kind == "hmc" else {}))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(mg.HERE, "g19_regression_traces.npz")
    np.savez_compressed(path, **out)
    print("g19", len(out), os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 100 * 1024


if __name__ == "__main__":
    main()
