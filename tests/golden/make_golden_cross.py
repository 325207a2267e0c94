#!/usr/bin/env python3
"""Generate tests/golden/g21_cross_traces.npz by running the REFERENCE (eeyore/models/bayesian_model.py) in f64 with a
non-Normal prior AND a regression loss together: ``model.prior`` a Laplace, StudentT or Cauchy distribution with distinct
per-parameter tables, ``loss`` one of make_golden_regression.py's three callables.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cross.py

It takes make_golden.py's helpers (the `kanga` stand-in, the recorder that wraps torch.randn / torch.rand / torch.normal),
make_golden_regression.py's model, rows and losses, and make_golden_priors.py's tables, so a trace is a pure function of
the recorded (z, u).  Everything is on MLP(2-3-1) tanh / none (P = 13) and that script's 40 synthetic rows (stored here
again: data/x, data/y, data/counts).

  values/<family>/<loss>   log_lik, log_prior, log_target and the gradient at 4 theta, for the 3 x 3 product of
                           laplace / studentt / cauchy and gauss / laplace / poisson
  trace/hmc                HMC (L = 5) under a Laplace prior and the Poisson loss, 60 draws
  trace/mala               MALA under a Student-t prior and the Gaussian loss, 60 draws
  trace/mh                 MetropolisHastings (NormalKernel) under a Cauchy prior and the Laplace loss, 60 draws

`meta` is a JSON string: the model (dims, activation codes), the scales of the losses and, per trace, its family, loss,
sampler and step (`par`: the step of HMC / MALA, the proposal scale of MH).  Every group stores the prior's tables [3, P]
(loc, scale, df; df NaN where the family has none); a values group theta [4, P], parts [4, 3] (log_lik, log_prior,
log_target) and grad [4, P]; a trace theta0, the initial target and gradient, the recorded z [n, P] / u [n] and the state
after every draw.  The script prints each trace's acceptance rate and its smallest |log u - log rate|: the seeds and steps
are chosen so that it stays above 1e-9 and both decisions occur.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
import make_golden_priors as mgp  # noqa: E402
import make_golden_regression as mgr  # noqa: E402

import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.samplers import HMC, MALA, MetropolisHastings  # noqa: E402

N_ITER, MODEL = 60, "mlp231"
F64 = torch.float64


def model_and_data(family, loss, seed):
    """make_golden_regression.py's model and rows under ``loss``, with the family's prior on distinct tables."""
    m, data = mgr.model_and_data(MODEL, loss)
    loc, scale, df = mgp.tables(m.num_params(), seed)
    m.prior = mgp.prior_of(family, loc, scale, df)
    return m, data, mgp.spec(family, loc, scale, df)


def values(family, loss, seed):
    m, data, rec = model_and_data(family, loss, seed)
    P = m.num_params()
    torch.manual_seed(seed)
    thetas = 0.7 * torch.randn(4, P, dtype=F64)
    lls, lps, lts, gs = [], [], [], []
    for th in thetas:
        lt, g = m.upto_grad_log_target(th.clone(), data.x, data.y)
        lts.append(mg.tnp(lt)); gs.append(mg.tnp(g))
        lls.append(mg.tnp(m.log_lik(data.x, data.y))); lps.append(mg.tnp(m.log_prior()))
    assert np.isfinite(np.array(lts)).all() and np.isfinite(np.array(gs)).all()
    rec.update(theta=mg.tnp(thetas), parts=np.stack([np.array(lls), np.array(lps), np.array(lts)], 1), grad=np.array(gs))
    return rec


def trace(family, loss, kind, seed, par):
    m, data, rec = model_and_data(family, loss, seed)
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
    rec.update({k: np.array(v) for k, v in out.items()})
    rec.update(z=np.array(zs), u=np.array(us), theta0=mg.tnp(th0), init_target=init_t, init_grad=init_g)
    print(f"g21 trace {kind} under {family} x {loss} P={P} acceptance {rec['accepted'].mean():.3f} "
          f"smallest |log u - log rate| {min(margins):.3e}")
    assert min(margins) > 1e-9 and 0 < rec["accepted"].sum() < N_ITER
    assert np.isfinite(rec["sample"]).all() and np.isfinite(rec["target_val"]).all()
    return rec


def main():
    torch.set_num_threads(1)
    dims, acts = mgr.MODELS[MODEL]
    out = {}
    meta = dict(model=dict(dims=dims, acts=[mgr.ACT[a] for a in acts]),
                scales={k: (1.0 if v is None else v) for k, v in mgr.SCALES.items()}, traces={})
    out["data/x"], out["data/y"], out["data/counts"] = mgr.rows(MODEL)
    for fi, family in enumerate(mgp.FAMILIES):
        for li, loss in enumerate(mgr.LOSSES):
            rec = values(family, loss, 2100 + 10 * fi + li)
            out.update({f"values/{family}/{loss}/{k}": np.asarray(v) for k, v in rec.items()})
    for kind, family, loss, seed, par in (("hmc", "laplace", "poisson", 2151, 0.08),
                                          ("mala", "studentt", "gauss", 2152, 0.01),
                                          ("mh", "cauchy", "laplace", 2153, 0.12)):
        rec = trace(family, loss, kind, seed, par)
        out.update({f"trace/{kind}/{k}": np.asarray(v) for k, v in rec.items()})
        meta["traces"][kind] = dict(family=family, loss=loss, par=par, **({"L": 5} if kind == "hmc" else {}))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(mg.HERE, "g21_cross_traces.npz")
    np.savez_compressed(path, **out)
    print("g21", len(out), os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 100 * 1024


if __name__ == "__main__":
    main()
