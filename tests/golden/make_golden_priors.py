#!/usr/bin/env python3
"""Generate tests/golden/g18_prior_traces.npz by running the REFERENCE (eeyore/models/bayesian_model.py with
``model.prior`` a Laplace, StudentT or Cauchy distribution) in f64.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_priors.py

It takes make_golden.py's helpers (the `kanga` stand-in, the recorder that wraps torch.randn / torch.rand / torch.normal),
so a trace is a pure function of the recorded (z, u).  Every prior has a distinct loc, scale and (Student-t) df for every
parameter.

  values/<family>/<model>   log_lik, log_prior, log_target and the gradient at 4 theta, for each family in
                            laplace / studentt / cauchy and each model in
                              mlp433   MLP(4-3-3) sigmoid / none, CE, iris, P = 27
                              mlp2321  MLP(2-3-2-1) sigmoid / tanh / sigmoid, BCE, xor, P = 20
                              lr       make_golden_ram.py's LogisticRegression(4, bias) on its 40 synthetic rows, P = 5
  trace/laplace             HMC (L = 5) on mlp433, 60 draws
  trace/studentt            MALA on mlp2321, 60 draws
  trace/cauchy              MetropolisHastings (NormalKernel, scale 0.25) on lr, 60 draws

`meta` is a JSON string: the models (dims, activation codes, likelihood code, data set: iris and xor are the arrays of
datasets.npz, the logistic regression's rows are data/lr/x, data/lr/y) and, per trace, its model, sampler and step (`par`:
the step of HMC / MALA, the proposal scale of MH).  Every group stores the prior's tables [3, P] (loc, scale, df; df NaN
where the family has none); a values group theta [4, P], parts [4, 3] (log_lik, log_prior, log_target) and grad [4, P]; a
trace theta0, the initial target and gradient, the recorded z [n, P] / u [n] and the state after every draw.  The script prints each trace's acceptance rate and its smallest
|log u - log rate|: the seeds are chosen so that it stays above 1e-9 and both decisions occur.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
import make_golden_ram as mgr  # noqa: E402

import torch  # noqa: E402
from torch.distributions import Cauchy, Laplace, Normal, StudentT  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.constants import loss_functions  # noqa: E402
from eeyore.models import mlp  # noqa: E402
from eeyore.samplers import HMC, MALA, MetropolisHastings  # noqa: E402

N_ITER = 60
F64 = torch.float64
FAMILIES = ("laplace", "studentt", "cauchy")


def tables(P, seed):
    """loc, scale, df [P], every entry different: shuffled grids, so neighbouring parameters do not have neighbouring
    tables."""
    rng = np.random.default_rng(seed)
    loc = rng.permutation(np.linspace(-0.4, 0.5, P))
    scale = rng.permutation(np.linspace(0.6, 2.2, P))
    df = rng.permutation(np.linspace(1.5, 9.0, P))
    return loc, scale, df


def prior_of(family, loc, scale, df):
    loc, scale, df = (torch.tensor(a, dtype=F64) for a in (loc, scale, df))
    return {"laplace": lambda: Laplace(loc, scale), "studentt": lambda: StudentT(df, loc, scale),
            "cauchy": lambda: Cauchy(loc, scale)}[family]()


def models():
    """name -> (model factory, dataset, dims, activations, likelihood)"""
    d = mg.datasets(F64)

    def mlp_of(dims, acts, lik):
        hp = mlp.Hyperparameters(dims=dims, bias=[True] * (len(dims) - 1), activations=acts)
        return lambda: mlp.MLP(loss=loss_functions[lik], hparams=hp, dtype=F64)

    a433, a2321 = [torch.sigmoid, None], [torch.sigmoid, torch.tanh, torch.sigmoid]
    return {
        "mlp433": (mlp_of([4, 3, 3], a433, "multiclass_classification"), d["iris"], [4, 3, 3], a433,
                   "multiclass_classification"),
        "mlp2321": (mlp_of([2, 3, 2, 1], a2321, "binary_classification"), d["xor"], [2, 3, 2, 1], a2321,
                    "binary_classification"),
        "lr": (mgr.lr_model, mgr.lr_data(), [4, 1], [torch.sigmoid], "binary_classification"),
    }


def spec(family, loc, scale, df):
    """The prior's tables as one array [3, P]: loc, scale, df (df is NaN where the family has none)."""
    return dict(tables=np.stack([loc, scale, df if family == "studentt" else np.full_like(loc, np.nan)]))


def values(name, family, seed):
    make, data, dims, acts, lik = models()[name]
    m = make()
    P = m.num_params()
    loc, scale, df = tables(P, seed)
    m.prior = prior_of(family, loc, scale, df)
    torch.manual_seed(seed)
    thetas = 0.7 * torch.randn(4, P, dtype=F64)
    lls, lps, lts, gs = [], [], [], []
    for th in thetas:
        lt, g = m.upto_grad_log_target(th.clone(), data.x, data.y)
        lts.append(mg.tnp(lt)); gs.append(mg.tnp(g))
        lls.append(mg.tnp(m.log_lik(data.x, data.y))); lps.append(mg.tnp(m.log_prior()))
    rec = spec(family, loc, scale, df)
    rec.update(theta=mg.tnp(thetas), parts=np.stack([np.array(lls), np.array(lps), np.array(lts)], 1), grad=np.array(gs))
    return rec


def trace(name, family, kind, seed, par):
    make, data, dims, acts, lik = models()[name]
    m = make()
    P = m.num_params()
    loc, scale, df = tables(P, seed)
    m.prior = prior_of(family, loc, scale, df)
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
    rows = dict(sample=[], target_val=[], accepted=[])
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
        rows["sample"].append(mg.tnp(s.current["sample"]))
        rows["target_val"].append(float(s.current["target_val"].detach()))
        rows["accepted"].append(int(s.current["accepted"]))
        s.counter.increment_idx()
    rec = spec(family, loc, scale, df)
    rec.update({k: np.array(v) for k, v in rows.items()})
    rec.update(z=np.array(zs), u=np.array(us), theta0=mg.tnp(th0), init_target=init_t, init_grad=init_g)
    print(f"g18 trace {family} {kind} on {name} P={P} acceptance {rec['accepted'].mean():.3f} "
          f"smallest |log u - log rate| {min(margins):.3e}")
    assert min(margins) > 1e-9 and 0 < rec["accepted"].sum() < N_ITER
    return rec


def main():
    torch.set_num_threads(1)
    out = {}
    # one JSON entry describes the models and the traces (many small arrays would cost more than the numbers they hold);
    # iris and xor are the arrays of datasets.npz, the logistic regression's rows are stored here
    ms = models()
    meta = dict(models={name: dict(dims=dims, acts=[mgr.ACT[a] for a in acts], lik=mgr.LIK[lik],
                                   data={"mlp433": "iris", "mlp2321": "xor", "lr": "lr"}[name])
                        for name, (_, _, dims, acts, lik) in ms.items()}, traces={})
    shipped = np.load(os.path.join(mg.HERE, "datasets.npz"))
    for name, ds in (("mlp433", "iris"), ("mlp2321", "xor")):
        assert np.array_equal(shipped[f"{ds}_x"], ms[name][1].x.numpy()) and np.array_equal(shipped[f"{ds}_y"], ms[name][1].y.numpy())
    out["data/lr/x"], out["data/lr/y"] = ms["lr"][1].x.numpy(), ms["lr"][1].y.numpy()
    for fi, family in enumerate(FAMILIES):
        for mi, name in enumerate(("mlp433", "mlp2321", "lr")):
            rec = values(name, family, 1800 + 10 * fi + mi)
            out.update({f"values/{family}/{name}/{k}": np.asarray(v) for k, v in rec.items()})
    for family, name, kind, seed, par in (("laplace", "mlp433", "hmc", 1851, 0.07),
                                          ("studentt", "mlp2321", "mala", 1852, 0.5),
                                          ("cauchy", "lr", "mh", 1853, 0.25)):
        rec = trace(name, family, kind, seed, par)
        out.update({f"trace/{family}/{k}": np.asarray(v) for k, v in rec.items()})
        meta["traces"][family] = dict(model=name, sampler=kind, par=par, **({"L": 5} if kind == "hmc" else {}))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(mg.HERE, "g18_prior_traces.npz")
    np.savez_compressed(path, **out)
    print("g18", len(out), os.path.getsize(path), "bytes;",
          "g17 is", os.path.getsize(os.path.join(mg.HERE, "g17_mala_mvn_traces.npz")), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(mg.HERE, "g17_mala_mvn_traces.npz"))


if __name__ == "__main__":
    main()
