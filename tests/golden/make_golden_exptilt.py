#!/usr/bin/env python3
"""Generate tests/golden/g20_exptilt_traces.npz by running the REFERENCE's samplers on its DistributionModel
(eeyore/models/distribution_model.py) with the closure densities written below, in f64.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_exptilt.py

It takes make_golden_dist.py's approach and make_golden.py's helpers (the `kanga` stand-in, the recorder that wraps
torch.randn / torch.rand): a trace is a pure function of the recorded draws.  Three targets, 50 draws per sampler:

  u  P = 1, the reference's unnormalised Gamma example verbatim (v = (2, 1), theta0 = -1): HMC (L = 3), MALA (step 0.25), MH
  n  P = 1, its normalised example (torch.distributions.Gamma): the same three
  m  P = 4, one coordinate each of Gamma, InverseGamma, Weibull (theta = log x plus the Jacobian) and Gumbel, all normalised,
     written with torch.distributions: HMC, MALA, MH, RAM and AM

Every group <target>/<sampler>/ stores theta0, the initial target (and gradient), the recorded z / u (AM: u_mix too), the
state after every draw and the sampler's settings; RAM and AM also their adapted matrices after the last draw.  Per target
the constructor arguments are stored under <target>/args/ and the tables (c, a, b, s) the named constructors of
eeyore_amd.models.targets are expected to produce under <target>/tables/, worked out below from the densities' textbook
forms.  HMC, MALA and MH must accept between 15 and 45 of their 50 proposals (asserted).
"""
import math
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
from make_golden_dist import adaptive_trace  # noqa: E402

import torch  # noqa: E402
from torch.distributions import Gamma, Gumbel, InverseGamma, Weibull  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.datasets import EmptyXYDataset  # noqa: E402
from eeyore.models import DistributionModel  # noqa: E402
from eeyore.samplers import AM, HMC, MALA, RAM, MetropolisHastings  # noqa: E402

N_ITER = 50
F64 = torch.float64

# the constructor arguments: u / n LogGamma(shape, scale); m one coordinate per family
ARGS = {
    "u": dict(shape=2.0, scale=1.0, normalized=0),
    "n": dict(shape=2.0, scale=1.0, normalized=1),
    "m": dict(gamma_shape=3.0, gamma_scale=0.5, invgamma_shape=2.5, invgamma_rate=1.5, weibull_scale=1.3,
              weibull_concentration=1.7, gumbel_loc=0.4, gumbel_scale=0.8, normalized=1),
}
# per target: theta0, HMC step, MALA step, MH scale, and the generator's seed for the MALA trace.  MALA's step on u and n is
# the example's, at which about 96 of 100 proposals are accepted: of the generator seeds 0..299 these are the first two whose
# 50 draws hold six rejections (44 accepts each; five more seeds give 45); every other trace takes the seed written in main().
SETTINGS = {"u": dict(theta0=[-1.0], hmc=1.0, mala=0.25, mh=2.5, mala_seed=142),
            "n": dict(theta0=[-1.0], hmc=1.0, mala=0.25, mh=2.5, mala_seed=182),
            "m": dict(theta0=[0.2, -0.3, 0.1, 0.5], hmc=0.55, mala=0.45, mh=0.6, am_b=2.38 / np.sqrt(4), am_c=0.5,
                      mala_seed=2000 + ord("m"))}


def tables(name):
    """(c, a, b, s) of log p = sum_i [c_i + a_i theta_i - b_i exp(s_i theta_i)] from the densities' textbook forms."""
    g = ARGS[name]
    if name in "un":
        k, t = g["shape"], g["scale"]
        c = -math.lgamma(k) - k * math.log(t) if g["normalized"] else 0.0
        return np.array([c]), np.array([k]), np.array([1.0 / t]), np.array([1.0])
    k, t = g["gamma_shape"], g["gamma_scale"]
    ik, ir = g["invgamma_shape"], g["invgamma_rate"]
    lam, wk = g["weibull_scale"], g["weibull_concentration"]
    mu, beta = g["gumbel_loc"], g["gumbel_scale"]
    c = [-math.lgamma(k) - k * math.log(t), ik * math.log(ir) - math.lgamma(ik), math.log(wk) - wk * math.log(lam),
         -math.log(beta) + mu / beta]
    a = [k, -ik, wk, -1.0 / beta]
    b = [1.0 / t, ir, lam ** -wk, math.exp(mu / beta)]
    s = [1.0, -1.0, wk, -1.0 / beta]
    return tuple(np.array(v, np.float64) for v in (c, a, b, s))


def closure(name):
    if name == "u":
        v = torch.tensor([2., 1.], dtype=torch.float64)

        def log_pdf(theta, x, y):
            return (v[0] - 1) * theta - torch.exp(theta) / v[1] + theta  # the last term: the Jacobian of theta = log x
        return log_pdf
    if name == "n":
        v = torch.tensor([2., 1.], dtype=torch.float64)

        def log_pdf(theta, x, y):
            return Gamma(v[0], 1 / v[1]).log_prob(torch.exp(theta)) + theta
        return log_pdf
    g = {k: torch.tensor(v, dtype=F64) for k, v in ARGS["m"].items()}

    def log_pdf(theta, x, y):
        return (Gamma(g["gamma_shape"], 1 / g["gamma_scale"]).log_prob(torch.exp(theta[0])) + theta[0]
                + InverseGamma(g["invgamma_shape"], g["invgamma_rate"]).log_prob(torch.exp(theta[1])) + theta[1]
                + Weibull(g["weibull_scale"], g["weibull_concentration"]).log_prob(torch.exp(theta[2])) + theta[2]
                + Gumbel(g["gumbel_loc"], g["gumbel_scale"]).log_prob(theta[3]))
    return log_pdf


def model_of(name):
    return DistributionModel(closure(name), len(SETTINGS[name]["theta0"]), dtype=F64)


def scalar(v):
    """The closures of u and n return a tensor of shape [1] (theta is [1]): the targets are stored as numbers."""
    return np.asarray(mg.tnp(v), np.float64).reshape(-1)[0]


def main():
    torch.set_num_threads(1)
    data = EmptyXYDataset()
    loader = DataLoader(data)
    x, y = next(iter(loader))
    out = {}
    for name in "unm":
        st = SETTINGS[name]
        P = len(st["theta0"])
        for k, v in ARGS[name].items():
            out[f"{name}/args/{k}"] = np.array(v)
        for k, v in zip("cabs", tables(name)):
            out[f"{name}/tables/{k}"] = v
        torch.manual_seed(2000 + ord(name))
        theta0 = torch.tensor(st["theta0"], dtype=F64)
        groups = {}
        s = HMC(model_of(name), theta0=theta0.clone(), dataloader=loader, step=st["hmc"], num_steps=3, chain=ChainList())
        init = dict(init_target=scalar(s.current["target_val"]), init_grad=mg.tnp(s.current["grad_val"]))
        groups["hmc"] = dict(mg.run_trace(s, data, N_ITER), step=np.array(st["hmc"]), L=np.array(3), **init)
        torch.manual_seed(st["mala_seed"])
        s = MALA(model_of(name), theta0=theta0.clone(), dataloader=loader, step=st["mala"], chain=ChainList())
        init = dict(init_target=scalar(s.current["target_val"]), init_grad=mg.tnp(s.current["grad_val"]))
        groups["mala"] = dict(mg.run_trace(s, data, N_ITER), step=np.array(st["mala"]), **init)
        torch.manual_seed(3000 + ord(name))
        s = MetropolisHastings(model_of(name), theta0=theta0.clone(), dataloader=loader, chain=ChainList())
        s.kernel.set_density_params(theta0.clone(), scale=torch.full([P], st["mh"], dtype=F64))
        init_t = scalar(s.current["target_val"])
        groups["mh"] = dict(mg.run_trace(s, data, N_ITER), scale=np.array(st["mh"]), init_target=init_t)
        if name == "m":
            s = RAM(model_of(name), theta0=theta0.clone(), dataloader=loader, cov0=0.3 * torch.eye(P, dtype=F64))
            init_t = float(s.current["target_val"].detach())
            groups["ram"] = dict(adaptive_trace(s, x, y, P, False), init_target=np.array(init_t), cov0=mg.tnp(s.cov0),
                                 a=np.array(s.a), g=np.array(s.g), chol=mg.tnp(s.chol_cov))
            eps, eye = 1e-6, torch.eye(P, dtype=F64)
            s = AM(model_of(name), theta0=theta0.clone(), dataloader=loader, l=0.2, b=st["am_b"], c=st["am_c"], t0=5,
                   transform=lambda cov: cov + eps * eye)
            init_t = float(s.current["target_val"].detach())
            rec = adaptive_trace(s, x, y, P, True)
            after = rec["n"] > 5
            iso = int((rec["u_mix"][after] < 0.2).sum())
            assert iso >= 3 and int(after.sum()) - iso >= 3, (name, iso)
            groups["am"] = dict(rec, init_target=np.array(init_t), cov0=mg.tnp(s.cov0), eps=np.array(eps), l=np.array(0.2),
                                b=np.array(st["am_b"]), c=np.array(st["am_c"]), t0=np.array(5),
                                cov=np.tril(mg.tnp(s.cov)), running_mean=mg.tnp(s.running_mean),
                                cov_sum=np.tril(mg.tnp(s.cov_sum)), num_accepted=np.array(int(s.num_accepted)))
        for g, rec in groups.items():
            n_acc = int(np.sum(rec["accepted"]))
            print(f"g20 {name}/{g} accepts {n_acc} of {N_ITER}")
            if g in ("hmc", "mala", "mh"):
                assert 15 <= n_acc <= 45, (name, g, n_acc)
            else:
                assert 0 < n_acc < N_ITER, (name, g, n_acc)
            out[f"{name}/{g}/theta0"] = mg.tnp(theta0)
            for k, v in rec.items():
                v = np.asarray(v)
                if k == "target_val":
                    v = v.reshape(N_ITER)
                out[f"{name}/{g}/{k}"] = v
    path = os.path.join(mg.HERE, "g20_exptilt_traces.npz")
    np.savez_compressed(path, **out)
    print("g20", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
