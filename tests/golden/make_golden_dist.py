#!/usr/bin/env python3
"""Generate tests/golden/g14_distribution_traces.npz by running the REFERENCE's samplers on its DistributionModel
(eeyore/models/distribution_model.py) with closure densities written below, in f64.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dist.py

It takes make_golden.py's approach and its helpers (the `kanga` stand-in, the recorder that wraps torch.randn /
torch.rand): a trace is a pure function of the recorded draws.  Two targets, 50 draws each of HMC (L = 3), MALA, MH, RAM
and AM:

  a  P = 2, one normalised component with a correlated covariance (torch.distributions.MultivariateNormal.log_prob)
  b  P = 3, two components with unequal weights and covariances, not normalised:
     log(w_0 exp(-d_0' inv(S_0) d_0 / 2) + w_1 exp(-d_1' inv(S_1) d_1 / 2))

Every group <target>/<sampler>/ stores theta0, the initial target (and gradient), the recorded z / u (AM: u_mix too), the
state after every draw and the sampler's settings; RAM and AM also their adapted matrices after the last draw.  The
target's weights, means, covs and `normalized` are stored once per target.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)

import torch  # noqa: E402
from torch.distributions import MultivariateNormal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.datasets import EmptyXYDataset  # noqa: E402
from eeyore.models import DistributionModel  # noqa: E402
from eeyore.samplers import AM, HMC, MALA, RAM, MetropolisHastings  # noqa: E402

N_ITER = 50
F64 = torch.float64

TARGETS = {
    "a": dict(weights=[1.0], means=[[0.5, -1.0]], covs=[[[1.0, 0.6], [0.6, 0.8]]], normalized=True),
    "b": dict(weights=[0.3, 1.1], means=[[-1.0, 0.5, 0.0], [1.5, -0.5, 1.0]],
              covs=[[[1.0, 0.3, 0.0], [0.3, 0.7, -0.2], [0.0, -0.2, 0.5]],
                    [[0.6, -0.1, 0.2], [-0.1, 1.2, 0.4], [0.2, 0.4, 0.9]]], normalized=False),
}
# per target: HMC step, MALA step, MH scale, AM (b, c)
SETTINGS = {"a": dict(hmc=1.04, mala=0.5, mh=0.9, am_b=2.38 / np.sqrt(2), am_c=0.7),
            "b": dict(hmc=0.4, mala=0.35, mh=0.7, am_b=2.38 / np.sqrt(3), am_c=0.5)}


def closure(spec):
    w = torch.tensor(spec["weights"], dtype=F64)
    means = [torch.tensor(m, dtype=F64) for m in spec["means"]]
    covs = [torch.tensor(c, dtype=F64) for c in spec["covs"]]
    if spec["normalized"]:
        assert len(means) == 1
        return lambda theta, x, y: MultivariateNormal(means[0], covariance_matrix=covs[0]).log_prob(theta)
    precs = [torch.inverse(c) for c in covs]

    def log_pdf(theta, x, y):
        terms = [w[k] * torch.exp(-0.5 * torch.dot(theta - means[k], precs[k] @ (theta - means[k])))
                 for k in range(len(means))]
        return torch.log(sum(terms))
    return log_pdf


def model_of(spec):
    return DistributionModel(closure(spec), len(spec["means"][0]), dtype=F64)


def adaptive_trace(s, x, y, P, is_am):
    rec = {k: [] for k in ("n", "idx", "z", "u_mix", "u", "sample", "target_val", "accepted")}
    with mg.Recorder() as r:
        for it in range(N_ITER):
            n = s.counter.idx + 1
            nu = len(r.u)
            s.draw(x, y)
            two = is_am and n > s.t0
            assert len(r.u) == nu + (2 if two else 1)
            rec["n"].append(n)
            rec["idx"].append(s.counter.idx)
            rec["z"].append(r.z[-1].reshape(P))
            rec["u_mix"].append(r.u[-2].item() if two else np.nan)
            rec["u"].append(r.u[-1].item())
            rec["sample"].append(mg.tnp(s.current["sample"]))
            rec["target_val"].append(float(s.current["target_val"].detach()))
            rec["accepted"].append(int(s.current["accepted"]))
            s.counter.increment_idx()
    return {k: np.array(v) for k, v in rec.items()}


def main():
    torch.set_num_threads(1)
    data = EmptyXYDataset()
    loader = DataLoader(data)
    x, y = next(iter(loader))
    out = {}
    for name, spec in TARGETS.items():
        P = len(spec["means"][0])
        st = SETTINGS[name]
        for k in ("weights", "means", "covs"):
            out[f"{name}/{k}"] = np.array(spec[k], np.float64)
        out[f"{name}/normalized"] = np.array(int(spec["normalized"]))
        torch.manual_seed(1400 + ord(name))
        theta0 = torch.tensor(spec["means"][0], dtype=F64) + 0.5 * torch.randn(P, dtype=F64)
        groups = {}
        # ---- HMC / MALA / MH through make_golden's run_trace
        s = HMC(model_of(spec), theta0=theta0.clone(), dataloader=loader, step=st["hmc"], num_steps=3, chain=ChainList())
        init = dict(init_target=mg.tnp(s.current["target_val"]), init_grad=mg.tnp(s.current["grad_val"]))
        groups["hmc"] = dict(mg.run_trace(s, data, N_ITER), step=np.array(st["hmc"]), L=np.array(3), **init)
        s = MALA(model_of(spec), theta0=theta0.clone(), dataloader=loader, step=st["mala"], chain=ChainList())
        init = dict(init_target=mg.tnp(s.current["target_val"]), init_grad=mg.tnp(s.current["grad_val"]))
        groups["mala"] = dict(mg.run_trace(s, data, N_ITER), step=np.array(st["mala"]), **init)
        s = MetropolisHastings(model_of(spec), theta0=theta0.clone(), dataloader=loader, chain=ChainList())
        s.kernel.set_density_params(theta0.clone(), scale=torch.full([P], st["mh"], dtype=F64))
        init_t = mg.tnp(s.current["target_val"])
        groups["mh"] = dict(mg.run_trace(s, data, N_ITER), scale=np.array(st["mh"]), init_target=init_t)
        # ---- RAM / AM
        s = RAM(model_of(spec), theta0=theta0.clone(), dataloader=loader, cov0=0.5 * torch.eye(P, dtype=F64))
        init_t = float(s.current["target_val"].detach())
        groups["ram"] = dict(adaptive_trace(s, x, y, P, False), init_target=np.array(init_t), cov0=mg.tnp(s.cov0),
                             a=np.array(s.a), g=np.array(s.g), chol=mg.tnp(s.chol_cov))
        eps, eye = 1e-6, torch.eye(P, dtype=F64)
        s = AM(model_of(spec), theta0=theta0.clone(), dataloader=loader, l=0.2, b=st["am_b"], c=st["am_c"], t0=5,
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
            print(f"g14 {name}/{g} acceptance {np.mean(rec['accepted']):.3f}")
            out[f"{name}/{g}/theta0"] = mg.tnp(theta0)
            for k, v in rec.items():
                out[f"{name}/{g}/{k}"] = np.asarray(v)
    path = os.path.join(mg.HERE, "g14_distribution_traces.npz")
    np.savez_compressed(path, **out)
    print("g14", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
