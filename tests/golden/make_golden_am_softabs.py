#!/usr/bin/env python3
"""Generate tests/golden/g22_am_softabs_traces.npz by running the REFERENCE's adaptive Metropolis sampler
(eeyore/samplers/am.py) in f64 with transform = lambda c: softabs(c, 1000.) (eeyore/stats/metrics.py), the transform of
its own AM examples, in the build container.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_am_softabs.py

make_golden_am.py's approach and record (a trace is a pure function of the recorded torch.randn / torch.rand draws), with
the adaptation state -- the lower triangles of cov and cov_sum, running_mean, num_accepted -- after EVERY draw, so that a
test can replay each draw from the recorded state before it.

  a  the bivariate normal mixture of the reference's example (means -+2, unit covariances, not normalised), P = 2,
     l = 0.01, b = 2, c = 2, theta0 = 0, 200 draws
  b  LogisticRegression(4, bias), BCE, the 40 synthetic rows of g13 group a, b = 2.38 / sqrt(5), c = 0.3, 120 draws
  c  MLP(4-3-3) sigmoid / none, CE, iris, P = 27, b = 2.38 / sqrt(27), c = 0.1, 60 draws

No recorded draw has |log u - log_rate| < 1e-6 (asserted; the seed moves on otherwise): a replay has no near-tie to excuse.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # tests.softabs_restatement
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
from make_golden_ram import ACT, LIK, lr_data, lr_model  # noqa: E402

import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.constants import loss_functions  # noqa: E402
from eeyore.datasets import EmptyXYDataset  # noqa: E402
from eeyore.models import DistributionModel, mlp  # noqa: E402
from eeyore.samplers import AM  # noqa: E402
from eeyore.stats import softabs  # noqa: E402

from tests.softabs_restatement import replay  # noqa: E402

A = 1000.0
F64 = torch.float64
MIX = dict(weights=[1.0, 1.0], means=[[-2.0, -2.0], [2.0, 2.0]], covs=[np.eye(2).tolist()] * 2)


def trace(s, x, y, n_iter):
    P = s.model.num_params()
    il = np.tril_indices(P)
    rec = {k: [] for k in ("n", "idx", "z", "u_mix", "u", "sample", "target_val", "accepted", "cov", "running_mean",
                           "cov_sum", "num_accepted")}
    with mg.Recorder() as r:
        for it in range(n_iter):
            n = s.counter.idx + 1
            nz, nu = len(r.z), len(r.u)
            s.draw(x, y)
            assert len(r.z) == nz + 1 and len(r.u) == nu + (2 if n > s.t0 else 1), (it, n)
            rec["n"].append(n)
            rec["idx"].append(s.counter.idx)
            rec["z"].append(r.z[-1].reshape(P))
            rec["u_mix"].append(r.u[-2].item() if n > s.t0 else np.nan)
            rec["u"].append(r.u[-1].item())
            rec["sample"].append(mg.tnp(s.current["sample"]))
            rec["target_val"].append(float(s.current["target_val"].detach()))
            rec["accepted"].append(int(s.current["accepted"]))
            rec["cov"].append(mg.tnp(s.cov)[il])
            rec["running_mean"].append(mg.tnp(s.running_mean))
            rec["cov_sum"].append(mg.tnp(s.cov_sum)[il])
            rec["num_accepted"].append(int(s.num_accepted))
            s.counter.increment_idx()
    return {k: np.array(v) for k, v in rec.items()}


def group(name, make, n_iter, b, c, l, extra):
    for seed in range(3, 40):
        torch.manual_seed(seed)
        model, theta0, loader = make()
        x, y = next(iter(loader))
        s = AM(model, theta0=theta0.clone(), dataloader=loader, l=l, b=b, c=c, t0=2, transform=lambda cov: softabs(cov, A))
        init_t = float(s.current["target_val"].detach())
        out = trace(s, x, y, n_iter)
        # the reference does not keep a rejected proposal's target: the log-rates come from the restatement's replay
        full = dict(out, theta0=mg.tnp(theta0), init_target=np.array(init_t), cov0=mg.tnp(s.cov0), l=np.array(l),
                    b=np.array(b), c=np.array(c), t0=np.array(2), offset=np.array(0), a=np.array(A), **extra)
        margins = np.array([abs(np.log(out["u"][it]) - got["log_rate"]) for it, got, _ in replay(full)])
        if margins.min() >= 1e-6 and 0 < out["accepted"].sum() < n_iter:
            break
        print(f"g22 {name}: seed {seed} has a near-tie ({margins.min():.3g}) or a constant chain, moving on")
    else:
        raise SystemExit(f"g22 {name}: no seed without a near-tie")
    after = out["n"] > 2
    fact = int((~(out["u_mix"][after] < l)).sum())
    assert fact >= 3, (name, fact)
    out.update(theta0=mg.tnp(theta0), init_target=np.array(init_t), cov0=mg.tnp(s.cov0), a=np.array(A), l=np.array(l),
               b=np.array(b), c=np.array(c), t0=np.array(2), offset=np.array(0), seed=np.array(seed), **extra)
    ev = np.linalg.eigvalsh(mg.tnp(s.cov)).min()
    print(f"g22 {name} P={theta0.shape[0]} draws={n_iter} seed={seed} acceptance {out['accepted'].mean():.3f} factor draws "
          f"{fact} smallest margin {margins.min():.3g} min eig of the last cov {ev:.3g}")
    return {f"{name}/{k}": v for k, v in out.items()}


def mixture():
    means = [torch.tensor(m, dtype=F64) for m in MIX["means"]]

    def log_pdf(theta, x, y):
        return torch.log(torch.exp(-0.5 * torch.dot(theta - means[0], theta - means[0]))
                         + torch.exp(-0.5 * torch.dot(theta - means[1], theta - means[1])))
    return DistributionModel(log_pdf, 2, dtype=F64), torch.zeros(2, dtype=F64), DataLoader(EmptyXYDataset())


def net(model_of, data):
    def make():
        model = model_of()
        P = model.num_params()
        model.prior = Normal(torch.zeros(P, dtype=F64), torch.ones(P, dtype=F64))
        return model, model.prior.sample(), DataLoader(data, batch_size=len(data))
    return make


def net_extra(dims, acts, lik, data, P):
    return dict(dims=np.array(dims), acts=np.array([ACT[a] for a in acts]), lik=np.array(LIK[lik]), x=data.x.numpy(),
                y=data.y.numpy(), prior_mu=np.zeros(P), prior_sigma=np.ones(P))


def main():
    torch.set_num_threads(1)
    d = mg.datasets(F64)
    out = {}
    mix = dict(weights=np.array(MIX["weights"]), means=np.array(MIX["means"]), covs=np.array(MIX["covs"]),
               normalized=np.array(0))
    out.update(group("a", mixture, 200, b=2.0, c=2.0, l=0.01, extra=mix))
    out.update(group("b", net(lr_model, lr_data()), 120, b=2.38 / np.sqrt(5), c=0.3, l=0.05,
                     extra=net_extra([4, 1], [torch.sigmoid], "binary_classification", lr_data(), 5)))
    hp = mlp.Hyperparameters(dims=[4, 3, 3], bias=[True] * 2, activations=[torch.sigmoid, None])
    out.update(group("c", net(lambda: mlp.MLP(loss=loss_functions["multiclass_classification"], hparams=hp, dtype=F64),
                              d["iris"]), 60, b=2.38 / np.sqrt(27), c=0.1, l=0.05,
                     extra=net_extra([4, 3, 3], hp.activations, "multiclass_classification", d["iris"], 27)))
    path = os.path.join(mg.HERE, "g22_am_softabs_traces.npz")
    np.savez_compressed(path, **out)
    print("g22", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
