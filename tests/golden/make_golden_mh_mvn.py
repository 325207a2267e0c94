#!/usr/bin/env python3
"""Generate tests/golden/g16_mh_mvn_traces.npz by running the REFERENCE's MetropolisHastings sampler
(eeyore/samplers/metropolis_hastings.py) with its MultivariateNormalKernel proposal, in f64.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mh_mvn.py

It takes make_golden.py's approach and its helpers (the `kanga` stand-in, the recorder that wraps torch.rand).
MultivariateNormal.rsample draws through torch.distributions.multivariate_normal._standard_normal, which is
torch.empty(...).normal_() and which that recorder does not see: this script wraps that name for the duration of a trace
and records its z, so a trace is a pure function of the recorded (z, u).

  a  target `a` of g14 (make_golden_dist.py: P = 2, one normalised component), scale_tril = I as in the reference's
     example, 300 draws
  b  target `b` of g14 (P = 3, two unnormalised components), a dense factor, 300 draws
  c  MLP(2-3-2-1) sigmoid / tanh / sigmoid, BCE, xor, a dense factor, 120 draws (P = 20: the file stays small)
  d  LogisticRegression(4, bias), BCE, make_golden_ram.py's 40 synthetic rows, a dense factor, symmetric=False, 300 draws

Every group stores its target, theta0, the initial target, the factor L, the recorded z [n, P] / u [n] and the state after
every draw.  The script prints each group's acceptance rate and its smallest |log u - log_rate|: the seeds are chosen so
that it stays above 1e-9 (symmetric=False adds two proposal log-densities that cancel only up to round-off).
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
import make_golden_dist as mgd  # noqa: E402
import make_golden_ram as mgr  # noqa: E402

import torch  # noqa: E402
import torch.distributions.multivariate_normal as tmvn  # noqa: E402
from torch.distributions import Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.constants import loss_functions  # noqa: E402
from eeyore.datasets import EmptyXYDataset  # noqa: E402
from eeyore.kernels import MultivariateNormalKernel  # noqa: E402
from eeyore.models import mlp  # noqa: E402
from eeyore.samplers import MetropolisHastings  # noqa: E402

N_ITER = 300
F64 = torch.float64


def dense_factor(P, scale, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    return torch.tensor(scale * np.linalg.cholesky(A @ A.T + 0.5 * np.eye(P)), dtype=F64)


def trace(name, model, x, y, loader, theta0, L, symmetric, N_ITER=N_ITER):
    P = model.num_params()
    kernel = MultivariateNormalKernel(theta0.clone(), L.clone())
    s = MetropolisHastings(model, theta0=theta0.clone(), dataloader=loader, symmetric=symmetric, kernel=kernel,
                           chain=ChainList())
    init_t = float(s.current["target_val"].detach())
    rec = dict(sample=[], target_val=[], accepted=[])
    margins = []
    inner = tmvn._standard_normal
    with mg.Recorder() as r:
        def standard_normal(shape, dtype, device):
            v = inner(shape, dtype, device)
            r.z.append(v.clone().numpy())
            return v
        tmvn._standard_normal = standard_normal
        try:
            for it in range(N_ITER):
                before = float(s.current["target_val"].detach())
                prop_seen = len(r.z)
                s.draw(x, y)
                assert len(r.z) == prop_seen + 1 and len(r.u) == it + 1
                prop = s.current["sample"].detach() if s.current["accepted"] else None
                rec["sample"].append(mg.tnp(s.current["sample"]))
                rec["target_val"].append(float(s.current["target_val"].detach()))
                rec["accepted"].append(int(s.current["accepted"]))
                # the margin of the decision, from the proposal rebuilt out of the recorded z
                th_prev = theta0 if it == 0 else torch.tensor(rec["sample"][it - 1], dtype=F64)
                th_prop = th_prev + torch.tril(L) @ torch.tensor(r.z[-1].reshape(P), dtype=F64)
                if prop is not None:
                    assert torch.allclose(prop, th_prop, rtol=0, atol=1e-14)
                log_rate = float(model.log_target(th_prop.clone(), x, y).detach()) - before
                margins.append(abs(np.log(r.u[-1].item()) - log_rate))
                s.counter.increment_idx()
        finally:
            tmvn._standard_normal = inner
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(z=np.stack(r.z).reshape(N_ITER, P), u=np.array([v.item() for v in r.u]), theta0=mg.tnp(theta0),
               init_target=np.array(init_t), L=mg.tnp(L), symmetric=np.array(int(symmetric)))
    print(f"g16 {name} P={P} draws={N_ITER} acceptance {out['accepted'].mean():.3f} "
          f"smallest |log u - log_rate| {min(margins):.3e}")
    assert min(margins) > 1e-9 and 0 < out["accepted"].sum() < N_ITER
    return out


def main():
    torch.set_num_threads(1)
    out = {}

    def put(name, rec):
        out.update({f"{name}/{k}": np.asarray(v) for k, v in rec.items()})

    empty = EmptyXYDataset()
    eloader = DataLoader(empty)
    ex, ey = next(iter(eloader))
    for name, L in (("a", torch.eye(2, dtype=F64)), ("b", dense_factor(3, 1.2, 161))):
        spec = mgd.TARGETS[name]
        P = len(spec["means"][0])
        torch.manual_seed(1600 + ord(name))
        theta0 = torch.tensor(spec["means"][0], dtype=F64) + 0.5 * torch.randn(P, dtype=F64)
        rec = trace(name, mgd.model_of(spec), ex, ey, eloader, theta0, L, True)
        rec.update({k: np.array(spec[k], np.float64) for k in ("weights", "means", "covs")})
        rec["normalized"] = np.array(int(spec["normalized"]))
        put(name, rec)

    def mlp_group(name, model, data, dims, acts, lik, L, symmetric, n_iter=N_ITER):
        torch.manual_seed(1600 + ord(name))
        P = model.num_params()
        model.prior = Normal(torch.zeros(P, dtype=F64), torch.ones(P, dtype=F64))
        theta0 = model.prior.sample()
        loader = DataLoader(data, batch_size=len(data))
        x, y = next(iter(loader))
        rec = trace(name, model, x, y, loader, theta0, L, symmetric, n_iter)
        rec.update(dims=np.array(dims), acts=np.array([mgr.ACT[a] for a in acts]), lik=np.array(mgr.LIK[lik]),
                   x=data.x.numpy(), y=data.y.numpy(), prior_mu=np.zeros(P), prior_sigma=np.ones(P))
        put(name, rec)

    hp = mlp.Hyperparameters(dims=[2, 3, 2, 1], bias=[True] * 3, activations=[torch.sigmoid, torch.tanh, torch.sigmoid])
    m = mlp.MLP(loss=loss_functions["binary_classification"], hparams=hp, dtype=F64)
    mlp_group("c", m, mg.datasets(F64)["xor"], [2, 3, 2, 1], hp.activations, "binary_classification",
              dense_factor(m.num_params(), 0.6, 163), True, n_iter=120)
    mlp_group("d", mgr.lr_model(), mgr.lr_data(), [4, 1], [torch.sigmoid], "binary_classification",
              dense_factor(5, 0.5, 164), False)
    path = os.path.join(mg.HERE, "g16_mh_mvn_traces.npz")
    np.savez_compressed(path, **out)
    print("g16", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
