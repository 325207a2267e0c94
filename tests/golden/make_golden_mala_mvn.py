#!/usr/bin/env python3
"""Generate tests/golden/g17_mala_mvn_traces.npz by running the REFERENCE's MALA sampler (eeyore/samplers/mala.py) with a
MultivariateNormalKernel proposal, in f64.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mala_mvn.py

It takes make_golden_mh_mvn.py's approach: make_golden.py's helpers (the `kanga` stand-in, the recorder that wraps
torch.rand) and a wrapper around torch.distributions.multivariate_normal._standard_normal, through which
MultivariateNormal.rsample draws, so a trace is a pure function of the recorded (z, u).

The reference's first draw samples around whatever `loc` the kernel was built with and re-centres only after a draw or in
`reset`; eeyore_amd always centres at kernel_mean(current).  Every trace therefore calls the reference's
`sampler.set_kernel(sampler.current)` once after construction.

  a  target `a` of g14 (make_golden_dist.py: P = 2, one normalised component), scale_tril = I, 140 draws
  b  target `b` of g14 (P = 3, two unnormalised components), a dense factor, 140 draws
  c  MLP(2-3-2-1) sigmoid / tanh / sigmoid, BCE, xor, a dense factor, 120 draws (P = 20: the file stays small)
  d  LogisticRegression(4, bias), BCE, make_golden_ram.py's 40 synthetic rows, a dense factor, 140 draws

Every group stores its target, theta0, the initial target and gradient, the factor L, the step, the recorded z [n, P] /
u [n] and the state after every draw (sample, target_val, grad_val, accepted).  The script prints each group's acceptance
rate and its smallest |log u - log_rate|: the seeds are chosen so that it stays above 1e-9.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
import make_golden_dist as mgd  # noqa: E402
import make_golden_ram as mgr  # noqa: E402
from make_golden_mh_mvn import dense_factor  # noqa: E402

import torch  # noqa: E402
import torch.distributions.multivariate_normal as tmvn  # noqa: E402
from torch.distributions import MultivariateNormal, Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.chains import ChainList  # noqa: E402
from eeyore.constants import loss_functions  # noqa: E402
from eeyore.datasets import EmptyXYDataset  # noqa: E402
from eeyore.kernels import MultivariateNormalKernel  # noqa: E402
from eeyore.models import mlp  # noqa: E402
from eeyore.samplers import MALA  # noqa: E402

N_ITER = 140
F64 = torch.float64


def trace(name, model, x, y, loader, theta0, L, step, n_iter=N_ITER):
    P = model.num_params()
    kernel = MultivariateNormalKernel(theta0.clone(), L.clone())
    s = MALA(model, theta0=theta0.clone(), dataloader=loader, step=step, kernel=kernel, chain=ChainList())
    s.set_kernel(s.current)
    init_t = float(s.current["target_val"].detach())
    init_g = mg.tnp(s.current["grad_val"])
    rec = dict(sample=[], target_val=[], grad_val=[], accepted=[])
    margins = []
    inner = tmvn._standard_normal
    with mg.Recorder() as r:
        def standard_normal(shape, dtype, device):
            v = inner(shape, dtype, device)
            r.z.append(v.clone().numpy())
            return v
        tmvn._standard_normal = standard_normal
        try:
            for it in range(n_iter):
                th = s.current["sample"].detach().clone()
                t = float(s.current["target_val"].detach())
                g = s.current["grad_val"].detach().clone()
                seen = len(r.z)
                s.draw(x, y)
                assert len(r.z) == seen + 1 and len(r.u) == it + 1
                rec["sample"].append(mg.tnp(s.current["sample"]))
                rec["target_val"].append(float(s.current["target_val"].detach()))
                rec["grad_val"].append(mg.tnp(s.current["grad_val"]))
                rec["accepted"].append(int(s.current["accepted"]))
                # the margin of the decision, from the proposal rebuilt out of the recorded z
                loc = th + 0.5 * step * g
                prop = loc + torch.tril(L) @ torch.tensor(r.z[-1].reshape(P), dtype=F64)
                if s.current["accepted"]:
                    assert torch.allclose(s.current["sample"].detach(), prop, rtol=0, atol=1e-14)
                tp, gp = model.upto_grad_log_target(prop.clone().detach(), x, y)
                loc2 = prop + 0.5 * step * gp.detach()
                log_rate = (float(tp.detach()) - t - float(MultivariateNormal(loc, scale_tril=L).log_prob(prop))
                            + float(MultivariateNormal(loc2, scale_tril=L).log_prob(th)))
                margins.append(abs(np.log(r.u[-1].item()) - log_rate))
                s.counter.increment_idx()
        finally:
            tmvn._standard_normal = inner
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(z=np.stack(r.z).reshape(n_iter, P), u=np.array([v.item() for v in r.u]), theta0=mg.tnp(theta0),
               init_target=np.array(init_t), init_grad=init_g, L=mg.tnp(L), step=np.array(float(step)))
    print(f"g17 {name} P={P} draws={n_iter} step={step} acceptance {out['accepted'].mean():.3f} "
          f"smallest |log u - log_rate| {min(margins):.3e}")
    assert min(margins) > 1e-9 and 0 < out["accepted"].sum() < n_iter
    return out


def main():
    torch.set_num_threads(1)
    out = {}

    def put(name, rec):
        out.update({f"{name}/{k}": np.asarray(v) for k, v in rec.items()})

    empty = EmptyXYDataset()
    eloader = DataLoader(empty)
    ex, ey = next(iter(eloader))
    for name, L, step in (("a", torch.eye(2, dtype=F64), 0.8), ("b", dense_factor(3, 1.2, 171), 0.5)):
        spec = mgd.TARGETS[name]
        P = len(spec["means"][0])
        torch.manual_seed(1700 + ord(name))
        theta0 = torch.tensor(spec["means"][0], dtype=F64) + 0.5 * torch.randn(P, dtype=F64)
        rec = trace(name, mgd.model_of(spec), ex, ey, eloader, theta0, L, step)
        rec.update({k: np.array(spec[k], np.float64) for k in ("weights", "means", "covs")})
        rec["normalized"] = np.array(int(spec["normalized"]))
        put(name, rec)

    def mlp_group(name, model, data, dims, acts, lik, L, step, n_iter=N_ITER):
        torch.manual_seed(1700 + ord(name))
        P = model.num_params()
        model.prior = Normal(torch.zeros(P, dtype=F64), torch.ones(P, dtype=F64))
        theta0 = model.prior.sample()
        loader = DataLoader(data, batch_size=len(data))
        x, y = next(iter(loader))
        rec = trace(name, model, x, y, loader, theta0, L, step, n_iter)
        rec.update(dims=np.array(dims), acts=np.array([mgr.ACT[a] for a in acts]), lik=np.array(mgr.LIK[lik]),
                   x=data.x.numpy(), y=data.y.numpy(), prior_mu=np.zeros(P), prior_sigma=np.ones(P))
        put(name, rec)

    hp = mlp.Hyperparameters(dims=[2, 3, 2, 1], bias=[True] * 3, activations=[torch.sigmoid, torch.tanh, torch.sigmoid])
    m = mlp.MLP(loss=loss_functions["binary_classification"], hparams=hp, dtype=F64)
    mlp_group("c", m, mg.datasets(F64)["xor"], [2, 3, 2, 1], hp.activations, "binary_classification",
              dense_factor(m.num_params(), 0.6, 173), 0.3, n_iter=120)
    mlp_group("d", mgr.lr_model(), mgr.lr_data(), [4, 1], [torch.sigmoid], "binary_classification",
              dense_factor(5, 0.5, 174), 0.1)
    path = os.path.join(mg.HERE, "g17_mala_mvn_traces.npz")
    np.savez_compressed(path, **out)
    print("g17", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
