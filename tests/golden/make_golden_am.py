#!/usr/bin/env python3
"""Generate tests/golden/g13_am_traces.npz by running the REFERENCE's adaptive Metropolis sampler
(eeyore/samplers/am.py) in the build container.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_am.py

It takes make_golden_ram.py's approach (make_golden.py's `kanga` stand-in and its recorder of torch.randn / torch.rand):
a trace is a pure function of the recorded draws.  All groups are f64 with transform = cov + eps I.  Per draw a group
stores the adaptation index n, the counter index idx, z [P], u_mix (NaN when the draw consumed no mixture uniform), u,
and the state after the draw; the lower triangles of cov and cov_sum (both symmetric), running_mean and num_accepted
after every 10th draw and after the last.

  a  LogisticRegression(4, bias), BCE, 40 synthetic rows, eps = 1e-6, b = 2.38 / sqrt(5), c = 0.3, 300 draws
  b  MLP(4-3-3) sigmoid / none, CE, iris, eps = 1e-6, b = 2.38 / sqrt(27), c = 0.1, 100 draws
  c  the model of (b), eps = 1e-4, b = 0.5, c = 0.1, t0 = 20, 100 draws
  d  the model of (a), 40 direct draw(x, y, offset=5) calls with the counter at 10, 11, ...

(The P = 27 groups are shortened from 300 draws to keep the file small.)
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)
from make_golden_ram import ACT, LIK, lr_data, lr_model  # noqa: E402

import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from eeyore.constants import loss_functions  # noqa: E402
from eeyore.models import mlp  # noqa: E402
from eeyore.samplers import AM  # noqa: E402


def trace(s, data, n_iter, offset, idx0):
    loader = DataLoader(data, batch_size=len(data))
    x, y = next(iter(loader))
    s.counter.idx = idx0
    P = s.model.num_params()
    rec = {k: [] for k in ("n", "idx", "z", "u_mix", "u", "sample", "target_val", "accepted", "cov", "running_mean",
                           "cov_sum", "num_accepted", "state_it")}
    with mg.Recorder() as r:
        for it in range(n_iter):
            n = s.counter.idx + 1 - offset
            nz, nu = len(r.z), len(r.u)
            s.draw(x, y, offset=offset)
            assert len(r.z) == nz + 1 and len(r.u) == nu + (2 if n > s.t0 else 1), (it, n)  # the two-uniform rule
            rec["n"].append(n)
            rec["idx"].append(s.counter.idx)
            rec["z"].append(r.z[-1].reshape(P))
            rec["u_mix"].append(r.u[-2].item() if n > s.t0 else np.nan)
            rec["u"].append(r.u[-1].item())
            rec["sample"].append(mg.tnp(s.current["sample"]))
            rec["target_val"].append(float(s.current["target_val"].detach()))
            rec["accepted"].append(int(s.current["accepted"]))
            if (it + 1) % 10 == 0 or it == n_iter - 1:
                rec["cov"].append(np.tril(mg.tnp(s.cov)))
                rec["running_mean"].append(mg.tnp(s.running_mean))
                rec["cov_sum"].append(np.tril(mg.tnp(s.cov_sum)))
                rec["num_accepted"].append(int(s.num_accepted))
                rec["state_it"].append(it)
            s.counter.increment_idx()
    return {k: np.array(v) for k, v in rec.items()}


def group(name, model, data, dims, acts, lik, n_iter, eps, b, c, l=0.05, t0=2, offset=0, idx0=0):
    torch.manual_seed(3)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, dtype=torch.float64), torch.ones(P, dtype=torch.float64))
    theta0 = model.prior.sample()
    eye = torch.eye(P, dtype=torch.float64)
    s = AM(model, theta0=theta0.clone(), dataloader=DataLoader(data, batch_size=len(data)), l=l, b=b, c=c, t0=t0,
           transform=lambda cov: cov + eps * eye)
    init_t = float(s.current["target_val"].detach())
    out = trace(s, data, n_iter, offset, idx0)
    after = out["n"] > t0
    iso = int((out["u_mix"][after] < l).sum())
    assert iso >= 3 and int(after.sum()) - iso >= 3, (name, iso, int(after.sum()))
    out.update(theta0=mg.tnp(theta0), init_target=np.array(init_t), cov0=mg.tnp(s.cov0), eps=np.array(eps),
               l=np.array(l), b=np.array(b), c=np.array(c), t0=np.array(t0), offset=np.array(offset),
               dims=np.array(dims), acts=np.array([ACT[a] for a in acts]), lik=np.array(LIK[lik]),
               x=data.x.numpy(), y=data.y.numpy(), prior_mu=np.zeros(P), prior_sigma=np.ones(P))
    ev = np.linalg.eigvalsh(out["cov"][-1], UPLO="L").min()
    print(f"g13 {name} P={P} draws={n_iter} acceptance {out['accepted'].mean():.3f} isotropic after t0 {iso} "
          f"min eig of the last cov {ev:.3g}")
    return {f"{name}/{k}": v for k, v in out.items()}


def main():
    torch.set_num_threads(1)
    d = mg.datasets(torch.float64)
    out = {}
    lr = ([4, 1], [torch.sigmoid], "binary_classification")
    out.update(group("a", lr_model(), lr_data(), *lr, 300, eps=1e-6, b=2.38 / np.sqrt(5), c=0.3))
    hp = mlp.Hyperparameters(dims=[4, 3, 3], bias=[True] * 2, activations=[torch.sigmoid, None])
    net = ([4, 3, 3], hp.activations, "multiclass_classification")
    m = mlp.MLP(loss=loss_functions["multiclass_classification"], hparams=hp, dtype=torch.float64)
    out.update(group("b", m, d["iris"], *net, 100, eps=1e-6, b=2.38 / np.sqrt(27), c=0.1))
    m = mlp.MLP(loss=loss_functions["multiclass_classification"], hparams=hp, dtype=torch.float64)
    out.update(group("c", m, d["iris"], *net, 100, eps=1e-4, b=0.5, c=0.1, t0=20))
    out.update(group("d", lr_model(), lr_data(), *lr, 40, eps=1e-6, b=2.38 / np.sqrt(5), c=0.3, l=0.2, offset=5,
                     idx0=10))
    path = os.path.join(mg.HERE, "g13_am_traces.npz")
    np.savez_compressed(path, **out)
    print("g13", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
