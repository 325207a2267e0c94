#!/usr/bin/env python3
"""Generate tests/golden/g12_gibbs_traces.npz by running the REFERENCE's Gibbs sampler (eeyore/samplers/gibbs.py) and
its MLP blocking methods (eeyore/models/mlp.py:56-103, eeyore/itertools/chunk_evenly.py) in the build container.  Run
from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gibbs.py

It takes make_golden.py's approach and its helpers (the `kanga` stand-in, the recorder that wraps torch.randn /
torch.rand / torch.normal): a trace is then a pure function of the recorded draws.  Trace groups, all f64:

  a  MLP(4-3-3) sigmoid / none, CE, iris, scalar scale, whole nodes
  b  MLP(2-3-2-1) sigmoid / tanh / sigmoid, BCE, xor, per-block scales, sub-block sizes [2, None, 3, 3, 2, None]
     (a node of layer 1 has 4 parameters: size 3 is chunk_evenly's uneven case, ONE chunk of 4; size 2 gives two)
  c  MLP(2-3-1) sigmoid / sigmoid, BCE, xor, bias = [False, True]
  d  MLP(1-2-1) sigmoid / sigmoid, BCE, a one-column data set: the dims[l] == 1 branch of annotated_par_block_indices

Each stores the spec, the data, the block table (blk_off, blk_idx, blk_scale per sub-step in visiting order), the
recorded z [n, P] (parameter i's normal at column i) and u [n, S], the state, target_val and flag vector after every
draw, and margin [n, S] = |log u - log_rate| per sub-step.  CONDITION ON THE INPUTS: the seed of a group is the first of
1000, 1001, ... for which the smallest margin of the whole trace is >= 1e-6; it is asserted and stored (min_margin,
seed), so an f64 replay may demand every decision equal.

Also: `blocking/<name>/...`: annotated_par_block_indices for every b and starting_par_block_indices for the
reference's three test models and more on which the reference's node numbering is right (no layer wider than all layers
before it together); `chunks/...`: chunk_evenly of range(L) for L = 1..12, n = 1..6, flattened.
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
from eeyore.itertools import chunk_evenly  # noqa: E402
from eeyore.models import mlp  # noqa: E402
from eeyore.samplers import Gibbs  # noqa: E402

ACT = {None: 0, torch.sigmoid: 1, torch.tanh: 2}
LIK = {"binary_classification": 0, "multiclass_classification": 1}
MIN_MARGIN = 1e-6


def make_model(dims, bias, acts, lik):
    hp = mlp.Hyperparameters(dims=dims, bias=bias, activations=acts)
    m = mlp.MLP(loss=loss_functions[lik], hparams=hp, dtype=torch.float64)
    P = m.num_params()
    m.prior = Normal(torch.zeros(P, dtype=torch.float64), torch.ones(P, dtype=torch.float64))
    return m


def one_column_data(n=24, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 1))
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-2.0 * x[:, 0]))).astype(np.float64)[:, None]
    return XYDataset(torch.tensor(x), torch.tensor(y))


def trace(seed, dims, bias, acts, lik, data, scales, sizes, n_iter):
    torch.manual_seed(seed)
    m = make_model(dims, bias, acts, lik)
    P = m.num_params()
    theta0 = m.prior.sample()
    loader = DataLoader(data, batch_size=len(data))
    x, y = next(iter(loader))
    s = Gibbs(m, theta0=theta0.clone(), dataloader=loader, scales=scales, node_subblock_size=sizes)
    blocks = s.get_blocks()
    sub = [idx for per in blocks for idx in per]
    sub_scale = [float(s.scales[b]) for b, per in enumerate(blocks) for _ in per]
    S = len(sub)
    off = np.cumsum([0] + [len(i) for i in sub]).astype(np.int32)
    init_t = float(s.current["target_val"].detach())
    rec = dict(sample=[], target_val=[], accepted=[], z=[], u=[], margin=[])
    for it in range(n_iter):
        t_before = float(s.current["target_val"].detach())
        with mg.Recorder() as r:
            s.draw(x, y)
        assert len(r.z) == len(r.u) == S and all(len(a) == len(i) for a, i in zip(r.z, sub))
        z = np.zeros(P)
        for a, i in zip(r.z, sub):
            z[i] = a
        u = np.array([v.item() for v in r.u])
        rec["z"].append(z)
        rec["u"].append(u)
        rec["sample"].append(mg.tnp(s.current["sample"]))
        rec["target_val"].append(float(s.current["target_val"].detach()))
        rec["accepted"].append(mg.tnp(s.current["accepted"]).astype(np.uint8))
        # the log-rates are not kept by the reference: re-derive them with its own model, carrying as it carries
        prop, tcur, mar = (rec["sample"][-2] if it else mg.tnp(theta0)).copy(), t_before, []
        cur = prop.copy()
        for k, i in enumerate(sub):
            prop[i] = prop[i] + sub_scale[k] * z[i]
            tv = float(m.log_target(torch.tensor(prop), x, y).detach())
            mar.append(abs(np.log(u[k]) - (tv - tcur)))
            if np.log(u[k]) < tv - tcur:
                cur[i], tcur = prop[i], tv
        assert np.array_equal(cur, rec["sample"][-1]) and tcur == rec["target_val"][-1]
        rec["margin"].append(np.array(mar))
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(dims=np.array(dims), bias=np.array([int(b) for b in bias]), acts=np.array([ACT[a] for a in acts]),
               lik=np.array(LIK[lik]), x=data.x.numpy(), y=data.y.numpy(), prior_mu=np.zeros(P), prior_sigma=np.ones(P),
               theta0=mg.tnp(theta0), init_target=np.array(init_t), blk_off=off,
               blk_idx=np.array([i for idx in sub for i in idx], np.int32), blk_scale=np.array(sub_scale),
               min_margin=np.array(out["margin"].min()), seed=np.array(seed))
    return out


def group(name, *args):
    for seed in range(1000, 1100):
        out = trace(seed, *args)
        if out["min_margin"] >= MIN_MARGIN:
            break
    assert out["min_margin"] >= MIN_MARGIN, name
    print(f"g12 {name} seed={seed} P={out['z'].shape[1]} S={out['u'].shape[1]} draws={len(out['u'])} "
          f"acceptance {out['accepted'].mean():.3f} min margin {float(out['min_margin']):.2e}")
    return {f"{name}/{k}": v for k, v in out.items()}


BLOCKING = {  # name: (dims, bias); the first three are the models of the reference's tests/test_gibbs_blocking.py
    "m2_3_1": ([2, 3, 1], [True, True]),
    "m4_3_3": ([4, 3, 3], [True, True]),
    "m2_3_2_1": ([2, 3, 2, 1], [True, True, True]),
    "m4_3_2_3": ([4, 3, 2, 3], [True, True, True]),
    "m1_2_1": ([1, 2, 1], [True, True]),
    "m2_3_1_nobias0": ([2, 3, 1], [False, True]),
    "m3_4_4_2_nobias1": ([3, 4, 4, 2], [True, False, True]),
    "m5_1_1": ([5, 1, 1], [True, True]),
}


def blocking_tables():
    out = {}
    for name, (dims, bias) in BLOCKING.items():
        m = make_model(dims, bias, [torch.sigmoid] * (len(dims) - 1), "binary_classification")
        rows = [m.annotated_par_block_indices(b) for b in range(m.num_par_blocks())]
        assert sorted(i for r in rows for i in r[0]) == list(range(m.num_params())), name  # the reference is right here
        out[f"blocking/{name}/dims"] = np.array(dims)
        out[f"blocking/{name}/bias"] = np.array([int(b) for b in bias])
        out[f"blocking/{name}/off"] = np.cumsum([0] + [len(r[0]) for r in rows])
        out[f"blocking/{name}/idx"] = np.array([i for r in rows for i in r[0]])
        out[f"blocking/{name}/layer_node"] = np.array([[r[1], r[2]] for r in rows])
        out[f"blocking/{name}/starts"] = np.array(m.starting_par_block_indices())
    return out


def chunk_pairs():
    rows = []  # (L, n, number of chunks, then the chunk lengths padded to 12)
    for L in range(1, 13):
        for n in range(1, 7):
            chunks = list(chunk_evenly(list(range(L)), n))
            flat = [i for c in chunks for i in c]
            assert flat == list(range(len(flat)))  # consecutive from 0: the lengths say everything
            rows.append([L, n, len(chunks)] + [len(c) for c in chunks] + [0] * (12 - len(chunks)))
    return {"chunks/table": np.array(rows, np.int16)}


def main():
    torch.set_num_threads(1)
    d = mg.datasets(torch.float64)
    sig, tanh = torch.sigmoid, torch.tanh
    out = {}
    out.update(group("a", [4, 3, 3], [True, True], [sig, None], "multiclass_classification", d["iris"], 0.2, None, 40))
    out.update(group("b", [2, 3, 2, 1], [True] * 3, [sig, tanh, sig], "binary_classification", d["xor"],
                     [0.5, 0.4, 0.6, 0.3, 0.7, 0.5], [2, None, 3, 3, 2, None], 60))
    out.update(group("c", [2, 3, 1], [False, True], [sig, sig], "binary_classification", d["xor"], 0.5, None, 40))
    out.update(group("d", [1, 2, 1], [True, True], [sig, sig], "binary_classification", one_column_data(),
                     [0.6, 0.4, 0.8], [None, 1, None], 40))
    out.update(blocking_tables())
    out.update(chunk_pairs())
    path = os.path.join(mg.HERE, "g12_gibbs_traces.npz")
    np.savez_compressed(path, **out)
    print("g12", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
