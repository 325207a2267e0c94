#!/usr/bin/env python3
"""Generate tests/golden/g15_mmd.npz by running the REFERENCE's eeyore.stats.discrepancy.squared_mmd / mmd and its
Kernel.K / symm_K / sum_K / sum_symm_K (eeyore/kernels/kernel.py: one Python call of k per pair) in f64.  Run from the
repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mmd.py

Samples are seeded normals, x2 shifted and widened against x1, rounded to f32-representable values before use, so the one
fixture serves f32 and f64 inputs.  Three shapes (n1, n2, p), six kernels (three with parameters, the three defaults), and
per shape the prefixes min(n, n1) of x1 for n in PREFIXES, each against the same prefix of x2 capped at n2 ("c") and against
all of x2 ("a").  Per shape s and kernel name kn, under s<s>/<kn>/:

    K [3, n2], symm_K [3, n1]    the first three rows of Kernel.K(x1, x2) and Kernel.symm_K(x1)
    sum11_d1 / sum11_d0 [5]      sum_symm_K(x1[:n]) with / without the diagonal
    sum22c_d1 / sum22c_d0 [5]    sum_symm_K(x2[:min(n, n2)]);   sum22a_d1 / sum22a_d0: of all of x2 (scalars)
    sum12c / sum12a [5]          sum_K(x1[:n], x2[:min(n, n2)]) / sum_K(x1[:n], x2)
    sqmmd_b1_c, sqmmd_b0_c, sqmmd_b1_a, sqmmd_b0_a [5]   squared_mmd, biased / unbiased, capped / all
    mmd_c, mmd_a [5]

and once: s<s>/x1, s<s>/x2, s<s>/prefix1, s<s>/prefix2c, kernels/<kn> = (kind, scale, l, third parameter or NaN).
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (registers the kanga stand-in and puts the reference on sys.path)

import torch  # noqa: E402

from eeyore.kernels import IsoSEKernel, PeriodicKernel, RQKernel  # noqa: E402
from eeyore.stats.discrepancy import mmd, squared_mmd  # noqa: E402

SHAPES = [(37, 29, 1), (37, 29, 3), (19, 17, 70)]
PREFIXES = [2, 5, 16, 17, 37]
ROWS = 3   # rows of K and symm_K that are kept (the sums cover every pair)
KERNELS = {
    "isose": (0, IsoSEKernel(0.7, 1.3), (0.7, 1.3, np.nan)),
    "rq": (1, RQKernel(1.2, 0.8, 1.5), (1.2, 0.8, 1.5)),
    "periodic": (2, PeriodicKernel(0.9, 1.1, 2.5), (0.9, 1.1, 2.5)),
    "isose_default": (0, IsoSEKernel(), (1.0, 1.0, np.nan)),
    "rq_default": (1, RQKernel(), (1.0, 1.0, 1.0)),
    "periodic_default": (2, PeriodicKernel(), (1.0, 1.0, 2.0)),
}


def main():
    torch.set_num_threads(1)
    out = {}
    for kn, (kind, _, par) in KERNELS.items():
        out[f"kernels/{kn}"] = np.array((kind,) + par, np.float64)
    for s, (n1, n2, p) in enumerate(SHAPES):
        rng = np.random.default_rng(1500 + s)
        x1 = rng.standard_normal((n1, p)).astype(np.float32).astype(np.float64)
        x2 = (0.4 + 1.25 * rng.standard_normal((n2, p))).astype(np.float32).astype(np.float64)
        pre1 = [min(n, n1) for n in PREFIXES]
        pre2 = [min(n, n2) for n in PREFIXES]
        out[f"s{s}/x1"], out[f"s{s}/x2"] = x1, x2
        out[f"s{s}/prefix1"], out[f"s{s}/prefix2c"] = np.array(pre1), np.array(pre2)
        l1 = [torch.tensor(r, dtype=torch.float64) for r in x1]   # lists of [p] tensors, as the reference's callers pass
        l2 = [torch.tensor(r, dtype=torch.float64) for r in x2]
        for kn, (_, ker, _) in KERNELS.items():
            g = f"s{s}/{kn}/"
            out[g + "K"] = mg.tnp(ker.K(l1[:ROWS], l2))
            out[g + "symm_K"] = mg.tnp(ker.symm_K(l1))[:ROWS]
            for d in (1, 0):
                out[g + f"sum11_d{d}"] = np.array([ker.sum_symm_K(l1[:a], include_diag=bool(d)).item() for a in pre1])
                out[g + f"sum22c_d{d}"] = np.array([ker.sum_symm_K(l2[:b], include_diag=bool(d)).item() for b in pre2])
                out[g + f"sum22a_d{d}"] = np.array(ker.sum_symm_K(l2, include_diag=bool(d)).item())
            out[g + "sum12c"] = np.array([ker.sum_K(l1[:a], l2[:b]).item() for a, b in zip(pre1, pre2)])
            out[g + "sum12a"] = np.array([ker.sum_K(l1[:a], l2).item() for a in pre1])
            for b in (1, 0):
                out[g + f"sqmmd_b{b}_c"] = np.array([squared_mmd(l1[:a], l2[:c], ker, biased=bool(b)).item()
                                                     for a, c in zip(pre1, pre2)])
                out[g + f"sqmmd_b{b}_a"] = np.array([squared_mmd(l1[:a], l2, ker, biased=bool(b)).item() for a in pre1])
            out[g + "mmd_c"] = np.array([mmd(l1[:a], l2[:c], ker).item() for a, c in zip(pre1, pre2)])
            out[g + "mmd_a"] = np.array([mmd(l1[:a], l2, ker).item() for a in pre1])
            print(f"g15 s{s} {kn}: mmd {out[g + 'mmd_a'][-1]:.6f}")
    path = os.path.join(mg.HERE, "g15_mmd.npz")
    np.savez_compressed(path, **out)
    print("g15", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
