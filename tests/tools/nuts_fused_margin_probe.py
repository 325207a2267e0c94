#!/usr/bin/env python3
"""Measure what tests/test_nuts_fused_gpu.py's tolerances are set from.

Runs the PARENT's path -- flags EY_NUTS_TREE_DEVICE alone: k_nuts_ws on the generic f32 evaluation -- on every case of
tests/nuts_fused_cases.py, each draw started from the restatement's f32 state, and prints per quantity the largest error
against the f64 restatement: target, energy and accept_stat absolutely, theta and the gradient relative to the chain's
largest entry.  TAU of a quantity = 8 x that figure rounded up to one digit; the TAUs of target, energy and accept_stat may
not exceed MARGIN_FLOOR.  Beside them, per case, the same figures of the fused kernel (flags EY_NUTS_FUSED) and the pairs on
which each path's outcome differs from the restatement's."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import nuts_fused_cases as nf  # noqa: E402
from tests import test_nuts_fused_gpu as tg  # noqa: E402


def figures(name, flags):
    _, _, ref = nf.restate(name)
    got = tg.draws_on_device(name, flags)
    worst, differ = dict.fromkeys(tg.VALUES, 0.0), 0
    for o, g in zip(ref, got):
        same = np.ones(nf.C, bool)
        for key in tg.OUTCOME:
            same &= g[key] == o[key].astype(int)
        differ += int((~same).sum())
        if same.any():
            sel = {key: v[same] for key, v in g.items()}
            for key, e in tg.errors(sel, {key: o[key][same] for key in tg.VALUES}).items():
                worst[key] = max(worst[key], e)
    return worst, differ


def round_up(x):
    digit = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / digit - 1e-9) * digit


def main():
    E = dict.fromkeys(tg.VALUES, 0.0)
    for name in nf.CASES:
        parent, dp = figures(name, tg.DEVICE)
        fused, df = figures(name, tg.FUSED)
        scale = max(float(np.abs(o["target"]).max()) for o in nf.restate(name)[2])
        print(f"{name:16s} parent: " + ", ".join(f"{k} {parent[k]:.3g}" for k in tg.VALUES) + f"; outcomes differ on {dp} of {nf.PAIRS}")
        print(f"{'':16s} fused:  " + ", ".join(f"{k} {fused[k]:.3g}" for k in tg.VALUES) + f"; outcomes differ on {df} of {nf.PAIRS}"
              f"; target magnitude {scale:.4g}")
        for k in E:
            E[k] = max(E[k], parent[k])
    for k in tg.VALUES:
        print(f"{k:12s} E = {E[k]:.3g}; 8 E = {8 * E[k]:.3g}; TAU = {round_up(8 * E[k]):.1g}")
    worst = max(round_up(8 * E[k]) for k in ("target", "energy", "accept_stat"))
    print(f"largest TAU of target, energy, accept_stat: {worst:.1g} (MARGIN_FLOOR {nf.MARGIN_FLOOR:g}): "
          f"{'within' if worst <= nf.MARGIN_FLOOR else 'ABOVE'} the floor")


if __name__ == "__main__":
    main()
