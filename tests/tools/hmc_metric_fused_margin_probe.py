#!/usr/bin/env python3
"""Measure what tests/test_hmc_metric_fused_gpu.py's tolerances are set from.

Runs the PARENT's path -- hmc_metric_step without EY_HMC_METRIC_FUSED: k_hmc_metric on the generic f32 evaluation -- on every
case of tests/hmc_metric_fused_cases.py, each draw started from the restatement's f32 state, and prints per quantity the largest
error against the f64 restatement: target, H_cur, H_prop and the rate absolutely (H_prop and the rate over the pairs that are
not blown), theta and the gradient relative to the chain's largest entry.  TAU of a quantity = 8 x that figure rounded up to
one digit; the TAUs of target, H_cur and H_prop may not exceed MARGIN_FLOOR.  Beside them, per case, the same figures of the
fused kernel (the bit set) and the pairs on which each path's decision differs from the restatement's."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import hmc_metric_fused_cases as hc  # noqa: E402
from tests import test_hmc_metric_fused_gpu as tg  # noqa: E402


def figures(name, flags):
    _, _, ref = hc.restate(name)
    got = tg.draws_on_device(name, flags)
    worst, differ = dict.fromkeys(tg.VALUES, 0.0), 0
    for o, g in zip(ref, got):
        same = g["accepted"] == o["accepted"].astype(int)
        differ += int((~same).sum())
        if same.any():
            sel = {key: v[same] for key, v in g.items()}
            want = {key: o[key][same] for key in tg.VALUES}
            for key, e in tg.errors(sel, want, ~hc.blown(o)[same]).items():
                worst[key] = max(worst[key], e)
    return worst, differ


def round_up(x):
    digit = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / digit - 1e-9) * digit


def main():
    E = dict.fromkeys(tg.VALUES, 0.0)
    for name in hc.CASES:
        parent, dp = figures(name, tg.PARENT)
        fused, df = figures(name, tg.FUSED)
        scale = max(float(np.abs(o["target"]).max()) for o in hc.restate(name)[2])
        print(f"{name:16s} parent: " + ", ".join(f"{k} {parent[k]:.3g}" for k in tg.VALUES) + f"; decisions differ on {dp} of {hc.PAIRS}")
        print(f"{'':16s} fused:  " + ", ".join(f"{k} {fused[k]:.3g}" for k in tg.VALUES) + f"; decisions differ on {df} of {hc.PAIRS}"
              f"; target magnitude {scale:.4g}")
        for k in E:
            E[k] = max(E[k], parent[k])
    for k in tg.VALUES:
        print(f"{k:12s} E = {E[k]:.3g}; 8 E = {8 * E[k]:.3g}; TAU = {round_up(8 * E[k]):.1g}")
    worst = max(round_up(8 * E[k]) for k in ("target", "h_cur", "h_prop"))
    print(f"largest TAU of target, h_cur, h_prop: {worst:.1g} (MARGIN_FLOOR {hc.MARGIN_FLOOR:g}): "
          f"{'within' if worst <= hc.MARGIN_FLOOR else 'ABOVE'} the floor")


if __name__ == "__main__":
    main()
