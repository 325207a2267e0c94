#!/usr/bin/env python3
"""Measure what tests/test_eslice_fused_gpu.py's tolerance TAU is set from.

E: the largest |ell_generic_f32 - ell_f64| over every point the f64 restatement evaluates in the N = 150 cases of
tests/eslice_fused_cases.py, with the GENERIC kernel's evaluation (k_eslice's, reached under EY_FORCE_GENERIC: see
``generic_ell_at`` of the test).  TAU = 8 E rounded up to one digit; it may not exceed 2e-2.  Beside it, per case: the fused
kernel's own largest |ell - ell_f64| on the same points (a finding if above TAU / 2), numpy's own f32 error, and the pairs
each case sets aside at TAU and at 2e-2."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import mlp_oracle as orc  # noqa: E402
from tests import eslice_fused_cases as fc  # noqa: E402
from tests import test_eslice_fused_gpu as tg  # noqa: E402


def main():
    E = fused = 0.0
    for name in fc.CASES:
        pl, dev, d, model = tg.plan_of(name), tg.device_args(name), fc.inputs(name), fc.model_of(name)
        fs = fc.chain_functions(name)[0]
        eg = ef = en = 0.0
        n = 0
        for o in fc.restate(name):
            pts, ch = tg._t(np.stack(o["points"])), np.array(o["point_chain"])
            temp = None if dev["temp"] is None else dev["temp"][torch.tensor(ch, device=tg.DEV)].contiguous()
            ell_g, _, at = tg.generic_ell_at(pl, pts, temp, dev["base"])
            want_g = np.array([fs[c](p)[0] for c, p in zip(ch, tg._np(at))])      # f64 at the point the kernel evaluated
            ell_f, _ = pl.eslice_ell(pts, temp=temp, **dev["base"])
            want_f = np.array([fs[c](p)[0] for c, p in zip(ch, tg._np(pts))])
            eg = max(eg, float(np.abs(tg._np(ell_g) - want_g).max()))
            ef = max(ef, float(np.abs(tg._np(ell_f) - want_f).max()))
            if d["base"] is None:   # numpy's own f32 evaluation of the likelihood
                spec = orc.Spec(model["dims"], model["acts"], model["lik"])
                for c, p, w in zip(ch, tg._np(pts), want_f):
                    t = None if d["temps"] is None else np.float32(d["temps"][c])
                    lik32 = orc.log_lik(spec, p.astype(np.float32), d["x"].astype(np.float32), d["y"].astype(np.float32), t)
                    en = max(en, abs(float(lik32) - w))
            n += len(ch)
        print(f"{name:18s} {n:4d} points: generic |ell - f64| {eg:.3g}, fused {ef:.3g}, numpy f32 {en:.3g}; "
              f"ell magnitude {np.abs(want_f).max():.4g}")
        if name in fc.N150:
            E, fused = max(E, eg), max(fused, ef)
    digit = 10.0 ** math.floor(math.log10(8 * E))
    tau = math.ceil(8 * E / digit - 1e-9) * digit
    print(f"E = {E:.3g} over the N = 150 cases; 8 E = {8 * E:.3g}; TAU = {tau:.1g} (limit {fc.ELL_MARGIN_MAX:g})")
    print(f"the fused kernel's largest error on those points: {fused:.3g} (TAU / 2 = {tau / 2:.3g})")
    for name in fc.CASES:
        print(f"{name:18s} pairs set aside at TAU: {fc.summary(name, tau)[0]} of {fc.PAIRS}; at {fc.ELL_MARGIN_MAX:g}: "
              f"{fc.summary(name)[0]}; stayed {fc.summary(name)[1]}; evaluations per draw {fc.summary(name)[2]:.2f}")


if __name__ == "__main__":
    main()
