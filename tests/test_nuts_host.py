"""NUTS without a device: the numpy restatement (tests/nuts_restatement.py) held to the invariance harness and to its own
iterative form, the word layout, the parity inputs of tests/nuts_cases.py, the sampler's refusals and the C ABI's surface.

The invariance case: 4096 chains from exact draws of the P = 2 mixture of tests/invariance.py, 8 iterations, max_depth 5,
identity metric, step 1.4 -- chosen on the CPU from the restatement alone as the step at which the mean accept statistic
is about 0.8 (the usual target of a step-size adaptation) and trees of depth 1, 2, 3 and 4 all occur.  The threshold is
``invariance.threshold`` for the z-scores this file asserts on (one set of features)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import invariance as iv
from tests import nuts_cases as nc
from tests import nuts_restatement as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS, ITERS, STEP, DEPTH_CAP = 4096, 8, 1.4, 5
TARGET = "mix2_2"
THRESHOLD = iv.threshold(iv.n_features(2))


def _ensemble(mutant, seed=7):
    """The final states of the invariance case, the depth histogram and the mean accept statistic."""
    tgt = iv.target_of(TARGET)
    f = nr.point_value_grad(tgt)
    rng = np.random.default_rng(seed)
    th = iv.exact_draws(tgt, CHAINS, rng)
    t, g = tgt.value_grad(th)
    mul, tmul = nr.metric_ops("diag", np.ones(tgt.P))
    depths, stat = np.zeros(nr.MAX_DEPTH + 1, int), 0.0
    for _ in range(ITERS):
        v0, u = rng.standard_normal((CHAINS, tgt.P)), rng.random((CHAINS, nr.words(DEPTH_CAP)))
        for c in range(CHAINS):
            o = nr.nuts_draw(f, th[c], t[c], g[c], v0[c], u[c], STEP, DEPTH_CAP, mul, tmul, mutant)
            th[c], t[c], g[c] = o["theta"], o["target"], o["grad"]
            depths[o["depth"]] += 1
            stat += o["accept_stat"]
    z = iv.z_scores(iv.features(th, t), iv.reference_moments(tgt, iv.N_REF, rng))
    return float(np.abs(z).max()), depths, stat / (CHAINS * ITERS)


def test_restatement_leaves_the_mixture_invariant():
    w, depths, stat = _ensemble(None)
    print(f"nuts restatement: largest |z| {w:.2f}, threshold {THRESHOLD:.2f}, depths {depths.tolist()}, accept_stat {stat:.3f}")
    assert all(depths[d] > 0 for d in (1, 2, 3, 4)), depths
    assert 0.6 < stat < 0.9, stat
    assert w < THRESHOLD, w


@pytest.mark.parametrize("mutant", ["leaf_unweighted", "top_always"])
def test_mutants_are_flagged(mutant):
    w, _, _ = _ensemble(mutant)
    print(f"nuts restatement, mutant {mutant}: largest |z| {w:.2f}, threshold {THRESHOLD:.2f}")
    assert w > THRESHOLD, w


def _seeded_draws(n=200):
    """n draws of single chains on the P = 5 mixture over a range of steps and both metric forms, by both forms of the tree."""
    tgt = iv.target_of("mix5_3")
    f = nr.point_value_grad(tgt)
    rng = np.random.default_rng(11)
    for k in range(n):
        kind = ("diag", "dense")[k % 2]
        table = 0.5 + rng.random(tgt.P) if kind == "diag" else iv.factors(1, tgt.P, rng, 1.0)[0]
        mul, tmul = nr.metric_ops(kind, table)
        th = iv.exact_draws(tgt, 1, rng)[0]
        t, g = f(th)
        args = (f, th, t, g, rng.standard_normal(tgt.P), rng.random(nr.words(6)), 0.05 * 1.8 ** (k % 8), 6, mul, tmul)
        yield nr.nuts_draw(*args), nr.nuts_draw_iterative(*args)


def test_iterative_checkpoints_equal_the_recursion_and_the_word_layout():
    stops, depths = set(), set()
    for a, b in _seeded_draws():
        for k in nr.OUTCOME + ("stop", "dir_words"):
            assert a[k] == b[k], (k, a[k], b[k])
        for k in nr.VALUES:
            assert np.array_equal(a[k], b[k]), k
        # one direction word per doubling begun: the doublings kept, and one more where the last subtree was discarded
        assert a["dir_words"] == a["depth"] + (a["stop"] in ("divergent", "subblock")), a
        if a["stop"] == "max_depth":
            assert a["dir_words"] == a["depth"] == 6
        assert a["n_leapfrog"] <= 2 ** a["dir_words"] - 1
        stops.add(a["stop"])
        depths.add(a["depth"])
    assert stops == {"max_depth", "divergent", "subblock", "tree"} and depths >= set(range(0, 7)), (stops, depths)


def test_word_layout_ignores_the_runtime_cap():
    """Raising max_depth moves no variate: a draw that ended below the smaller cap is the same draw."""
    n = 0
    for a, _ in _seeded_draws(60):
        pass
    tgt = iv.target_of("mix5_3")
    f = nr.point_value_grad(tgt)
    rng = np.random.default_rng(5)
    mul, tmul = nr.metric_ops("diag", np.ones(tgt.P))
    for k in range(40):
        th = iv.exact_draws(tgt, 1, rng)[0]
        t, g = f(th)
        args = (f, th, t, g, rng.standard_normal(tgt.P), rng.random(nr.words(7)), 0.6)
        a, b = nr.nuts_draw(*args, 5, mul, tmul), nr.nuts_draw(*args, 7, mul, tmul)
        if a["stop"] != "max_depth":
            n += 1
            assert all(np.array_equal(a[k], b[k]) for k in nr.OUTCOME + nr.VALUES)
    assert n >= 20


def test_parity_inputs_cover_every_outcome_and_stay_clear_of_the_margin():
    """What tests/test_nuts_gpu.py relies on, by the restatement alone: over the 11 chains x 4 draws of the cases every
    depth 0 ... 5 occurs, and each case has a divergent draw, one stopped by max_depth and one by a sub-block check; at
    most 5 % of a case's (chain, draw) pairs have a decision within the margin."""
    depths = set()
    for name in nc.CASES:
        outs = nc.restate(name)
        stops = {s for o in outs for s in o["stop"]}
        depths |= {int(d) for o in outs for d in o["depth"]}
        margin = np.stack([o["margin"] for o in outs])
        assert {"divergent", "max_depth", "subblock"} <= stops, (name, stops)
        assert any(o["divergent"].any() for o in outs), name
        assert (margin <= nc.MARGIN).mean() <= nc.MAX_UNDER, (name, margin.min())
    assert depths == set(range(0, nc.MAX_DEPTH + 1)), depths


def _model(dims=(2, 2, 1)):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=list(dims)))


def test_sampler_refusals_on_a_stub_plan(monkeypatch):
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.samplers import NUTS, DenseMetric, HMC
    from eeyore_amd.tuners import WindowedAdaptation
    dl = DataLoader(EmptyXYDataset())
    m = _model()
    P, C = m.num_params(), 4
    th0 = torch.zeros(C, P, dtype=m.dtype)
    monkeypatch.setattr(HMC, "set_current", lambda self, theta, data=None: None)  # (no device here)
    assert issubclass(NUTS, HMC)
    for bad in (0, 11, 2.5):
        with pytest.raises(ValueError, match="max_depth"):
            NUTS(m, theta0=th0, dataloader=dl, max_depth=bad)
    with pytest.raises(ValueError, match="init_step_mode='reference'"):
        NUTS(m, theta0=th0, dataloader=dl, init_step_mode='reference')
    with pytest.raises(ValueError, match="'diag' or 'dense'"):
        NUTS(m, theta0=th0, dataloader=dl, metric='full')
    big = _model((8, 14, 1))
    assert big.num_params() > 128
    with pytest.raises(ValueError, match="limited to 128 parameters"):
        NUTS(big, theta0=torch.zeros(C, big.num_params(), dtype=big.dtype), dataloader=dl)
    with pytest.raises(ValueError, match="rng='torch'"):
        NUTS(m, theta0=th0, dataloader=dl, tuner=WindowedAdaptation(num_steps=1), rng='torch')
    s = NUTS(m, theta0=th0, dataloader=dl)
    assert s._metric_form == 'diag' and torch.equal(s._metric, torch.ones(P, dtype=m.dtype))   # metric=None: the identity
    assert s.max_depth == 10 and s.num_steps is None and s.rng == 'philox'
    with pytest.raises(ValueError, match="leapfrog"):
        s.leapfrog(th0, th0, None, None)
    s = NUTS(m, theta0=th0, dataloader=dl, metric=DenseMetric(torch.eye(P, dtype=m.dtype)), max_depth=3,
             tuner=WindowedAdaptation(num_steps=1))
    assert s._metric_form == 'dense' and s.max_depth == 3 and callable(s._warmup_launch)
    v0, u = NUTS(m, theta0=th0, dataloader=dl, rng='torch', max_depth=4)._nuts_randoms(C, P)
    assert tuple(v0.shape) == (C, P) and tuple(u.shape) == (C, 21 + 2 ** 4)


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_nuts.h")).read()
    declared = set(re.findall(r"^int (ey_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.NUTS_SYMBOLS) == {"ey_nuts_step", "ey_nuts_run", "ey_nuts_warmup"}, declared
    assert not set(L.NUTS_SYMBOLS) & (set(L.SYMBOLS) | set(L.EXT_SYMBOLS) | set(L.WARMUP_SYMBOLS))
    for inc in ("eeyore_amd.h", "eeyore_amd_ext.h", "eeyore_amd_warmup.h"):
        assert f'#include "{inc}"' in hdr
    assert "#define EY_NUTS_MAX_DEPTH 10" in hdr and L.EY_NUTS_MAX_DEPTH == nr.MAX_DEPTH == 10
    lib = L.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for name, (res, args) in L.NUTS_SYMBOLS.items():
        assert f" T {name}\n" in exported, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        proto = hdr[hdr.index("int " + name + "("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == len(args), name
    # the run is ey_hmc_metric_run's arguments with the outputs and two records before the stream; the warm-up adds
    # ey_hmc_metric_warmup's eleven
    hrun, run, warm = (t[n][1] for t, n in ((L.EXT_SYMBOLS, "ey_hmc_metric_run"), (L.NUTS_SYMBOLS, "ey_nuts_run"),
                                              (L.NUTS_SYMBOLS, "ey_nuts_warmup")))
    assert list(run[:len(hrun) - 1]) == list(hrun[:-1]) and len(run) == len(hrun) + 7
    assert list(warm[:len(run) - 1]) == list(run[:-1]) and len(warm) == len(run) + 11
