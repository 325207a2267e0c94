"""Elliptical slice sampling without a device: the numpy restatement (tests/eslice_restatement.py) held to the invariance
harness, the parity inputs of tests/eslice_cases.py, the word layout, the sampler's refusals and the C ABI's surface.

The invariance calibration follows tests/test_invariance_host.py: 4096 chains from exact draws, 8 iterations, 4 x 4096
reference draws, ``invariance.threshold`` over the z-scores this file asserts on.  Its target is the linear-Gaussian plan
of dims [3, 1] on TWO rows: four parameters, two of which the data leave to the prior, so a transition that counts the prior
twice, or scales it wrongly under a temperature, ends in another law (on the 50 and 70 rows of lin3 and lin12 the prior's
share of the posterior precision is 2e-3, and neither mutant would show)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import eslice_cases as ec
from tests import eslice_restatement as er
from tests import invariance as iv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_HOST, N_HOST = 4096, 8
SMALL = (3, 2)   # dims [3, 1] on two rows
HALVES = (1.0, 0.5)
THRESHOLD = iv.threshold(3 * iv.n_features(4))   # one group untempered, two under the halves


def _ensemble(target, groups, mutant=None, seed=3, chains=C_HOST):
    """(largest |z|, mean evaluations per draw, share of draws that moved) of N_HOST iterations from exact starts."""
    tgt = iv.linear_gaussian(*target)[2] if isinstance(target, tuple) else iv.target_of(target)
    rng = np.random.default_rng(seed)
    R = chains // len(groups)
    temps = None if groups == (1.0,) else np.repeat(groups, R)
    f, m, s = ec.batch_setup(target, temps, mutant)
    th = np.concatenate([iv.exact_draws(tgt, R, rng, t) for t in groups])
    ell, tv = f(th, np.arange(chains))
    evals = moved = 0.0
    for _ in range(N_HOST):
        z, u = rng.standard_normal(th.shape), rng.random((chains, er.words()))
        th, ell, tv, acc, ne = er.draw_batch(f, th, ell, tv, m, s, z, u)
        evals, moved = evals + ne.mean() / N_HOST, moved + acc.mean() / N_HOST
    logp = tv if temps is None else tv / temps
    z = np.stack([iv.z_scores(iv.features(th[k * R:(k + 1) * R], logp[k * R:(k + 1) * R]),
                              iv.reference_moments(tgt, 4 * chains, rng, t)) for k, t in enumerate(groups)])
    return float(np.abs(z).max()), evals, moved


# ------------------------------------------------------------------------------------------------ invariance calibration
@pytest.mark.parametrize("groups", [(1.0,), HALVES], ids=["t1", "halves"])
def test_restatement_leaves_the_posterior_invariant(groups):
    w, evals, moved = _ensemble(SMALL, groups)
    print(f"eslice restatement, {groups}: largest |z| {w:.2f}, threshold {THRESHOLD:.2f}, evals {evals:.2f}, moved {moved:.3f}")
    assert w < THRESHOLD and moved > 0.99, (w, moved)


@pytest.mark.parametrize("mutant,groups", [("whole_target", (1.0,)), ("untempered_scale", HALVES)])
def test_mutants_are_flagged(mutant, groups):
    """Slicing on the whole target under the prior counts the prior twice; sigma in place of sigma / sqrt(t) samples
    lik^t N(0, sigma^2) where the tempered posterior is lik^t N(0, sigma^2 / t).  Both beyond twice the threshold."""
    w, _, _ = _ensemble(SMALL, groups, mutant)
    print(f"eslice restatement, mutant {mutant}: largest |z| {w:.2f}, threshold {THRESHOLD:.2f}")
    assert w > 2 * THRESHOLD, w


@pytest.mark.parametrize("target,dtype,temp,base", ec.INVARIANCE, ids=[c[0] for c in ec.INVARIANCE])
def test_the_device_tests_setups_by_the_restatement(target, dtype, temp, base):
    """What tests/test_eslice_invariance_gpu.py relies on: the base factors give 1.5 to 8 evaluations per draw, the plans
    under their own prior the figures of ``PRIOR_EVALS``; every draw moves; the restatement itself stays below the
    threshold on these targets."""
    groups = HALVES if temp == "halves" else (1.0,)
    w, evals, moved = _ensemble(target, groups)
    print(f"eslice restatement, {target}: largest |z| {w:.2f}, evals {evals:.2f}, moved {moved:.3f}")
    assert w < iv.threshold(len(groups) * iv.n_features(iv.target_of(target).P)) and moved > 0.99
    if base:
        assert ec.EVALS_BAND[0] < evals < ec.EVALS_BAND[1], evals
    else:
        assert abs(evals - ec.PRIOR_EVALS[target]) < ec.EVALS_TOL and evals > ec.EVALS_BAND[1], evals


# ------------------------------------------------------------------------------------------------ the parity inputs
@pytest.fixture(scope="module")
def restated():
    return {name: ec.restate(name) for name in ec.CASES}


def test_parity_inputs_stay_clear_of_the_margin(restated):
    """At most 5 % of a case's (chain, draw) pairs are lost to a margin <= 1e-9, a chain followed to its first such draw."""
    for name, outs in restated.items():
        live, kept = np.ones(ec.C, bool), 0
        for o in outs:
            live &= o["margin"] > ec.MARGIN
            kept += int(live.sum())
        assert kept >= (1 - ec.MAX_UNDER) * ec.C * ec.DRAWS, (name, kept)


def test_parity_inputs_cover_every_path(restated):
    evals = np.concatenate([o["n_evals"] for outs in restated.values() for o in outs])
    assert (evals == 1).any() and (evals >= 4).any() and (evals >= 1).all()
    assert sum(int(o["neg"].sum()) for outs in restated.values() for o in outs) >= 1
    assert sum(int(o["pos"].sum()) for outs in restated.values() for o in outs) >= 1
    for name, outs in restated.items():
        ex = np.stack([o["exhausted"] for o in outs])
        acc = np.stack([o["accepted"] for o in outs])
        assert (ex == ~acc).all(), name   # from a finite start a chain stays only where its bracket is exhausted
        if ec.CASES[name].get("max_shrinks") == 2:
            ne = np.stack([o["n_evals"] for o in outs])
            assert 1 <= ex.sum() < ex.size // 2 and (ne[ex] == 3).all() and (ne <= 3).all(), (name, ex.sum())
            th0 = ec.inputs(name)["theta"]
            assert all(np.array_equal(outs[0]["theta"][c], th0[c]) for c in np.flatnonzero(ex[0]))
        else:
            assert not ex.any(), name


def test_batch_form_equals_the_chain_form():
    """``draw_batch`` (the calibration's) against ``draw`` (the parity's) on the linear-Gaussian case under temperatures."""
    name = "lin12/temp"
    d = ec.inputs(name)
    f, m, s = ec.batch_lin(ec.LIN, d["temps"])
    th, ell, tv = ec.start(name)
    for k, o in enumerate(ec.restate(name)):
        th, ell, tv, acc, ne = er.draw_batch(f, th, ell, tv, m, s, d["z"][k], d["u"][k])
        assert np.array_equal(acc, o["accepted"]) and np.array_equal(ne, o["n_evals"])
        np.testing.assert_allclose(th, o["theta"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(ell, o["ell"], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ the word layout
def test_word_layout_and_the_independence_of_max_shrinks():
    """Word 0 the height, 1 the first angle, 2 + k the k-th shrink, whatever the cap: a draw that ended within two shrinks
    is the same draw under max_shrinks 2 and 8; one that did not stays under 2 and goes on under 8."""
    assert er.words() == 2 + er.MAX_SHRINKS == 66 and er.words(2) == 4
    name = "xor/laplace/base"
    d = ec.inputs(name)
    fs, m, s = ec.chain_functions(name)
    th, ell, tv = ec.start(name)
    a = er.draw_chains(fs, th, ell, tv, m, s, d["z"][0], d["u"][0], 2)
    b = er.draw_chains(fs, th, ell, tv, m, s, d["z"][0], d["u"][0], 8)
    within = ~a["exhausted"]
    assert 3 <= within.sum() < ec.C
    for k in ("theta", "ell", "target", "accepted", "n_evals"):
        assert np.array_equal(a[k][within], b[k][within]), k
    assert (b["n_evals"][~within] > 3).all() and not a["accepted"][~within].any()
    # the words themselves: u_0 = 0 takes the first point; the first angle is u_1 turns; the first shrink reads word 2
    f, c = fs[0], 0
    u = d["u"][0][c].copy()
    u[0] = 0.0
    o = er.draw(f, th[c], ell[c], tv[c], m, s[c], d["z"][0][c], u)
    cs, sn = np.cos(2 * np.pi * u[1]), np.sin(2 * np.pi * u[1])
    assert o["n_evals"] == 1 and o["accepted"]
    np.testing.assert_allclose(o["theta"], m + (th[c] - m) * cs + s[c] * d["z"][0][c] * sn, rtol=0, atol=1e-14)
    u[0], u[1] = 0.5, 0.75             # the first point is made to miss: a = 0.75 >= 0 shrinks hi to a, the bracket
    trail = []                         # [a - 1, a] stays, and the next angle is lo + (hi - lo) u_2

    def g(t):
        trail.append(t.copy())
        e, tt = f(t)
        return (-np.inf if len(trail) == 1 else e), tt
    o = er.draw(g, th[c], ell[c], tv[c], m, s[c], d["z"][0][c], u)
    assert len(trail) == o["n_evals"] >= 2 and o["pos"] >= 1
    a2 = -0.25 + (0.75 + 0.25) * u[2]
    cs, sn = np.cos(2 * np.pi * a2), np.sin(2 * np.pi * a2)
    np.testing.assert_allclose(trail[1], m + (th[c] - m) * cs + s[c] * d["z"][0][c] * sn, rtol=0, atol=1e-13)
    # a chain whose carried ell is not finite stays put without evaluating
    o = er.draw(f, th[c], np.nan, tv[c], m, s[c], d["z"][0][c], d["u"][0][c])
    assert o["n_evals"] == 0 and not o["accepted"] and np.array_equal(o["theta"], th[c])


# ------------------------------------------------------------------------------------------------ refusals, the surface
def _model(dims=(2, 2, 1), prior=None):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=list(dims)), prior=prior)


def test_sampler_refusals_on_a_stub(monkeypatch):
    from torch.distributions import Laplace, Normal, StudentT
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.models import DistributionModel
    from eeyore_amd.models.targets import MultivariateNormal
    from eeyore_amd.samplers import EllipticalSlice, SingleChainSerialSampler
    dl = DataLoader(EmptyXYDataset())
    m = _model()
    P, C = m.num_params(), 4
    th0 = torch.zeros(C, P, dtype=m.dtype)
    monkeypatch.setattr(EllipticalSlice, "set_current", lambda self, theta, data=None: None)  # (no device here)
    assert issubclass(EllipticalSlice, SingleChainSerialSampler)
    assert EllipticalSlice.keys == ['sample', 'target_val', 'accepted', 'n_evals']
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="max_shrinks"):
            EllipticalSlice(m, theta0=th0, dataloader=dl, max_shrinks=bad)
    lap = _model(prior=Laplace(torch.zeros(P, dtype=m.dtype), torch.ones(P, dtype=m.dtype)))
    with pytest.raises(ValueError, match="must be an elementwise Normal"):
        EllipticalSlice(lap, theta0=th0, dataloader=dl)
    dist = DistributionModel(MultivariateNormal(np.zeros(3), np.eye(3)), 3)
    with pytest.raises(ValueError, match="nothing to slice under"):
        EllipticalSlice(dist, theta0=torch.zeros(C, 3, dtype=dist.dtype), dataloader=dl)
    one = torch.ones(P, dtype=m.dtype)
    with pytest.raises(ValueError, match="torch.distributions.Normal"):
        EllipticalSlice(m, theta0=th0, dataloader=dl, base=StudentT(3 * one, 0 * one, one))
    with pytest.raises(ValueError, match="one distribution per parameter"):
        EllipticalSlice(m, theta0=th0, dataloader=dl, base=Normal(torch.zeros(P + 1), torch.ones(P + 1)))
    for scale in (0 * one, -one, one * float("inf"), one * float("nan")):
        with pytest.raises(ValueError, match="positive and finite"):
            EllipticalSlice(m, theta0=th0, dataloader=dl, base=Normal(0 * one, scale, validate_args=False))
    with pytest.raises(ValueError, match="rng must be"):
        EllipticalSlice(m, theta0=th0, dataloader=dl, rng='numpy')
    s = EllipticalSlice(m, theta0=th0, dataloader=dl)
    assert s.max_shrinks == 64 and s.rng == 'philox' and s._base() == dict(base_loc=None, base_scale=None)
    s = EllipticalSlice(lap, theta0=th0, dataloader=dl, base=Normal(0.0, 2.0), max_shrinks=3, rng='torch')
    assert s.max_shrinks == 3 and torch.equal(s._base_scale, 2 * one) and torch.equal(s._base_loc, 0 * one)
    z, u = s._randoms(C, P)
    assert tuple(z.shape) == (C, P) and tuple(u.shape) == (C, 2 + 3)
    s = EllipticalSlice(dist, theta0=torch.zeros(C, 3, dtype=dist.dtype), dataloader=dl, base=Normal(torch.zeros(3), 1.5))
    assert tuple(s._base_scale.shape) == (3,) and s._base_scale.dtype == dist.dtype


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_eslice.h")).read()
    declared = set(re.findall(r"^int (ey_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.ESLICE_SYMBOLS) == {"ey_eslice_ell", "ey_eslice_step", "ey_eslice_run"}, declared
    assert not set(L.ESLICE_SYMBOLS) & (set(L.SYMBOLS) | set(L.EXT_SYMBOLS) | set(L.WARMUP_SYMBOLS) | set(L.NUTS_SYMBOLS))
    for inc in ("eeyore_amd.h", "eeyore_amd_ext.h", "eeyore_amd_warmup.h", "eeyore_amd_nuts.h"):
        assert f'#include "{inc}"' in hdr
    assert "#define EY_ESLICE_MAX_SHRINKS 64" in hdr and L.EY_ESLICE_MAX_SHRINKS == er.MAX_SHRINKS == 64
    lib = L.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for name, (res, args) in L.ESLICE_SYMBOLS.items():
        assert f" T {name}\n" in exported, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        proto = hdr[hdr.index("int " + name + "("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == len(args), name
    # the run is ey_mh_run's arguments with ell, the base and max_shrinks for the scale, and n_evals and its record
    # before the stream; the step takes ey_mh_step's (z, u) and the table's width
    mrun, run, step = L.SYMBOLS["ey_mh_run"][1], L.ESLICE_SYMBOLS["ey_eslice_run"][1], L.ESLICE_SYMBOLS["ey_eslice_step"][1]
    assert list(run[7:-3]) == list(mrun[4:-1]) and len(run) == len(mrun) + 5
    assert list(step[10:16]) == list(L._DRAW) and len(step) == 19
    # the plan's methods take what the entry points do
    from eeyore_amd.plan import Plan
    for name in ("eslice_ell", "eslice_step", "eslice_run"):
        assert callable(getattr(Plan, name))
