"""The windowed warm-up of HMC under a metric, without a GPU: the numpy restatement (tests/hmc_warmup_restatement.py) against
the schedule's known answers, the product's schedule, ``from_samples`` (the class that defines the estimate) and the host
tuner's recurrence; the restated warm-up on an ill-conditioned Gaussian; the sampler's refusals; the C-ABI surface of
include/eeyore_amd_warmup.h."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from eeyore_amd.samplers import DenseMetric, DiagMetric
from eeyore_amd.tuners import WindowedAdaptation  # (every test of this file needs the feature: none runs without it)
from tests import hmc_warmup_restatement as R
from tests.hmc_metric_restatement import DIAG, TRIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64

# The scenario of the adaptation tests, here and on the device (tests/test_hmc_warmup_gpu.py): N(0, Sigma) in P = 8
# dimensions with condition number 1e3, 64 chains, 300 warm-up draws of 8 leapfrog steps, target acceptance 0.8.
ADAPT = dict(P=8, cond=1e3, C=64, n=300, num_steps=8, d=0.8)
# form -> seeds (of the target, the start and the restatement's random numbers) for which the restatement ends with
# cond(L^-1 Sigma L^-T) < 5, searched on the CPU with the test below
ADAPT_SEEDS = {TRIL: [0], DIAG: [0]}


def adapt_start(seed, C=ADAPT["C"], P=ADAPT["P"]):
    return 0.5 * np.random.default_rng(seed).standard_normal((C, P))


# ------------------------------------------------------------------------------------------------ the schedule
def test_windows_known_answers():
    assert [e for _, e in R.windows(1000)] == [100, 150, 250, 450, 950]
    assert [e for _, e in R.windows(300)] == [100, 150, 250]
    assert R.windows(100) == [(15, 90)]
    assert R.windows(19) == [] and R.windows(1000)[0] == (75, 100)
    tuner = WindowedAdaptation(num_steps=4)
    assert [e for _, e in tuner.windows(1000)] == [100, 150, 250, 450, 950]
    assert [e for _, e in tuner.windows(300)] == [100, 150, 250]
    assert tuner.windows(100) == [(15, 90)]


def test_windows_equal_the_restatement_for_every_length():
    tuner = WindowedAdaptation(num_steps=1)
    other = WindowedAdaptation(num_steps=1, init_buffer=10, term_buffer=7, base_window=3)
    for n in range(1, 1201):
        w = tuner.windows(n)
        assert w == R.windows(n), n
        assert other.windows(n) == R.windows(n, 10, 7, 3), n
        # contiguous, doubling until the stretched last one, inside the burn-in; the phases tile [0, n)
        for (s0, e0), (s1, e1) in zip(w, w[1:]):
            assert e0 == s1 and (e1 - s1 == 2 * (e0 - s0) or (s1, e1) == w[-1])
        assert all(0 <= s < e <= n for s, e in w)
        ph = tuner.phases(n)
        assert ph[0][0] == 0 and ph[-1][1] == n and all(a[1] == b[0] for a, b in zip(ph, ph[1:]))
        assert [(s, e) for s, e, adapts in ph if adapts] == w


# ------------------------------------------------------------------------------------------------ the estimate
@pytest.mark.parametrize("n,C,P", [(2, 1, 1), (5, 3, 2), (9, 11, 65)])
@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "per_chain"])
@pytest.mark.parametrize("form", [DIAG, TRIL], ids=["diag", "dense"])
def test_moments_give_the_estimate_of_from_samples(form, pooled, n, C, P):
    """The independent yardstick: DiagMetric / DenseMetric.from_samples define the estimate from the draws themselves."""
    rng = np.random.default_rng(n + 10 * C + P)
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    draws = rng.standard_normal((n, C, P)) @ A.T + rng.standard_normal((1, C, P))
    mean, M2 = R.welford_chains(draws, form)
    np.testing.assert_allclose(mean, draws.mean(0), rtol=1e-12, atol=1e-13)
    got = R.metric_from_moments(mean, M2, n, form, pooled)
    cls = DiagMetric if form == DIAG else DenseMetric
    want = cls.from_samples(torch.tensor(draws), per_chain=not pooled).table.numpy()
    assert got.shape == want.shape
    # rtol 1e-10, taken against the table's largest entry as well as each entry's own size: nine draws in 65 dimensions
    # give a covariance of rank 8 plus the shrinkage, and the entries of its factor pass through zero (measured: 1.3e-14
    # absolute on entries of 1e-8 beside a diagonal of order one)
    err = np.abs(got - want)
    print(f"largest error {err.max():.3e} of {np.abs(want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
    if form == TRIL:  # the strict upper triangle of M2 is never read
        dirty = M2 + np.triu(np.full((P, P), np.nan), 1)
        assert np.array_equal(R.metric_from_moments(mean, dirty, n, form, pooled), got)


def test_welford_continues_across_a_split():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((7, 5))
    for form in (DIAG, TRIL):
        whole = R.welford(x, form)
        first = R.welford(x[:4], form)
        both = R.welford(x[4:], form, mean=first[0], M2=first[1], count=4)
        assert np.array_equal(whole[0], both[0]) and np.array_equal(whole[1], both[1])
        d = x - x.mean(0)
        np.testing.assert_allclose(whole[1], (d * d).sum(0) if form == DIAG else d.T @ d, rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------------------------------------ dual averaging
def test_da_recurrence_is_the_host_tuners():
    from eeyore_amd.tuners import PerChainDATuner
    rng = np.random.default_rng(0)
    C, eub = 4, 0.25
    e0 = torch.tensor(0.02 + 0.1 * rng.random(C), dtype=F64)
    tuner = PerChainDATuner(e0, num_steps=3, d=0.7, eub=eub)
    states = [R.da_restart(float(e)) for e in e0]
    wa = WindowedAdaptation(num_steps=3, d=0.7, eub=eub)
    capped = 0
    for idx in range(12):
        rate = rng.random(C)
        rate[0] = np.nan if idx == 3 else rate[0]
        assert wa.coefficients(idx + 1) == tuner.coefficients(idx)
        step, _ = tuner.tune(torch.tensor(rate), idx, return_e=idx != 11)
        for c in range(C):
            states[c], s = R.da_update(states[c], idx + 1, rate[c], 0.7, np.log(eub), averaged=idx == 11)
            np.testing.assert_allclose(s, float(step[c]), rtol=1e-13)
            capped += idx != 11 and s == eub
        np.testing.assert_allclose([s[0] for s in states], tuner.barh.numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose([s[1] for s in states], tuner.logbare.numpy(), rtol=1e-13, atol=1e-15)
    assert capped > 0
    np.testing.assert_allclose(wa.restart(e0).numpy(), np.stack(states) * [0, 0, 1], rtol=1e-15)


# ------------------------------------------------------------------------------------------------ it adapts
@pytest.mark.parametrize("form", [TRIL, DIAG], ids=["dense", "diag"])
def test_restated_warm_up_whitens_an_ill_conditioned_gaussian(form):
    for seed in ADAPT_SEEDS[form]:
        Sigma, vg = R.gaussian_case(form, ADAPT["P"], ADAPT["cond"], seed)
        assert np.linalg.cond(Sigma) > 100
        th, steps, metric, rates = R.warm_up(vg, adapt_start(seed), form, ADAPT["n"], ADAPT["num_steps"], d=ADAPT["d"],
                                             seed=seed)
        cond = R.whitened_condition(Sigma, form, metric)
        print(f"form {form} seed {seed}: cond(Sigma) {np.linalg.cond(Sigma):.1f} -> {cond:.3f}, steps "
              f"{steps.min():.3f} .. {steps.max():.3f}, acceptance of the last 50 draws {rates[-50:].mean():.3f}")
        assert cond < 5
        assert np.isfinite(steps).all() and (steps > 0).all() and np.isfinite(th).all()


# ------------------------------------------------------------------------------------------------ the sampler
def _model(P_dims=(2, 2, 1)):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=list(P_dims)))


def test_sampler_refusals_each_with_its_message(monkeypatch):
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.samplers import HMC
    dl = DataLoader(EmptyXYDataset())
    m = _model()
    P, C = m.num_params(), 4
    th0 = torch.zeros(C, P, dtype=m.dtype)
    wa = lambda **kw: WindowedAdaptation(num_steps=3, **kw)  # noqa: E731
    monkeypatch.setattr(HMC, "set_current", lambda self, theta, data=None: None)  # (no device here)
    with pytest.raises(ValueError, match="one chain"):
        HMC(m, theta0=th0[0], dataloader=dl, metric='diag', tuner=wa())
    with pytest.raises(ValueError, match="one chain"):
        HMC(m, dataloader=dl, metric='diag', tuner=wa())
    with pytest.raises(ValueError, match="rng='torch'"):
        HMC(m, theta0=th0, dataloader=dl, metric='diag', tuner=wa(), rng='torch')
    with pytest.raises(ValueError, match="no metric given"):
        HMC(m, theta0=th0, dataloader=dl, tuner=wa())
    with pytest.raises(ValueError, match="per-chain temperature"):
        HMC(m, theta0=th0, dataloader=dl, metric='dense', tuner=wa(), temperature=torch.linspace(0.1, 1, C))
    with pytest.raises(ValueError, match="'diag' or 'dense'"):
        HMC(m, theta0=th0, dataloader=dl, metric='full', tuner=wa())
    # pooled=False takes the temperature vector; the shorthands are the identities of their forms
    s = HMC(m, theta0=th0, dataloader=dl, metric='dense', tuner=wa(pooled=False), temperature=torch.linspace(0.1, 1, C))
    assert s._metric_form == 'dense' and torch.equal(s._metric, torch.eye(P, dtype=m.dtype)) and s.num_steps == 3
    s = HMC(m, theta0=th0, dataloader=dl, metric='diag', tuner=wa())
    assert s._metric_form == 'diag' and torch.equal(s._metric, torch.ones(P, dtype=m.dtype))
    with pytest.raises(ValueError, match="verbose=True"):
        s.run(num_epochs=30, num_burnin_epochs=20, verbose=True)
    s._set_metric(DiagMetric(torch.ones(2, P)), index=[0, 1, 1, 0])
    with pytest.raises(ValueError, match="metric index table"):
        s.run(num_epochs=30, num_burnin_epochs=20)
    s._set_metric(DiagMetric(torch.ones(P)))
    s.counter.num_batches = 3
    with pytest.raises(ValueError, match="minibatches"):
        s.run(num_epochs=30, num_burnin_epochs=20)
    for bad in (dict(num_steps=0), dict(num_steps=2, d=1.0), dict(num_steps=2, base_window=0), dict(num_steps=2, eub=0.0)):
        with pytest.raises(ValueError, match="WindowedAdaptation"):
            WindowedAdaptation(**bad)


def test_init_step_per_chain_checks_its_momentum(monkeypatch):
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.samplers import HMC
    m = _model()
    monkeypatch.setattr(HMC, "set_current", lambda self, theta, data=None: None)
    s = HMC(m, theta0=torch.zeros(3, m.num_params(), dtype=m.dtype), dataloader=DataLoader(EmptyXYDataset()))
    monkeypatch.setattr(type(m), "_plan", lambda self, x, y: None)
    with pytest.raises(ValueError, match="momentum must be"):
        s.init_step_per_chain(torch.zeros(3, m.num_params(), dtype=m.dtype), momentum=torch.zeros(2, m.num_params()))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_warmup_header_declares_what_the_binding_holds_and_the_library_exports():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_warmup.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.WARMUP_SYMBOLS) == {"ey_hmc_metric_warmup", "ey_metric_from_moments"}, declared
    assert not set(L.WARMUP_SYMBOLS) & (set(L.SYMBOLS) | set(L.EXT_SYMBOLS))
    assert '#include "eeyore_amd.h"' in hdr
    lib = L.lib()
    for name, (res, args) in L.WARMUP_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        proto = hdr[hdr.index("int " + name + "("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == len(args), name
    # the warm-up call is the run's arguments with its own between `accepted` and the stream
    run, warm = L.EXT_SYMBOLS["ey_hmc_metric_run"][1], L.WARMUP_SYMBOLS["ey_hmc_metric_warmup"][1]
    assert list(warm[:len(run) - 1]) == list(run[:-1]) and len(warm) == len(run) + 11
    for word in ("only j <= i", "ey_plan_attach_da", "in index order", "left\n *    untouched"):
        assert word in hdr, word


def test_argument_errors_without_gpu():
    lib = L.lib()
    p = ct.c_void_p(8)
    nan = float("nan")
    assert lib.ey_hmc_metric_warmup(None, p, p, p, p, 0, 1, None, 0.1, None, 3, None, 1, 0, 0, 0, 0, 4, None, None, None,
                                    None, p, None, None, 0, 0.8, nan, 0, None, None, 0, None, None, None) == -1
    assert b"null plan" in lib.ey_last_error() and b"ey_hmc_metric_warmup" in lib.ey_last_error()
    mm = lambda *a: lib.ey_metric_from_moments(*a)  # noqa: E731
    assert mm(p, p, 1, 1, 3, 0, 1, 1, p, p, None) == -1  # C n < 2
    assert b"at least two draws" in lib.ey_last_error()
    assert mm(p, p, 1, 7, 3, 0, 0, 1, p, p, None) == -1  # per chain: n < 2 whatever C
    assert mm(p, p, 0, 7, 3, 0, 1, 1, p, p, None) == -1
    assert mm(p, p, 9, 3, 2, 2, 1, 1, p, p, None) == -1 and b"EY_METRIC_DIAG or EY_METRIC_TRIL" in lib.ey_last_error()
    assert mm(p, p, 9, 3, 2, 1, 1, 7, p, p, None) == -1 and b"dtype" in lib.ey_last_error()
    assert mm(None, p, 9, 3, 2, 1, 1, 1, p, p, None) == -1 and b"null argument" in lib.ey_last_error()
    assert mm(p, p, 9, 3, 2, 1, 1, 1, p, None, None) == -1
    assert mm(p, p, 9, 0, 2, 1, 1, 1, p, p, None) == -1
    assert mm(p, p, 9, 3, 129, 1, 1, 1, p, p, None) == -2 and b"128" in lib.ey_last_error()
