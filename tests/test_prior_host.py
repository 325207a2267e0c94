"""Laplace, Student-t and Cauchy priors, the host side (no GPU): the mapping from torch.distributions objects to the tables
of ey_plan_set_prior_family (eeyore_amd/models/priors.py), the refusals, the library's new symbols, and the torch f64
restatement (tests/prior_restatement.py) against the reference's recorded values and traces (g18_prior_traces.npz)."""
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import (Cauchy, Independent, Laplace, MixtureSameFamily, MultivariateNormal, Normal, StudentT,
                                 Categorical, Uniform)

from eeyore_amd import _lib as L
from eeyore_amd.models.priors import prior_tables
from tests import prior_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
P = 7


def _tables(seed=0):
    rng = np.random.default_rng(seed)
    return (torch.tensor(rng.standard_normal(P)), torch.tensor(0.5 + rng.random(P)), torch.tensor(1.0 + 5 * rng.random(P)))


# ------------------------------------------------------------------------------------------------ priors.py
def test_the_four_classes_map_to_their_family_and_tables():
    loc, scale, df = _tables()
    for prior, family, want_df in ((Normal(loc, scale), L.EY_PRIOR_NORMAL, None),
                                   (Laplace(loc, scale), L.EY_PRIOR_LAPLACE, None),
                                   (StudentT(df, loc, scale), L.EY_PRIOR_STUDENT_T, df),
                                   (Cauchy(loc, scale), L.EY_PRIOR_STUDENT_T, torch.ones(P, dtype=F64))):
        fam, lo, sc, d = prior_tables(prior, P)
        assert fam == family, prior
        assert torch.equal(lo, loc) and torch.equal(sc, scale)
        assert (d is None) if want_df is None else torch.equal(d, want_df)
    assert (L.EY_PRIOR_NORMAL, L.EY_PRIOR_LAPLACE, L.EY_PRIOR_STUDENT_T) == (0, 1, 2)


def test_scalar_parameters_are_expanded():
    loc, _, _ = _tables()
    fam, lo, sc, d = prior_tables(Laplace(loc, 0.75), P)
    assert fam == L.EY_PRIOR_LAPLACE and tuple(sc.shape) == (P,) and bool((sc == 0.75).all()) and d is None
    fam, lo, sc, d = prior_tables(StudentT(3.0, loc, torch.tensor(2.0, dtype=F64)), P)
    assert tuple(d.shape) == (P,) and bool((d == 3.0).all()) and bool((sc == 2.0).all()) and torch.equal(lo, loc)
    fam, lo, sc, d = prior_tables(Cauchy(0.5, torch.ones(P, dtype=F64)), P)
    assert fam == L.EY_PRIOR_STUDENT_T and bool((lo == 0.5).all()) and bool((d == 1.0).all()) and tuple(d.shape) == (P,)


def _rejected():
    loc, scale, df = _tables()
    return {
        "Uniform": Uniform(loc - 1, loc + 1),
        "MultivariateNormal": MultivariateNormal(loc, torch.eye(P, dtype=F64)),
        "Independent": Independent(Normal(loc, scale), 1),
        "MixtureSameFamily": MixtureSameFamily(Categorical(torch.ones(P, 2)), Normal(torch.zeros(P, 2), torch.ones(P, 2))),
        "laplace_wrong_length": Laplace(loc[:-1], scale[:-1]),
        "studentt_2d": StudentT(df.reshape(1, P), loc.reshape(1, P), scale.reshape(1, P)),
        "cauchy_scalar": Cauchy(0.0, 1.0),
        "normal_wrong_length": Normal(torch.zeros(P + 1), torch.ones(P + 1)),
        "not_a_distribution": (loc, scale),
    }


@pytest.mark.parametrize("name", list(_rejected()))
def test_rejected_priors_raise_value_error_naming_the_accepted_classes(name):
    with pytest.raises(ValueError, match="Normal, Laplace, StudentT and Cauchy"):
        prior_tables(_rejected()[name], P)


def test_models_refuse_a_prior_without_a_kernel_before_touching_a_plan():
    """The model maps its prior before it uploads anything: with a plan already in place (a stand-in here, there is no
    GPU) a refused prior raises and the plan sees no call."""
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import logistic_regression, mlp

    class Seen:
        P, calls = 0, []

        def set_prior(self, *a):
            self.calls.append(("normal",) + a)

        def set_prior_family(self, *a):
            self.calls.append(a)

    m1 = mlp.MLP(loss_functions["multiclass_classification"], hparams=mlp.Hyperparameters([4, 3, 3], activations=[torch.sigmoid, None]))
    m2 = logistic_regression.LogisticRegression(loss_functions["binary_classification"],
                                                hparams=logistic_regression.Hyperparameters(input_size=4))
    for m in (m1, m2):
        n = m.num_params()
        seen = Seen()
        seen.P, seen.calls = n, []
        object.__setattr__(m, "_hip_plan", seen)
        m.prior = Uniform(-torch.ones(n, dtype=F64), torch.ones(n, dtype=F64))
        with pytest.raises(ValueError, match="Normal, Laplace, StudentT and Cauchy"):
            m._plan(None, None)
        assert seen.calls == []
        m.prior = Cauchy(torch.zeros(n, dtype=F64), 2.0)
        m._plan(None, None)
        assert len(seen.calls) == 1 and seen.calls[0][0] == L.EY_PRIOR_STUDENT_T and bool((seen.calls[0][3] == 1).all())
        m._plan(None, None)  # uploaded once
        assert len(seen.calls) == 1
        m.prior = Normal(torch.zeros(n, dtype=F64), torch.ones(n, dtype=F64))
        m._plan(None, None)
        assert seen.calls[1][0] == "normal"  # a Normal prior goes through set_prior, as it always has


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ey_plan_set_prior_family", "ey_plan_prior_family"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name), name
    assert len(L.SYMBOLS["ey_plan_set_prior_family"][1]) == 6
    for name, value in (("EY_PRIOR_NORMAL", 0), ("EY_PRIOR_LAPLACE", 1), ("EY_PRIOR_STUDENT_T", 2)):
        assert re.search(rf"\b{name} = {value}\b", hdr), name
    lib = L.lib()
    assert lib.ey_plan_prior_family(None) == L.EY_PRIOR_NORMAL
    assert lib.ey_plan_set_prior_family(None, L.EY_PRIOR_LAPLACE, None, None, None, None) == -1
    assert b"null argument" in lib.ey_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
G18 = pr.load_g18()
VALUE_GROUPS = sorted(k for k in G18 if k.startswith("values/"))
TRACE_GROUPS = sorted(k for k in G18 if k.startswith("trace/"))


def test_the_fixture_holds_what_it_should():
    assert len(VALUE_GROUPS) == 9 and TRACE_GROUPS == ["trace/cauchy", "trace/laplace", "trace/studentt"]
    for key in VALUE_GROUPS:
        rec = G18[key]
        n = pr.group_target(rec).P
        assert rec["theta"].shape == (4, n) and rec["grad"].shape == (4, n) and n in (27, 20, 5)
        for tab in ("loc", "scale") + (("df",) if rec["family"] == "studentt" else ()):
            assert len(set(rec[tab].tolist())) == n, (key, tab)  # a distinct entry for every parameter
    for key in TRACE_GROUPS:
        rec = G18[key]
        assert rec["z"].shape[0] == 60 and 0 < rec["accepted"].sum() < 60
    assert [G18[k]["sampler"] for k in TRACE_GROUPS] == ["mh", "hmc", "mala"]
    assert G18["trace/laplace"]["L"] == 5 and G18["trace/cauchy"]["scale_mh"] == 0.25
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "g18_prior_traces.npz"))
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g17_mala_mvn_traces.npz"))


@pytest.mark.parametrize("key", VALUE_GROUPS)
def test_restatement_reproduces_the_recorded_values(key):
    rec = G18[key]
    tgt = pr.group_target(rec)
    for i, th in enumerate(rec["theta"]):
        ll, lp, lt, g = tgt.parts(th)
        np.testing.assert_allclose(ll, rec["log_lik"][i], rtol=1e-12)
        np.testing.assert_allclose(lp, rec["log_prior"][i], rtol=1e-12)
        np.testing.assert_allclose(lt, rec["log_target"][i], rtol=1e-12)
        np.testing.assert_allclose(g, rec["grad"][i], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(tgt.log_prior(th), rec["log_prior"][i], rtol=1e-12)


@pytest.mark.parametrize("key", TRACE_GROUPS)
def test_restatement_replays_the_recorded_traces(key):
    rec = G18[key]
    out = pr.replay(rec)
    assert np.array_equal(out["accepted"], rec["accepted"])  # every decision
    assert out["margin"].min() > 1e-9
    np.testing.assert_allclose(out["sample"], rec["sample"], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(out["target_val"], rec["target_val"], rtol=1e-10, atol=1e-11)


def test_closed_forms_of_the_kernel_match_torch():
    """The formulas the kernel evaluates, written out in numpy f64 from the tables the library builds,
    against torch.distributions: const - sum |d| / b, and const - sum h log1p(d^2 w) with Cauchy as nu = 1; the gradients
    -sign(d) / b (0 at d = 0, what autograd gives) and -2 h d w / (1 + d^2 w)."""
    from math import lgamma
    rng = np.random.default_rng(5)
    n = 11
    loc, b, nu = rng.standard_normal(n), 0.3 + rng.random(n), 0.5 + 6 * rng.random(n)
    th = loc + rng.standard_normal(n) * np.array([1e-3, 1.0, 1e3] * 4)[:n]
    th[4] = loc[4]  # theta_i = loc_i exactly
    d = th - loc
    t = torch.tensor(th, requires_grad=True)
    lp = Laplace(torch.tensor(loc), torch.tensor(b)).log_prob(t).sum()
    g, = torch.autograd.grad(lp, t)
    np.testing.assert_allclose(np.sum(-np.log(2 * b)) - np.sum(np.abs(d) / b), float(lp.detach()), rtol=1e-14)
    np.testing.assert_allclose(-np.sign(d) / b, g.numpy(), rtol=1e-14)
    assert g[4] == 0.0
    for df in (nu, np.ones(n)):
        w, h = 1.0 / (df * b * b), 0.5 * (df + 1.0)
        c = sum(lgamma(0.5 * (v + 1)) - lgamma(0.5 * v) - 0.5 * np.log(v * np.pi) - np.log(s) for v, s in zip(df, b))
        dist = StudentT(torch.tensor(df), torch.tensor(loc), torch.tensor(b))
        t = torch.tensor(th, requires_grad=True)
        lp = dist.log_prob(t).sum()
        g, = torch.autograd.grad(lp, t)
        np.testing.assert_allclose(c - np.sum(h * np.log1p(d * d * w)), float(lp.detach()), rtol=1e-13)
        np.testing.assert_allclose(-2 * h * d * w / (1 + d * d * w), g.numpy(), rtol=1e-12, atol=1e-300)
    cp = Cauchy(torch.tensor(loc), torch.tensor(b)).log_prob(torch.tensor(th)).sum()
    np.testing.assert_allclose(float(lp.detach()), float(cp), rtol=1e-13)
    np.testing.assert_allclose(c, np.sum(-np.log(np.pi) - np.log(b)), rtol=1e-14)


@pytest.mark.parametrize("family", ["laplace", "studentt"])
@pytest.mark.parametrize("sampler", pr.OTHER_SAMPLERS)
def test_the_other_samplers_cases_stay_clear_of_the_decision_margin(sampler, family):
    """The inputs tests/test_prior_gpu.py feeds RAM, AM, Gibbs and the two factor proposals: by the restatements alone at
    most 1 of the 55 decisions of a sampler (Gibbs: of its 55 x 6 sub-steps) lies within 1e-9 of log u, and both decisions
    occur."""
    d = pr.other_case(sampler, family)
    assert int((d["margin"] <= 1e-9).sum()) <= 1
    assert 0 < d["accepted"].sum() < d["accepted"].size
    assert d["theta"].shape == (5, 11, 27) and np.isfinite(d["target"]).all()
    if sampler == "am":
        assert set(np.unique(d["branch"])) == {0, 1}  # the isotropic and the factor proposal
