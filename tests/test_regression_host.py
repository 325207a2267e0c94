"""Regression likelihoods and network outputs, the host side (no GPU): the loss factories of eeyore_amd.constants against
torch.distributions, the refusals, the library's new symbols, the example, and the torch f64 restatement
(tests/regression_restatement.py) against the reference's recorded values and traces (g19_regression_traces.npz)."""
import ast
import ctypes as ct
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import Laplace, Normal, Poisson

from eeyore_amd import _lib as L
from eeyore_amd.constants import Loss, gaussian_loss, laplace_loss, loss_functions, poisson_loss
from tests import regression_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _out_y(seed=0, n=9, dk=2):
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.standard_normal((n, dk))), torch.tensor(rng.standard_normal((n, dk)))


# ------------------------------------------------------------------------------------------------ constants
@pytest.mark.parametrize("scale", [1.0, 0.35, 4.0])
def test_factories_evaluate_the_torch_distributions(scale):
    out, y = _out_y()
    g, lp = gaussian_loss(scale), laplace_loss(scale)
    assert (g.code, lp.code, g.scale, lp.scale) == (2, 3, scale, scale)
    np.testing.assert_allclose(float(g(out, y)), float(-Normal(out, scale).log_prob(y).sum()), rtol=1e-15)
    np.testing.assert_allclose(float(lp(out, y)), float(-Laplace(out, scale).log_prob(y).sum()), rtol=1e-15)
    # ... which are the closed forms of include/eeyore_amd.h
    r = (out - y).numpy()
    np.testing.assert_allclose(float(g(out, y)), -np.sum(-np.log(scale * np.sqrt(2 * np.pi)) - r * r / (2 * scale ** 2)),
                               rtol=1e-14)
    np.testing.assert_allclose(float(lp(out, y)), -np.sum(-np.log(2 * scale) - np.abs(r) / scale), rtol=1e-14)


def test_poisson_loss_is_the_log_density_up_to_the_factorial_term():
    out, _ = _out_y(1)
    counts = torch.tensor(np.random.default_rng(2).poisson(2.0, size=tuple(out.shape)).astype(np.float64))
    p = poisson_loss()
    assert p.code == 4 and p.scale is None
    want = torch.nn.PoissonNLLLoss(log_input=True, full=False, reduction='sum')(out, counts)
    np.testing.assert_allclose(float(p(out, counts)), float(want), rtol=1e-15)
    np.testing.assert_allclose(float(p(out, counts)), float(-(counts * out - out.exp()).sum()), rtol=1e-14)
    full = -Poisson(out.exp()).log_prob(counts).sum()  # the normalised density: differs by sum log(y!) alone
    np.testing.assert_allclose(float(full - p(out, counts)), float(torch.lgamma(counts + 1).sum()), rtol=1e-12)


def test_dict_entries_and_repr():
    assert set(loss_functions) == {'binary_classification', 'multiclass_classification', 'regression', 'robust_regression',
                                   'count_regression'}
    reg, rob, cnt = (loss_functions[k] for k in ('regression', 'robust_regression', 'count_regression'))
    assert (reg.code, reg.scale, rob.code, rob.scale, cnt.code, cnt.scale) == (2, 1.0, 3, 1.0, 4, None)
    assert (L.EY_LIK_GAUSS_SUM, L.EY_LIK_LAPLACE_SUM, L.EY_LIK_POISSON_SUM) == (2, 3, 4)
    out, y = _out_y(3)
    np.testing.assert_allclose(float(reg(out, y)), float(gaussian_loss()(out, y)), rtol=0)
    np.testing.assert_allclose(float(rob(out, y)), float(laplace_loss()(out, y)), rtol=0)
    assert repr(reg) == "Loss('regression', code=2, scale=1.0)"
    assert repr(laplace_loss(0.25)) == "Loss('robust_regression', code=3, scale=0.25)"
    assert repr(cnt) == "Loss('count_regression', code=4)"
    # the classification losses are what they were: no scale, the old repr
    assert repr(loss_functions['binary_classification']) == "Loss('binary_classification', code=0)"
    assert loss_functions['multiclass_classification'].scale is None
    assert Loss('x', 0, None).scale is None


@pytest.mark.parametrize("scale", [0.0, -1.0, float('inf'), float('nan')])
def test_a_scale_that_is_not_positive_and_finite_is_refused(scale):
    for factory in (gaussian_loss, laplace_loss):
        with pytest.raises(ValueError, match="finite and > 0"):
            factory(scale)


def test_logistic_regression_refuses_a_regression_loss():
    from eeyore_amd.models import logistic_regression as lr
    for loss in (loss_functions['regression'], laplace_loss(2.0), poisson_loss()):
        with pytest.raises(ValueError, match="regression loss"):
            lr.LogisticRegression(loss, hparams=lr.Hyperparameters(input_size=4))
    lr.LogisticRegression(loss_functions['binary_classification'], hparams=lr.Hyperparameters(input_size=4))


def test_mlp_hands_code_and_scale_to_its_plan(monkeypatch):
    """MLP creates its plan with the loss's code and sets the scale once (a stand-in plan: there is no GPU here)."""
    from eeyore_amd.models import mlp
    made = []

    class Seen:
        def __init__(self, dims, bias, acts, code, dtype, device):
            self.P, self.code, self.scales, self.priors = 13, code, [], 0
            made.append(self)

        def set_lik_scale(self, s):
            self.scales.append(s)

        def set_prior(self, *a):
            self.priors += 1

    monkeypatch.setattr(mlp, "Plan", Seen)
    hp = mlp.Hyperparameters([2, 3, 1], activations=[torch.tanh, None])
    for loss, code, scales in ((gaussian_loss(0.7), 2, [0.7]), (loss_functions['robust_regression'], 3, [1.0]),
                               (poisson_loss(), 4, []), (loss_functions['binary_classification'], 0, [])):
        m = mlp.MLP(loss, hparams=hp)
        m._plan(None, None)
        m._plan(None, None)
        assert (made[-1].code, made[-1].scales, made[-1].priors) == (code, scales, 1), loss
    assert len(made) == 4
    with pytest.raises(ValueError, match="Gaussian, Laplace and Poisson"):
        mlp.MLP(lambda out, y: 0.0, hparams=hp)._plan(None, None)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ey_plan_set_lik_scale", "ey_plan_lik_scale", "ey_forward"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name), name
    assert L.SYMBOLS["ey_plan_set_lik_scale"] == (ct.c_int, [ct.c_void_p, ct.c_double])
    assert L.SYMBOLS["ey_plan_lik_scale"] == (ct.c_double, [ct.c_void_p])
    assert L.SYMBOLS["ey_forward"] == (ct.c_int, [ct.c_void_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_void_p])
    for name, value in (("EY_LIK_BCE_SUM", 0), ("EY_LIK_CE_SUM", 1), ("EY_LIK_GAUSS_SUM", 2), ("EY_LIK_LAPLACE_SUM", 3),
                        ("EY_LIK_POISSON_SUM", 4)):
        assert re.search(rf"\b{name} = {value}\b", hdr), name
    assert "up to a constant in y" in re.sub(r"[\s*]+", " ", hdr)  # the Poisson form's caveat
    lib = L.lib()
    assert lib.ey_plan_lik_scale(None) == 1.0
    assert lib.ey_plan_set_lik_scale(None, 1.0) == -1 and b"null plan" in lib.ey_last_error()
    assert lib.ey_forward(None, None, 1, None, None) == -1 and b"null plan" in lib.ey_last_error()


def test_the_example_imports_and_parses():
    path = os.path.join(ROOT, "examples", "sinusoid_regression_hmc.py")
    tree = ast.parse(open(path).read())
    assert "main" in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    spec = importlib.util.spec_from_file_location("sinusoid_regression_hmc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # imports the package; main() runs under __main__ only
    assert callable(mod.main) and mod.NOISE > 0


# ------------------------------------------------------------------------------------------------ the restatement
G19 = rr.load_g19()
VALUE_GROUPS = sorted(k for k in G19 if k.startswith("values/"))
TRACE_GROUPS = sorted(k for k in G19 if k.startswith("trace/"))


def test_the_fixture_holds_what_it_should():
    assert VALUE_GROUPS == [f"values/{loss}/{m}" for loss in sorted(rr.LOSSES) for m in ("mlp231", "mlp432")]
    assert TRACE_GROUPS == ["trace/gauss", "trace/laplace", "trace/poisson"]
    for key in VALUE_GROUPS:
        rec = G19[key]
        n = rr.group_target(rec).P
        assert rec["theta"].shape == (4, n) and rec["grad"].shape == (4, n) and n in (13, 23)
        assert rec["x"].shape == (40, rec["dims"][0]) and rec["y"].shape == (40, rec["dims"][-1])
        assert np.isfinite(rec["parts"]).all() and np.isfinite(rec["grad"]).all()
        if rec["loss"] == "poisson":  # counts
            assert np.array_equal(rec["y"], np.round(rec["y"])) and rec["y"].min() >= 0 and rec["y"].max() >= 2
    assert [G19[k]["sampler"] for k in TRACE_GROUPS] == ["hmc", "mala", "mh"]
    for key in TRACE_GROUPS:
        rec = G19[key]
        assert rec["z"].shape[0] == 60 and 0 < rec["accepted"].sum() < 60
    assert G19["trace/gauss"]["L"] == 5
    assert (G19["trace/gauss"]["lik_scale"], G19["trace/laplace"]["lik_scale"]) == (0.6, 0.8)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g19_regression_traces.npz")) <= 100 * 1024


@pytest.mark.parametrize("key", VALUE_GROUPS)
def test_restatement_reproduces_the_recorded_values(key):
    rec = G19[key]
    tgt = rr.group_target(rec)
    for i, th in enumerate(rec["theta"]):
        ll, lp, lt, g = tgt.parts(th)
        np.testing.assert_allclose(ll, rec["log_lik"][i], rtol=1e-12)
        np.testing.assert_allclose(lp, rec["log_prior"][i], rtol=1e-12)
        np.testing.assert_allclose(lt, rec["log_target"][i], rtol=1e-12)
        np.testing.assert_allclose(g, rec["grad"][i], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(tgt.rows(th).sum(), rec["log_lik"][i], rtol=1e-12)  # the row terms add up to it


@pytest.mark.parametrize("key", TRACE_GROUPS)
def test_restatement_replays_the_recorded_traces(key):
    rec = G19[key]
    out = rr.replay(rec)
    assert np.array_equal(out["accepted"], rec["accepted"])  # every decision
    assert out["margin"].min() > 1e-9
    np.testing.assert_allclose(out["sample"], rec["sample"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["target_val"], rec["target_val"], rtol=1e-12, atol=1e-12)


def test_closed_forms_of_the_kernels_match_autograd():
    """The output deltas the kernels use, written out in numpy from the constants the library builds, against
    autograd through the reference-side losses: -r / s^2, -sign(r) / s with sign(0) = 0, and y - exp(out)."""
    out, y = _out_y(4)
    y[2, 0] = out[2, 0]  # r = 0 exactly
    s = 0.7
    r = (out - y).numpy()
    for name, want in (("gauss", -r / s ** 2), ("laplace", -np.sign(r) / s), ("poisson", (y - out.exp()).numpy())):
        o = out.clone().requires_grad_(True)
        g, = torch.autograd.grad(-rr.loss_fn(name, s)(o, y), o)
        np.testing.assert_allclose(g.numpy(), want, rtol=1e-14, atol=0)
        if name == "laplace":
            assert g[2, 0] == 0.0


@pytest.mark.parametrize("sampler", rr.SAMPLERS)
def test_the_sampler_cases_stay_clear_of_the_decision_margin(sampler):
    """The inputs tests/test_regression_gpu.py feeds every sampler: by the restatements alone at most 1 of a sampler's 55
    decisions (Gibbs: of its 55 x 4 sub-steps) lies within 1e-9 of log u, and both decisions occur."""
    d = rr.sampler_case(sampler)
    assert int((d["margin"] <= 1e-9).sum()) <= 1
    assert 0 < d["accepted"].sum() < d["accepted"].size
    assert d["theta"].shape == (5, 11, 13) and np.isfinite(d["target"]).all()


def test_the_closed_form_case_is_what_the_gpu_test_assumes():
    """The conjugate posterior of the one-layer Gaussian plan, checked against the restated target (its Hessian is minus the
    precision, its gradient vanishes at the mean), and the restated HMC's acceptance at the step the GPU test uses."""
    x, y, mean, cov = rr.linear_gaussian()
    tgt = rr.Target([3, 1], [0], "gauss", x, y, scale=0.7, sigma=2.0)
    assert tgt.P == 4
    _, g = tgt.value_and_grad(mean)
    np.testing.assert_allclose(g, 0.0, atol=1e-10)
    d = np.array([0.3, -0.2, 0.1, 0.4])
    t0, tp = tgt.log_target(mean), tgt.log_target(mean + d)
    np.testing.assert_allclose(tp - t0, -0.5 * d @ np.linalg.inv(cov) @ d, rtol=1e-10)
    rate = rr.hmc_acceptance(tgt, rr.CLOSED_FORM_STEP, rr.CLOSED_FORM_L)
    print("restated HMC acceptance on the closed-form target:", rate)
    assert 0.6 <= rate <= 0.95
