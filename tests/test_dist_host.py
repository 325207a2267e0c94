"""DistributionModel without a GPU: the numpy restatement (tests/dist_restatement.py) against the reference's own traces
(tests/golden/g14_distribution_traces.npz) and against torch's MixtureSameFamily with autograd, the target objects' torch
call, the host-side validation of ey_plan_create_mixture, and the Python argument errors."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import dist_restatement as dr
from tests.am_restatement import am_draw
from tests.helpers import load
from tests.ram_restatement import ram_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("hmc", "mala", "mh", "ram", "am")


def g14():
    z = load("g14_distribution_traces.npz")
    out = {}
    for name in "ab":
        tgt = dict(weights=z[f"{name}/weights"], means=z[f"{name}/means"], covs=z[f"{name}/covs"],
                   normalized=bool(z[f"{name}/normalized"]))
        recs = {s: {k.split("/", 2)[2]: z[k] for k in z.files if k.startswith(f"{name}/{s}/")} for s in SAMPLERS}
        out[name] = (tgt, recs)
    return out


def replay(sampler, rec, vg, check):
    """Replay one g14 trace draw by draw with ``vg`` (theta -> (value, grad)) as the target; ``check(it, theta, target,
    accepted)`` compares the state after draw ``it``.  Used by the host test (restatement) and the GPU test's reference."""
    tf = lambda th: vg(th)[0]  # noqa: E731
    theta, target = rec["theta0"].copy(), float(rec["init_target"])
    n_it = rec["z"].shape[0]
    if sampler in ("hmc", "mala"):
        grad = rec["init_grad"].copy()
    if sampler == "ram":
        chol = np.linalg.cholesky(rec["cov0"])
    if sampler == "am":
        P = theta.shape[0]
        st = dict(theta=theta, target=target, mean=np.zeros(P), cov_sum=np.zeros((P, P)), cov=rec["cov0"].copy(),
                  num_accepted=0)
    for it in range(n_it):
        z, u = rec["z"][it], float(rec["u"][it])
        if sampler == "hmc":
            theta, target, grad, acc = dr.hmc_draw(vg, theta, target, grad, z, u, float(rec["step"]), int(rec["L"]))[:4]
        elif sampler == "mala":
            theta, target, grad, acc = dr.mala_draw(vg, theta, target, grad, z, u, float(rec["step"]))[:4]
        elif sampler == "mh":
            theta, target, acc = dr.mh_draw(tf, theta, target, z, u, float(rec["scale"]))[:3]
        elif sampler == "ram":
            theta, target, chol, acc = ram_draw(tf, theta, target, chol, z, u, int(rec["n"][it]), float(rec["a"]),
                                                float(rec["g"]))[:4]
        else:
            o = am_draw(tf, *(st[k] for k in ("theta", "target", "mean", "cov_sum", "cov", "num_accepted")), rec["cov0"],
                        z, rec["u_mix"][it], u, int(rec["idx"][it]), 0, l=float(rec["l"]), b=float(rec["b"]),
                        c=float(rec["c"]), t0=int(rec["t0"]), eps=float(rec["eps"]))
            assert o["branch"] != 2
            st = {k: o[k] for k in st}
            theta, target, acc = o["theta"], o["target"], o["accepted"]
        check(it, theta, target, acc)
    if sampler == "ram":
        return chol
    if sampler == "am":
        return st


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("name", list("ab"))
def test_restatement_reproduces_reference_traces(name, sampler):
    tgt, recs = g14()[name]
    rec = recs[sampler]
    vg = dr.mix_value_grad_fn(*dr.tables(**tgt))
    v0, g0 = vg(rec["theta0"])
    np.testing.assert_allclose(v0, float(rec["init_target"]), rtol=1e-12)
    if "init_grad" in rec:
        np.testing.assert_allclose(g0, rec["init_grad"], rtol=1e-9, atol=1e-12)

    def check(it, theta, target, acc):
        assert acc == bool(rec["accepted"][it]), it
        np.testing.assert_allclose(theta, rec["sample"][it], rtol=1e-9, atol=1e-9 * np.abs(rec["sample"][it]).max())
        np.testing.assert_allclose(target, float(rec["target_val"][it]), rtol=1e-9)

    end = replay(sampler, rec, vg, check)
    assert 0 < rec["accepted"].sum() < len(rec["accepted"])
    if sampler == "ram":
        np.testing.assert_allclose(end, rec["chol"], rtol=1e-9, atol=1e-9 * np.abs(rec["chol"]).max())
    if sampler == "am":
        np.testing.assert_allclose(np.tril(end["cov"]), rec["cov"], rtol=1e-9, atol=1e-9 * np.abs(rec["cov"]).max())
        assert end["num_accepted"] == int(rec["num_accepted"])


@pytest.mark.parametrize("P,M", [(1, 1), (2, 2), (5, 3), (65, 2), (128, 16)])
def test_value_and_gradient_equal_torch_mixture(P, M):
    from torch.distributions import Categorical, MixtureSameFamily, MultivariateNormal
    w, means, covs, _ = dr.random_mixture(P, M, seed=P + M)
    w = w / w.sum()  # MixtureSameFamily normalises its weights: the normalised density needs weights that sum to one
    c, mean, prec = dr.tables(w, means, covs, normalized=True)
    mix = MixtureSameFamily(Categorical(torch.tensor(w)), MultivariateNormal(torch.tensor(means),
                                                                            covariance_matrix=torch.tensor(covs)))
    rng = np.random.default_rng(3)
    for i in range(4):
        th = means[i % M] + rng.standard_normal(P)
        t = torch.tensor(th, requires_grad=True)
        val = mix.log_prob(t)
        (grad,) = torch.autograd.grad(val, t)
        v, g = dr.mix_value_grad(c, mean, prec, th)
        np.testing.assert_allclose(v, val.item(), rtol=1e-10)
        np.testing.assert_allclose(g, grad.numpy(), rtol=1e-8, atol=1e-10 * np.abs(grad.numpy()).max())
        vt, gt = dr.mix_value_grad(c, mean, prec, th, temperature=0.3)
        np.testing.assert_allclose([vt], [0.3 * v], rtol=1e-15)
        np.testing.assert_allclose(gt, 0.3 * g, rtol=1e-15)


def test_restatement_nan_and_minus_infinity():
    c, mean, prec = dr.tables(*dr.random_mixture(3, 2, seed=1)[:3])
    v, g = dr.mix_value_grad(c, mean, prec, np.array([0.1, np.nan, 0.2]))
    assert np.isnan(v) and np.isnan(g).all()
    v, _ = dr.mix_value_grad(c, mean, prec, np.array([1e200, 1e200, -1e200]))  # q overflows: every a_k is -inf
    assert np.isnan(v)
    far = mean[0] + 40 * np.sqrt(np.diag(np.linalg.inv(prec[0])))  # the max-subtraction path: no underflow to log(0)
    v, g = dr.mix_value_grad(c, mean, prec, far)
    assert np.isfinite(v) and np.isfinite(g).all() and v < -500


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("P,M", [(1, 1), (3, 2), (7, 4)])
def test_target_objects_equal_the_restatement(P, M, normalized):
    from eeyore_amd.models import MultivariateNormal, NormalMixture
    w, means, covs, _ = dr.random_mixture(P, M, seed=10 * P + M)
    tgt = NormalMixture(w, means, covs, normalized=normalized) if M > 1 else \
        MultivariateNormal(means[0], covs[0], normalized=normalized)
    c, mean, prec = dr.tables(w if M > 1 else [1.0], means, covs, normalized=normalized)
    np.testing.assert_allclose(tgt.c, c, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(tgt.prec, prec, rtol=1e-12, atol=1e-13)
    assert all(np.array_equal(tgt.prec[k], tgt.prec[k].T) for k in range(M))
    rng = np.random.default_rng(0)
    th = means[rng.integers(0, M, 6)] + rng.standard_normal((6, P))
    t = torch.tensor(th, requires_grad=True)
    vals = tgt(t, None, None)
    assert vals.shape == (6,)
    (grads,) = torch.autograd.grad(vals.sum(), t)
    for i in range(6):
        v, g = dr.mix_value_grad(c, mean, prec, th[i])
        np.testing.assert_allclose(vals[i].item(), v, rtol=1e-12)
        np.testing.assert_allclose(grads[i].numpy(), g, rtol=1e-9, atol=1e-12)
        assert abs(tgt(torch.tensor(th[i]), None, None).item() - v) <= 1e-12 * max(1.0, abs(v))  # theta [P] -> 0-d
    assert tgt(torch.tensor(th[0]), None, None).dim() == 0


def test_reference_example_density_is_weights_one_one():
    from eeyore_amd.models import NormalMixture
    m = [-2 * torch.ones(2, dtype=torch.float64), 2 * torch.ones(2, dtype=torch.float64)]
    tgt = NormalMixture([1, 1], torch.stack(m), torch.stack([torch.eye(2, dtype=torch.float64)] * 2), normalized=False)
    th = torch.tensor([0.3, -1.2], dtype=torch.float64)
    want = torch.log(torch.exp(-0.5 * torch.dot(th - m[0], th - m[0])) + torch.exp(-0.5 * torch.dot(th - m[1], th - m[1])))
    assert abs(tgt(th, None, None).item() - want.item()) <= 1e-14


# ---- the C ABI's validation, all of it before the device is touched
def _create(P, M, c=None, mean=None, prec=None, dtype=L.EY_F64):
    Pn, Mn = max(int(P), 1), max(int(M), 1)
    c = np.zeros(Mn) if c is None else np.asarray(c, np.float64)
    mean = np.zeros((Mn, Pn)) if mean is None else np.asarray(mean, np.float64)
    prec = np.tile(np.eye(Pn), (Mn, 1, 1)) if prec is None else np.asarray(prec, np.float64)
    c, mean, prec = (np.ascontiguousarray(a) for a in (c, mean, prec))
    dp = ct.POINTER(ct.c_double)
    h = ct.c_void_p()
    rc = L.lib().ey_plan_create_mixture(ct.byref(h), P, M, c.ctypes.data_as(dp), mean.ctypes.data_as(dp),
                                        prec.ctypes.data_as(dp), dtype, 0)
    if rc == 0:
        L.lib().ey_plan_destroy(h)
    assert rc == 0 or not h.value
    return rc, L.lib().ey_last_error().decode()


def test_symbol_is_exported_and_bound():
    assert "ey_plan_create_mixture" in L.SYMBOLS
    assert hasattr(L.lib(), "ey_plan_create_mixture")
    with open(os.path.join(ROOT, "include", "eeyore_amd.h")) as f:
        assert "int ey_plan_create_mixture(ey_plan** out, int64_t P, int M," in f.read()


EY_INVALID, EY_UNSUPPORTED = -1, -2


def _sym(P, fill):
    a = np.eye(P)
    fill(a)
    return a[None]


@pytest.mark.parametrize("want,kw,word", [
    (EY_INVALID, dict(P=0, M=1), "P must"),
    (EY_INVALID, dict(P=-3, M=1), "P must"),
    (EY_INVALID, dict(P=2, M=0), "M must"),
    (EY_UNSUPPORTED, dict(P=129, M=1), "128"),
    (EY_UNSUPPORTED, dict(P=2, M=17), "16"),
    (EY_INVALID, dict(P=2, M=1, c=[np.nan]), "finite"),
    (EY_INVALID, dict(P=2, M=1, c=[np.inf]), "finite"),
    (EY_INVALID, dict(P=2, M=2, mean=[[0, 0], [0, -np.inf]]), "finite"),
    (EY_INVALID, dict(P=2, M=1, prec=[[[1, np.nan], [np.nan, 1]]]), "finite"),
    (EY_INVALID, dict(P=2, M=1, prec=[[[1, 0.25], [0.25 * (1 + 2 ** -52), 1]]]), "symmetric"),
    (EY_INVALID, dict(P=3, M=2, prec=np.stack([np.eye(3), np.diag([1.0, 0.0, 1.0])])), "diagonal"),
    (EY_INVALID, dict(P=2, M=1, prec=[[[-1.0, 0], [0, 1]]]), "diagonal"),
    (EY_INVALID, dict(P=2, M=1, dtype=7), "dtype"),
])
def test_create_mixture_refuses_on_the_host(want, kw, word):
    rc, msg = _create(**kw)
    assert rc == want, (rc, msg)
    assert "ey_plan_create_mixture" in msg and word in msg, msg


def test_create_mixture_null_arguments():
    assert L.lib().ey_plan_create_mixture(None, 2, 1, None, None, None, L.EY_F64, 0) == EY_INVALID
    h = ct.c_void_p()
    assert L.lib().ey_plan_create_mixture(ct.byref(h), 2, 1, None, None, None, L.EY_F64, 0) == EY_INVALID and not h.value


# ---- Python argument errors
def test_target_value_errors():
    from eeyore_amd.models import MultivariateNormal, NormalMixture
    eye = np.eye(2)
    for bad in (dict(weights=[1, 0], means=np.zeros((2, 2)), covs=[eye, eye]),          # a weight <= 0
                dict(weights=[1, -1], means=np.zeros((2, 2)), covs=[eye, eye]),
                dict(weights=[1, 1], means=np.zeros((3, 2)), covs=[eye, eye]),          # mismatched shapes
                dict(weights=[1, 1], means=np.zeros((2, 2)), covs=[eye]),
                dict(weights=[1, 1], means=np.zeros((2, 2)), covs=[np.eye(3), np.eye(3)]),
                dict(weights=[1], means=np.zeros((1, 2)), covs=[[[1.0, 2.0], [2.0, 1.0]]]),  # not positive definite
                dict(weights=[1], means=np.zeros((1, 2)), covs=[[[1.0, 0.5], [0.4, 1.0]]]),  # not symmetric
                dict(weights=[1], means=[[0.0, np.nan]], covs=[eye])):
        with pytest.raises(ValueError):
            NormalMixture(**bad)
    with pytest.raises(ValueError):
        MultivariateNormal(np.zeros(2), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        MultivariateNormal(np.zeros((1, 2)), eye)


def test_distribution_model_errors_and_surface(capsys):
    from eeyore_amd.models import DistributionModel, MultivariateNormal
    from eeyore_amd.samplers import Gibbs
    with pytest.raises(ValueError, match="NormalMixture, MultivariateNormal"):
        DistributionModel(lambda theta, x, y: -0.5 * (theta ** 2).sum(), 2)
    tgt = MultivariateNormal(np.zeros(2), np.eye(2))
    with pytest.raises(ValueError, match="num_params"):
        DistributionModel(tgt, 3)
    m = DistributionModel(tgt, 2, temperature=0.5, dtype=torch.float32)
    assert m.num_params() == 2 and m.theta.dtype == torch.float32 and m.theta.requires_grad
    assert [n for n, _ in m.named_parameters()] == ["theta"] and m.temperature == 0.5 and m.log_pdf is tgt
    m.set_params(torch.tensor([1.0, 2.0]))
    assert m.get_params().tolist() == [1.0, 2.0]
    m.summary()
    assert "Number of distribution parameters: 2" in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match="DistributionModel"):
        Gibbs(m, theta0=torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the hot path is the HIP library: a cpu model has no plan
        m.log_target(torch.zeros(2), None, None)
