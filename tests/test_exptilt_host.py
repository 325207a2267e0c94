"""The exponential-tilt targets of DistributionModel without a GPU: the numpy restatement (tests/exptilt_restatement.py)
against the reference's own traces (tests/golden/g20_exptilt_traces.npz), the target objects' torch call and named
constructors, the host-side validation of ey_plan_create_exptilt, and the Python argument errors."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import exptilt_restatement as er
from tests.helpers import load
from tests.test_dist_host import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = [(n, s) for n in "un" for s in ("hmc", "mala", "mh")] + [("m", s) for s in ("hmc", "mala", "mh", "ram", "am")]


def g20():
    """{name: (tables (c, a, b, s), constructor arguments, {sampler: record})}"""
    z = load("g20_exptilt_traces.npz")
    out = {}
    for name in "unm":
        tab = tuple(z[f"{name}/tables/{k}"] for k in "cabs")
        args = {k.split("/", 2)[2]: z[k] for k in z.files if k.startswith(f"{name}/args/")}
        samplers = sorted({k.split("/")[1] for k in z.files if k.startswith(f"{name}/")} - {"args", "tables"})
        recs = {s: {k.split("/", 2)[2]: z[k] for k in z.files if k.startswith(f"{name}/{s}/")} for s in samplers}
        out[name] = (tab, args, recs)
    return out


def target_of(name, args):
    """The target object of a g20 group, built by the named constructors from the stored arguments."""
    from eeyore_amd.models import Gumbel, LogGamma, LogInverseGamma, LogWeibull, targets
    g = {k: float(v) for k, v in args.items()}
    nz = bool(g["normalized"])
    if name in "un":
        return LogGamma(g["shape"], g["scale"], normalized=nz)
    return targets.concat(LogGamma(g["gamma_shape"], g["gamma_scale"], nz),
                          LogInverseGamma(g["invgamma_shape"], g["invgamma_rate"], nz),
                          LogWeibull(g["weibull_scale"], g["weibull_concentration"], nz),
                          Gumbel(g["gumbel_loc"], g["gumbel_scale"], nz))


# ---- 1. the restatement replays the reference's traces
@pytest.mark.parametrize("name,sampler", TRACES)
def test_restatement_reproduces_reference_traces(name, sampler):
    tab, _, recs = g20()[name]
    assert sorted(recs) == sorted(s for n, s in TRACES if n == name)
    rec = recs[sampler]
    vg = er.tilt_value_grad_fn(*tab)
    v0, g0 = vg(rec["theta0"])
    np.testing.assert_allclose(v0, float(rec["init_target"]), rtol=1e-9)
    if "init_grad" in rec:
        np.testing.assert_allclose(g0, rec["init_grad"], rtol=1e-9, atol=1e-12)

    def check(it, theta, target, acc):
        assert acc == bool(rec["accepted"][it]), it
        np.testing.assert_allclose(theta, rec["sample"][it], rtol=1e-8, atol=1e-8 * np.abs(rec["sample"][it]).max())
        np.testing.assert_allclose(target, float(rec["target_val"][it]), rtol=1e-9)

    end = replay(sampler, rec, vg, check)
    n_acc = int(rec["accepted"].sum())
    assert 0 < n_acc < len(rec["accepted"])
    if sampler in ("hmc", "mala", "mh"):
        assert 15 <= n_acc <= 45
    if sampler == "ram":
        np.testing.assert_allclose(end, rec["chol"], rtol=1e-8, atol=1e-8 * np.abs(rec["chol"]).max())
    if sampler == "am":
        np.testing.assert_allclose(np.tril(end["cov"]), rec["cov"], rtol=1e-8, atol=1e-8 * np.abs(rec["cov"]).max())
        assert end["num_accepted"] == int(rec["num_accepted"])


# ---- 2. the target objects' torch call and its autograd gradient
def _objects():
    from eeyore_amd.models import ExponentialTilt
    out = [(target_of(n, a), tab) for n, (tab, a, _) in g20().items()]
    for P in (1, 5, 128):
        c, a, b, s = er.random_tilt(P, seed=P)
        out.append((ExponentialTilt(a, b, s, c=c), (c, a, b, s)))
    return out


def test_target_objects_equal_the_restatement():
    rng = np.random.default_rng(0)
    for tgt, tab in _objects():
        P = tgt.P
        assert P == len(tab[0])
        th = er.mode(tab) + 0.7 * rng.standard_normal((20, P)) / np.abs(tab[3])
        t = torch.tensor(th, requires_grad=True)
        vals = tgt(t, None, None)
        assert vals.shape == (20,) and vals.dtype == torch.float64
        (grads,) = torch.autograd.grad(vals.sum(), t)
        for i in range(20):
            v, g, S = er.tilt_value_grad(*tab, th[i])
            assert abs(vals[i].item() - v) <= 1e-12 * S
            assert np.all(np.abs(grads[i].numpy() - g) <= 1e-12 * S)
            one = tgt(torch.tensor(th[i]), None, None)  # theta [P] -> 0-d
            assert one.dim() == 0 and abs(one.item() - v) <= 1e-12 * S
        assert tgt(t.detach().float()).dtype == torch.float32


# ---- 3. ... equals the reference's closure at the recorded start
@pytest.mark.parametrize("name", list("unm"))
def test_target_objects_equal_the_recorded_closure_value(name):
    _, args, recs = g20()[name]
    tgt = target_of(name, args)
    for rec in recs.values():
        v = tgt(torch.tensor(rec["theta0"]), None, None)
        np.testing.assert_allclose(v.item(), float(rec["init_target"]), rtol=1e-12)
    t = torch.tensor(recs["mala"]["theta0"], requires_grad=True)
    (g,) = torch.autograd.grad(tgt(t), t)
    np.testing.assert_allclose(g.numpy(), recs["mala"]["init_grad"], rtol=1e-12)


# ---- 4. the named constructors
@pytest.mark.parametrize("name", list("unm"))
def test_named_constructors_give_the_stored_tables(name):
    tab, args, _ = g20()[name]
    tgt = target_of(name, args)
    for got, want in zip((tgt.c, tgt.a, tgt.b, tgt.s), tab):
        assert got.dtype == np.float64 and got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-15)


def test_named_constructors_equal_the_restatement_and_broadcast():
    from eeyore_amd.models import Gumbel, LogGamma, LogInverseGamma, LogWeibull
    x, y = np.array([0.7, 2.0, 3.5]), 1.3
    for cls, fn, args in ((LogGamma, er.log_gamma, (x, y)), (LogInverseGamma, er.log_inverse_gamma, (y, x)),
                          (LogWeibull, er.log_weibull, (x, y)), (Gumbel, er.gumbel, (-x, y))):
        for nz in (True, False):
            tgt = cls(*args, normalized=nz)
            assert tgt.P == 3 and tgt.normalized == nz
            for got, want in zip((tgt.c, tgt.a, tgt.b, tgt.s), fn(*args, normalized=nz)):
                np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-15)
            assert nz or not tgt.c.any()
        assert cls(torch.tensor(2.0), 0.5).P == 1


def test_normalised_members_integrate_to_one():
    """exp(log p) of every family sums to one over a fine grid of theta: the constants c are the normalisers."""
    from eeyore_amd.models import Gumbel, LogGamma, LogInverseGamma, LogWeibull
    th = torch.linspace(-30, 30, 600001, dtype=torch.float64)[:, None]
    for tgt in (LogGamma(2.0, 1.0), LogGamma(0.7, 3.0), LogInverseGamma(2.5, 1.5), LogWeibull(1.3, 1.7), Gumbel(0.4, 0.8)):
        mass = torch.trapezoid(torch.exp(tgt(th)), th[:, 0]).item()
        assert abs(mass - 1) < 1e-9, (tgt, mass)


# ---- 5. concat
def test_concat_keeps_coordinate_order():
    from eeyore_amd.models import ExponentialTilt, Gumbel, LogGamma, targets
    p = [LogGamma([2.0, 3.0], 1.5), Gumbel(0.1, 0.8, normalized=False), ExponentialTilt([1.0, -2.0], [0.5, 0.6], [2.0, -0.5])]
    j = targets.concat(*p)
    assert j.P == 5 and type(j) is ExponentialTilt
    for n in "cabs":
        assert np.array_equal(getattr(j, n), np.concatenate([getattr(t, n) for t in p]))
    th = torch.tensor([0.1, -0.2, 0.3, 0.4, -0.5], dtype=torch.float64)
    want = p[0](th[:2]) + p[1](th[2:3]) + p[2](th[3:])
    assert abs(j(th).item() - want.item()) <= 1e-14
    assert targets.concat(p[1]).P == 1
    for bad in ((), (p[0], "x"), (targets.MultivariateNormal(np.zeros(2), np.eye(2)),)):
        with pytest.raises(ValueError):
            targets.concat(*bad)
    assert set(targets.TARGETS) >= {ExponentialTilt, LogGamma, Gumbel, targets.LogInverseGamma, targets.LogWeibull,
                                    targets.NormalMixture, targets.MultivariateNormal}


# ---- 6. the restatement's edge cases
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_restatement_overflow_underflow_and_nan(sign):
    c, a, b, s = er.random_tilt(3, seed=2)
    s = np.abs(s) * np.array([1.0, sign, -1.0])
    a = np.abs(a) * np.sign(s)
    th = er.mode((c, a, b, s))
    hi = th.copy()
    hi[1] = 800 / s[1]
    v, g, _ = er.tilt_value_grad(c, a, b, s, hi)
    assert v == -np.inf and not np.isnan(g).any()
    assert np.isinf(g[1]) and np.sign(g[1]) == -np.sign(s[1]) and np.isfinite(g[[0, 2]]).all()
    vt, gt, _ = er.tilt_value_grad(c, a, b, s, hi, temperature=0.3)
    assert vt == -np.inf and gt[1] == g[1]
    lo = th.copy()
    lo[1] = -800 / s[1]
    v, g, _ = er.tilt_value_grad(c, a, b, s, lo)
    assert np.isfinite(v) and g[1] == a[1] and np.isfinite(g).all()
    bad = th.copy()
    bad[1] = np.nan
    v, g, S = er.tilt_value_grad(c, a, b, s, bad)
    assert np.isnan(v) and np.isnan(g[1]) and np.isnan(S)
    v, g, S = er.tilt_value_grad(c, a, b, s, th)  # at the mode: a zero gradient, S above |value|
    assert np.abs(g).max() <= 1e-14 * np.abs(a).max() and S >= abs(v)
    vb, gb = er.tilt_value_grad_batch(c, a, b, s, np.stack([th, hi, lo]))
    assert vb[0] == v and vb[1] == -np.inf and gb[2, 1] == a[1]


# ---- 7. the symbol
def test_symbol_is_exported_and_bound():
    assert "ey_plan_create_exptilt" in L.SYMBOLS
    assert hasattr(L.lib(), "ey_plan_create_exptilt")
    with open(os.path.join(ROOT, "include", "eeyore_amd.h")) as f:
        text = f.read()
    decl = "int ey_plan_create_exptilt(ey_plan** out, int64_t P, const double* c, const double* a, const double* b,"
    assert decl in text and text.index(decl) > text.index("int ey_plan_create_mixture(")


# ---- 8. the C ABI's validation, all of it before the device is touched
EY_INVALID, EY_UNSUPPORTED = -1, -2


def _create(P, c=None, a=None, b=None, s=None, dtype=L.EY_F64):
    Pn = max(int(P), 1)
    tabs = [np.ascontiguousarray(np.full(Pn, d) if t is None else np.asarray(t, np.float64))
            for t, d in ((c, 0.0), (a, 2.0), (b, 1.0), (s, 1.0))]
    dp = ct.POINTER(ct.c_double)
    h = ct.c_void_p(1)
    rc = L.lib().ey_plan_create_exptilt(ct.byref(h), P, *(t.ctypes.data_as(dp) for t in tabs), dtype, 0)
    if rc == 0:
        L.lib().ey_plan_destroy(h)
    assert rc == 0 or not h.value
    return rc, L.lib().ey_last_error().decode()


@pytest.mark.parametrize("want,kw,word", [
    (EY_INVALID, dict(P=2, c=[0, np.nan]), "c[1] is not finite"),
    (EY_INVALID, dict(P=2, c=[np.inf, 0]), "c[0] is not finite"),
    (EY_INVALID, dict(P=2, a=[2, np.nan]), "a[1] is not finite"),
    (EY_INVALID, dict(P=2, a=[-np.inf, 2]), "a[0] is not finite"),
    (EY_INVALID, dict(P=2, b=[1, np.inf]), "b[1] is not finite"),
    (EY_INVALID, dict(P=2, b=[np.nan, 1]), "b[0] is not finite"),
    (EY_INVALID, dict(P=2, s=[1, np.nan]), "s[1] is not finite"),
    (EY_INVALID, dict(P=2, s=[np.inf, 1]), "s[0] is not finite"),
    (EY_INVALID, dict(P=3, b=[1, 1, 0.0]), "b[2]"),
    (EY_INVALID, dict(P=3, b=[1, -0.5, 1]), "b[1]"),
    (EY_INVALID, dict(P=3, s=[1, 0.0, 1]), "s[1]"),
    (EY_INVALID, dict(P=3, a=[2, 2, 2], s=[1, 1, -1]), "a[2]"),
    (EY_INVALID, dict(P=2, a=[-2, 0.0], s=[-1, 1]), "a[1]"),
    (EY_INVALID, dict(P=0), "P must"),
    (EY_INVALID, dict(P=-3), "P must"),
    (EY_UNSUPPORTED, dict(P=129), "128"),
    (EY_INVALID, dict(P=2, dtype=7), "dtype"),
])
def test_create_exptilt_refuses_on_the_host(want, kw, word):
    rc, msg = _create(**kw)
    assert rc == want, (rc, msg)
    assert "ey_plan_create_exptilt" in msg and word in msg, msg


def test_create_exptilt_null_arguments():
    lib = L.lib()
    one = np.ones(2)
    dp = one.ctypes.data_as(ct.POINTER(ct.c_double))
    assert lib.ey_plan_create_exptilt(None, 2, dp, dp, dp, dp, L.EY_F64, 0) == EY_INVALID
    for k in range(4):
        tabs = [dp] * 4
        tabs[k] = None
        h = ct.c_void_p(1)
        assert lib.ey_plan_create_exptilt(ct.byref(h), 2, *tabs, L.EY_F64, 0) == EY_INVALID and not h.value
        assert "ey_plan_create_exptilt" in lib.ey_last_error().decode() and "null" in lib.ey_last_error().decode()


# ---- 9. Python argument errors
def test_target_value_errors():
    from eeyore_amd.models import ExponentialTilt, Gumbel, LogGamma, LogInverseGamma, LogWeibull
    ok = dict(a=[2.0, 2.0], b=[1.0, 1.0], s=[1.0, 1.0], c=[0.0, 0.0])
    ExponentialTilt(**ok)
    for key, val in (("a", [2.0, np.nan]), ("b", [np.inf, 1.0]), ("s", [1.0, -np.inf]), ("c", [np.nan, 0.0]),  # non-finite
                     ("b", [1.0, 0.0]), ("b", [-1.0, 1.0]), ("s", [0.0, 1.0]), ("a", [2.0, -2.0]), ("a", [0.0, 2.0]),
                     ("a", [2.0, 2.0, 2.0]), ("b", np.ones((2, 2))), ("s", []), ("a", "x")):  # shapes and types
        with pytest.raises(ValueError):
            ExponentialTilt(**dict(ok, **{key: val}))
    with pytest.raises(ValueError, match=r"b\[1\]"):
        ExponentialTilt([2.0, 2.0], [1.0, -1.0], 1.0)
    for cls in (LogGamma, LogInverseGamma, LogWeibull):
        for bad in ((0.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (1.0, np.inf), ([1.0, 2.0], [1.0, 2.0, 3.0])):
            with pytest.raises(ValueError):
                cls(*bad)
    for bad in ((0.0, 0.0), (np.inf, 1.0), (0.0, -2.0)):
        with pytest.raises(ValueError):
            Gumbel(*bad)


# ---- 10. the model surface
def test_distribution_model_errors_and_surface(capsys):
    from eeyore_amd.models import DistributionModel, LogGamma, targets
    from eeyore_amd.samplers import Gibbs
    with pytest.raises(ValueError, match="NormalMixture, MultivariateNormal"):
        DistributionModel(lambda theta, x, y: theta.sum() - torch.exp(theta).sum(), 2)
    tgt = targets.concat(LogGamma(2.0, 1.0), targets.Gumbel(0.0, 1.0))
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
