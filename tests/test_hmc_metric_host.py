"""HMC with a fixed metric, without a GPU: the numpy restatement (tests/hmc_metric_restatement.py) against the oracle's HMC
draw, an independently written momentum form and the whitening invariance; the metric classes; the C-ABI surface of
include/eeyore_amd_ext.h; the sampler's refusals; the seed table of the GPU test."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from eeyore_amd.samplers import DenseMetric, DiagMetric  # (every test of this file needs the feature: none runs without it)
from oracle import mlp_oracle as orc
from tests import dist_restatement as dr
from tests.hmc_metric_restatement import DIAG, TRIL, factor, hmc_metric_draw, hmc_metric_draw_momentum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _mlp_case(seed=0):
    """MLP(4-3-3) with a softmax likelihood on 30 rows, as a Spec and a value-and-gradient function."""
    rng = np.random.default_rng(seed)
    dims, acts, lik, N = [4, 3, 3], [1, 0], 1, 30
    x = rng.standard_normal((N, dims[0]))
    y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    spec = orc.Spec(dims, acts, lik)

    def vg(th):
        t, g = orc.upto_grad_log_target(spec, np.asarray(th, np.float64), x, y)
        return float(t), g
    return spec, x, y, vg, sum((dims[k] + 1) * dims[k + 1] for k in range(2))


def _chol(P, rng, cond=50.0):
    q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    S = (q * np.logspace(0, np.log10(cond), P)) @ q.T * 0.05
    return np.linalg.cholesky((S + S.T) / 2)


@pytest.mark.parametrize("form", [DIAG, TRIL], ids=["diag", "dense"])
@pytest.mark.parametrize("num_steps", [1, 3, 8])
def test_identity_metric_is_the_oracles_hmc_draw(form, num_steps):
    spec, x, y, vg, P = _mlp_case()
    rng = np.random.default_rng(1)
    metric = np.ones(P) if form == DIAG else np.eye(P)
    accepts = 0
    for it in range(12):
        th = 0.3 * rng.standard_normal(P)
        v, u, step = rng.standard_normal(P), rng.random(), 0.02 + 0.1 * rng.random()
        t0, g0 = vg(th)
        new, info = orc.hmc_draw(spec, dict(sample=th, target_val=np.float64(t0), grad_val=g0), v, u, x, y, step, num_steps)
        w_th, w_t, w_g, acc, hc, hp, rate, v_end = hmc_metric_draw(vg, th, t0, g0, form, metric, v, u, step, num_steps)
        assert acc == bool(info["accepted"])
        accepts += acc
        np.testing.assert_allclose([hc, hp, rate], [info["h_cur"], info["h_prop"], info["rate"]], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(w_th, new["sample"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(w_t, new["target_val"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(w_g, new["grad_val"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(v_end, -info["prop_momentum"], rtol=1e-12, atol=1e-12)  # the oracle negates it
    assert 0 < accepts


@pytest.mark.parametrize("form", [DIAG, TRIL], ids=["diag", "dense"])
def test_velocity_form_equals_the_momentum_form(form):
    spec, x, y, vg, P = _mlp_case(2)
    rng = np.random.default_rng(3)
    accepts = rejects = 0
    for it in range(16):
        metric = 0.5 + rng.random(P) if form == DIAG else _chol(P, rng)
        th = 0.3 * rng.standard_normal(P)
        v, u, step, n = rng.standard_normal(P), rng.random(), 0.15 + 0.5 * rng.random(), int(rng.integers(1, 6))
        t0, g0 = vg(th)
        a = hmc_metric_draw(vg, th, t0, g0, form, metric, v, u, step, n)
        b = hmc_metric_draw_momentum(vg, th, t0, g0, form, metric, v, u, step, n)
        assert a[3] == b[3]
        accepts, rejects = accepts + a[3], rejects + (not a[3])
        for k in (0, 1, 2, 4, 5, 6):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(a[7], factor(form, metric).T @ b[7], rtol=1e-10, atol=1e-10)  # v = L^T p
    assert accepts and rejects


@pytest.mark.parametrize("P", [2, 7, 33])
def test_whitening_invariance(P):
    """N(0, Sigma) under the metric chol(Sigma) from theta = L q is N(0, I) under the identity from q: with the same v and
    u, h_cur, h_prop and the decision agree and theta' = L q'."""
    rng = np.random.default_rng(P)
    Lf = _chol(P, rng, cond=1e3)
    Sigma = Lf @ Lf.T
    prec = np.linalg.inv(Sigma)
    prec = (prec + prec.T) / 2
    vg_a = lambda th: (-0.5 * float(th @ prec @ th), -(prec @ th))  # noqa: E731
    vg_b = lambda q: (-0.5 * float(q @ q), -q)  # noqa: E731
    accepts = rejects = 0
    for it in range(12):
        q, v, u = 1.5 * rng.standard_normal(P), rng.standard_normal(P), rng.random()
        step, n = 0.3 + 1.2 * rng.random(), int(rng.integers(1, 5))
        ta, ga = vg_a(Lf @ q)
        tb, gb = vg_b(q)
        a = hmc_metric_draw(vg_a, Lf @ q, ta, ga, TRIL, Lf, v, u, step, n)
        b = hmc_metric_draw(vg_b, q, tb, gb, TRIL, np.eye(P), v, u, step, n)
        assert a[3] == b[3]
        accepts, rejects = accepts + a[3], rejects + (not a[3])
        np.testing.assert_allclose([a[4], a[5]], [b[4], b[5]], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(a[0], Lf @ b[0], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(a[7], b[7], rtol=1e-10, atol=1e-10)
    assert accepts and (rejects or P == 2)


def test_restatement_reads_the_lower_triangle_only_and_rejects_a_nan_rate():
    rng = np.random.default_rng(0)
    L0 = np.tril(rng.standard_normal((4, 4))) + 2 * np.eye(4)
    dirty = L0 + np.triu(np.full((4, 4), np.nan), 1)
    th, v = rng.standard_normal(4), rng.standard_normal(4)
    vg = lambda q: (-0.5 * float(q @ q), -q)  # noqa: E731
    a = hmc_metric_draw(vg, th, *vg(th), TRIL, L0, v, 0.5, 0.3, 3)
    b = hmc_metric_draw(vg, th, *vg(th), TRIL, dirty, v, 0.5, 0.3, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.isfinite(a[5])
    nan = lambda q: (float("nan"), q * float("nan"))  # noqa: E731
    r = hmc_metric_draw(nan, th, *vg(th), TRIL, L0, v, 0.0, 0.3, 2)
    assert r[3] is False and np.array_equal(r[0], th) and np.isnan(r[6])
    with pytest.raises(ValueError):
        factor(2, L0)


# ------------------------------------------------------------------------------------------------ the metric classes
def _formula(x, dense):
    """Stan's regularised estimate, written out in numpy: x [n, P]."""
    n, P = x.shape
    d = x - x.mean(0)
    S = d.T @ d / (n - 1)
    est = n / (n + 5.0) * S + 1e-3 * 5.0 / (n + 5.0) * np.eye(P)
    return np.linalg.cholesky(est) if dense else np.sqrt(np.diag(est))


def test_from_samples_against_the_formula():
    from eeyore_amd.chains import ChainBuffer
    rng = np.random.default_rng(4)
    n, C, P = 40, 3, 5
    A = rng.standard_normal((P, P))
    x = rng.standard_normal((n, C, P)) @ A.T + rng.standard_normal((1, C, 1))
    xt = torch.tensor(x)
    pooled = x.reshape(n * C, P)
    np.testing.assert_allclose(DenseMetric.from_samples(xt).scale_tril.numpy(), _formula(pooled, True), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(DiagMetric.from_samples(xt).scale.numpy(), _formula(pooled, False), rtol=1e-11, atol=1e-12)
    dm, gm = DenseMetric.from_samples(xt, per_chain=True), DiagMetric.from_samples(xt, per_chain=True)
    assert tuple(dm.scale_tril.shape) == (C, P, P) and tuple(gm.scale.shape) == (C, P) and dm.per_chain and gm.per_chain
    for c in range(C):
        np.testing.assert_allclose(dm.scale_tril[c].numpy(), _formula(x[:, c], True), rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(gm.scale[c].numpy(), _formula(x[:, c], False), rtol=1e-11, atol=1e-12)
    # the regularisation keeps a degenerate sample usable: a constant coordinate gets the floor sqrt(1e-3 5 / (n + 5))
    flat = xt.clone()
    flat[..., 0] = 2.0
    np.testing.assert_allclose(DiagMetric.from_samples(flat).scale[0].item(), np.sqrt(1e-3 * 5 / (n * C + 5)), rtol=1e-12)
    assert torch.isfinite(DenseMetric.from_samples(flat).scale_tril).all()
    # a ChainBuffer of draws is read through get_samples
    buf = ChainBuffer(keys=['sample'])
    for i in range(n):
        buf.detach_and_update(dict(sample=xt[i]))
    assert torch.equal(DenseMetric.from_samples(buf).scale_tril, DenseMetric.from_samples(xt).scale_tril)
    for bad in (xt[0], xt[:1], "x"):
        with pytest.raises(ValueError, match="from_samples"):
            DiagMetric.from_samples(bad)


def test_metric_constructors_refuse_bad_tables():
    ok = DiagMetric(torch.tensor([1.0, 2.0]))
    assert ok.form == 'diag' and ok.num_params == 2 and not ok.per_chain and DiagMetric(torch.ones(3, 2)).per_chain
    for bad, word in ((torch.ones(2, 2, 2), "must be"), (torch.tensor(1.0), "must be"), ([1.0, 2.0], "must be"),
                      (torch.tensor([1.0, float("inf")]), "non-finite"), (torch.tensor([1.0, float("nan")]), "non-finite"),
                      (torch.tensor([1.0, 0.0]), "positive"), (torch.tensor([[1.0, 1.0], [1.0, -2.0]]), "positive")):
        with pytest.raises(ValueError, match=word):
            DiagMetric(bad)
    eye = torch.eye(3)
    upper_nan = eye + torch.triu(torch.full((3, 3), float("nan")), 1)
    ok = DenseMetric(upper_nan)  # the strict upper triangle is never read
    assert ok.form == 'dense' and ok.num_params == 3 and not ok.per_chain and DenseMetric(eye.expand(4, 3, 3)).per_chain
    lower_nan = eye.clone()
    lower_nan[2, 0] = float("nan")
    zero_diag = eye.clone()
    zero_diag[1, 1] = 0.0
    for bad, word in ((torch.ones(3), "must be"), (torch.ones(2, 3), "must be"), (torch.ones(2, 2, 3, 3), "must be"),
                      (None, "must be"), (lower_nan, "non-finite"), (zero_diag, "positive diagonal"),
                      (-eye, "positive diagonal"), (torch.stack([eye, zero_diag]), "positive diagonal")):
        with pytest.raises(ValueError, match=word):
            DenseMetric(bad)
    assert torch.equal(DenseMetric.identity(3).scale_tril, torch.eye(3, dtype=F64))
    assert torch.equal(DiagMetric.identity(3).scale, torch.ones(3, dtype=F64))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_ext_header_declares_what_the_binding_holds_and_the_library_exports():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_ext.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.EXT_SYMBOLS) == {"ey_hmc_metric_step", "ey_hmc_metric_run"}, declared ^ set(L.EXT_SYMBOLS)
    assert not set(L.EXT_SYMBOLS) & set(L.SYMBOLS)
    assert '#include "eeyore_amd.h"' in hdr
    lib = L.lib()
    for name, (res, args) in L.EXT_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # the number of arguments the binding passes is the number the header declares
    for name in declared:
        proto = hdr[hdr.index("int " + name + "("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == len(L.EXT_SYMBOLS[name][1]), name
    forms = dict(re.findall(r"(EY_METRIC_[A-Z]+) = (\d+)", re.search(r"enum ey_metric_form \{([^}]*)\}", hdr).group(1)))
    assert {k: int(v) for k, v in forms.items()} == {"EY_METRIC_DIAG": L.EY_METRIC_DIAG, "EY_METRIC_TRIL": L.EY_METRIC_TRIL}
    assert (DIAG, TRIL) == (L.EY_METRIC_DIAG, L.EY_METRIC_TRIL)
    comment = hdr[:hdr.index("int ey_hmc_metric_step")].rsplit("/*", 1)[1]
    for word in ("only j <= i", "ey_plan_attach_da", "EY_ERR_UNSUPPORTED", "v = L^T p"):
        assert word in comment, word


def test_argument_errors_without_gpu():
    lib = L.lib()
    p = ct.c_void_p(1)
    assert lib.ey_hmc_metric_step(None, p, p, p, p, 1, 1, None, None, None, 0.1, None, 3, None, 1, 0, 0, 0, 0, p, None, None,
                                  None, None) == -1
    assert b"null plan" in lib.ey_last_error() and b"ey_hmc_metric_step" in lib.ey_last_error()
    assert lib.ey_hmc_metric_run(None, p, p, p, p, 0, 1, None, 0.1, None, 3, None, 1, 0, 0, 0, 0, 8, None, None, None, None,
                                 p, None) == -1
    assert b"ey_hmc_metric_run" in lib.ey_last_error()


# ------------------------------------------------------------------------------------------------ the sampler
def test_sampler_refusals_before_any_launch():
    from torch.utils.data import DataLoader
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import HMC
    dl = DataLoader(EmptyXYDataset())
    small = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[2, 2, 1]))
    P = small.num_params()
    for metric in (DiagMetric(torch.ones(P)), DenseMetric(torch.eye(P))):
        with pytest.raises(ValueError, match="init_step_mode='reference'"):
            HMC(small, dataloader=dl, metric=metric, init_step_mode='reference')
        s = HMC(small, dataloader=dl, metric=metric)
        assert s._metric_form == metric.form and s._metric_index is None and s.metric is metric
        assert tuple(s._metric.shape) == tuple(metric.table.shape) and s._metric.dtype == small.dtype
        with pytest.raises(ValueError, match="no metric form"):
            s.leapfrog(torch.zeros(P), torch.zeros(P), None, None)
    assert HMC(small, dataloader=dl)._metric is None  # no metric: the plain kernels
    with pytest.raises(ValueError, match="DiagMetric or a DenseMetric"):
        HMC(small, dataloader=dl, metric=torch.eye(P))
    with pytest.raises(ValueError, match=f"the model has {P}"):
        HMC(small, dataloader=dl, metric=DiagMetric(torch.ones(P + 1)))
    with pytest.raises(ValueError, match="one entry or one per chain"):
        HMC(small, dataloader=dl, metric=DiagMetric(torch.ones(2, P)))
    big = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[6, 14, 2, 1]))
    Pb = big.num_params()
    assert Pb > 128
    with pytest.raises(ValueError, match="DenseMetric is limited to 128"):
        HMC(big, dataloader=dl, metric=DenseMetric(torch.eye(Pb)))
    assert HMC(big, dataloader=dl, metric=DiagMetric(torch.ones(Pb)))._metric_form == 'diag'  # no such limit
    # a table with an index, as PowerPosteriorSampler hands one over
    s = HMC(small, dataloader=dl)
    s._set_metric(DiagMetric(torch.ones(3, P)), index=[0])
    assert s._metric_index.dtype == torch.int32 and s._metric_index.tolist() == [0]
    s._set_metric(None)
    assert s._metric is None and s._metric_form is None and s._metric_index is None


def test_seed_table_of_the_gpu_test_keeps_the_restatement_decided():
    """The one-step GPU test allows at most 3 chains of a case inside the decision margin, none at C = 1; for its seeds the
    restatement alone leaves none there, with ten times the tolerance to spare, in f64 and on the inputs rounded to f32."""
    from tests import test_hmc_metric_gpu as T
    assert set(T.STEPS) == set(T.PLANS)
    for name in T.PLANS:
        for kind in T.KINDS:
            for C in T.CS:
                for num_steps in ([3, 1] if name in T.ONE_STEP_PLANS else [3]):
                    seed = T.SEEDS.get((name, kind, C, num_steps), 0)
                    for f32 in (False, True):
                        assert T._undecided(name, kind, C, num_steps, seed, f32, slack=10.0) == 0, (name, kind, C, num_steps)


def test_mixture_restatement_is_whitening_invariant_too():
    """The device test's construction, on the CPU: N(mu_k, Sigma) under chol(Sigma) against N(L^-1 mu_k, I)."""
    rng = np.random.default_rng(5)
    P, M = 2, 2
    Lf = _chol(P, rng, cond=1e3)
    w = 0.5 + rng.random(M)
    mu_q = 1.5 * rng.standard_normal((M, P))
    ta = dr.tables(w / w.sum(), mu_q @ Lf.T, np.stack([Lf @ Lf.T] * M), False)
    tb = dr.tables(w / w.sum(), mu_q, np.stack([np.eye(P)] * M), False)
    vg_a, vg_b = dr.mix_value_grad_fn(*ta), dr.mix_value_grad_fn(*tb)
    for it in range(6):
        q, v, u = mu_q[it % M] + rng.standard_normal(P), rng.standard_normal(P), rng.random()
        a = hmc_metric_draw(vg_a, Lf @ q, *vg_a(Lf @ q), TRIL, Lf, v, u, 0.4, 3)
        b = dr.hmc_draw(vg_b, q, *vg_b(q), v, u, 0.4, 3)
        assert a[3] == b[3]
        np.testing.assert_allclose([a[4], a[5]], [b[5], b[6]], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a[0], Lf @ b[0], rtol=1e-9, atol=1e-9)
