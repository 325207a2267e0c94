"""MetropolisHastings with a MultivariateNormalKernel proposal, without a GPU: the numpy restatement against the
reference's own traces (tests/golden/g16_mh_mvn_traces.npz), the kernel class against torch's MultivariateNormal, the
factor checks and the C-ABI surface."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import MultivariateNormal

from eeyore_amd import _lib as L
from tests.helpers import load
from tests.mh_mvn_restatement import group_target, mh_mvn_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _groups():
    z = load("g16_mh_mvn_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abcd"}


@pytest.mark.parametrize("name", list("abcd"))
def test_restatement_reproduces_reference_traces(name):
    rec = _groups()[name]
    tf = group_target(rec)
    th, tv = rec["theta0"].copy(), float(rec["init_target"])
    assert abs(tf(th) - tv) <= 1e-12 * max(1.0, abs(tv))
    assert rec["z"].shape[0] <= 300
    for it in range(rec["z"].shape[0]):
        th, tv, acc, _ = mh_mvn_draw(tf, th, tv, rec["L"], rec["z"][it], rec["u"][it])
        assert acc == bool(rec["accepted"][it]), it
        np.testing.assert_allclose(th, rec["sample"][it], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(tv, rec["target_val"][it], rtol=1e-12, atol=1e-12)


def test_fixture_groups_mix_accepts_and_rejects():
    g = _groups()
    for name, rec in g.items():
        assert 0 < rec["accepted"].sum() < len(rec["accepted"]), name
    assert np.array_equal(g["a"]["L"], np.eye(2)) and int(g["d"]["symmetric"]) == 0
    for name in "bcd":  # dense factors
        Lg = g[name]["L"]
        assert (Lg[np.tril_indices_from(Lg, -1)] != 0).all(), name


def test_restatement_reads_the_lower_triangle_only():
    rng = np.random.default_rng(0)
    L0 = np.tril(rng.standard_normal((4, 4)))
    dirty = L0 + np.triu(np.full((4, 4), np.nan), 1)
    th, z = rng.standard_normal(4), rng.standard_normal(4)
    tf = lambda v: -0.5 * float(v @ v)  # noqa: E731
    a = mh_mvn_draw(tf, th, tf(th), L0, z, 0.5)
    b = mh_mvn_draw(tf, th, tf(th), dirty, z, 0.5)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def _factor(P, seed, scale=0.7):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(P, P, generator=g, dtype=F64) / P ** 0.5
    return scale * torch.linalg.cholesky(A @ A.T + 0.5 * torch.eye(P, dtype=F64))


def test_kernel_agrees_with_torch_multivariate_normal():
    from eeyore_amd.kernels import MultivariateNormalKernel, NormalizedKernel
    P = 4
    loc, L1 = torch.linspace(-1, 1, P, dtype=F64), _factor(P, 1)
    k = MultivariateNormalKernel(loc, L1)
    assert isinstance(k, NormalizedKernel) and k.scale_tril is L1
    ref = MultivariateNormal(loc, scale_tril=L1)
    x = torch.tensor([0.3, -0.2, 0.9, 0.0], dtype=F64)
    assert torch.equal(k.log_prob(x), ref.log_prob(x))
    torch.manual_seed(5)
    a = k.sample()
    torch.manual_seed(5)
    assert torch.equal(a, ref.sample())
    # k(x1, x2): the density of x1 under the kernel centred at x2, with or without a new factor
    x2, L2 = torch.tensor([0.5, 0.5, -0.5, 0.1], dtype=F64), _factor(P, 2, 1.3)
    torch.testing.assert_close(k.k(x, x2), MultivariateNormal(x2, scale_tril=L1).log_prob(x).exp(), rtol=1e-14, atol=0)
    torch.testing.assert_close(k.k(x, x2, scale_tril=L2), MultivariateNormal(x2, scale_tril=L2).log_prob(x).exp(),
                               rtol=1e-14, atol=0)
    assert k.scale_tril is L2
    # a batched loc broadcasts torch's copy of the factor, not the kernel's own
    kb = MultivariateNormalKernel(torch.zeros(3, P, dtype=F64), L1)
    assert tuple(kb.scale_tril.shape) == (P, P) and tuple(kb.density.scale_tril.shape) == (3, P, P)
    kc = MultivariateNormalKernel(torch.zeros(3, P, dtype=F64), torch.stack([L1, L2, L1]))
    assert tuple(kc.scale_tril.shape) == (3, P, P)


def test_set_density_params_really_uses_the_new_factor():
    from eeyore_amd.kernels import MultivariateNormalKernel
    P = 3
    loc, L1, L2 = torch.tensor([1.0, -2.0, 0.5], dtype=F64), _factor(P, 3), _factor(P, 4, 2.0)
    k = MultivariateNormalKernel(torch.zeros(P, dtype=F64), L1)
    k.set_density_params(loc, scale_tril=L2)
    torch.manual_seed(11)
    s = k.sample()
    torch.manual_seed(11)
    z = torch.empty(P, dtype=F64).normal_()  # what MultivariateNormal.rsample draws
    torch.testing.assert_close(s - loc, L2 @ z, rtol=1e-14, atol=1e-15)
    assert not torch.allclose(s - loc, L1 @ z)
    # recentring alone keeps the factor
    k.set_density_params(torch.zeros(P, dtype=F64))
    torch.manual_seed(11)
    torch.testing.assert_close(k.sample(), L2 @ z, rtol=1e-14, atol=1e-15)


def test_check_scale_tril_refuses_each_bad_input():
    from eeyore_amd.kernels import check_scale_tril
    P = 3
    good = _factor(P, 6)
    check_scale_tril(good, P)
    check_scale_tril(torch.stack([good, 2 * good]), P)
    dirty = good.clone()
    dirty[0, 2] = float("nan")  # the strict upper triangle is never read
    check_scale_tril(dirty, P)
    for bad in (torch.ones(P), torch.eye(P + 1, dtype=F64), torch.zeros(2, P, P + 1), torch.zeros(1, 2, P, P),
                torch.zeros(0, P, P), [[1.0]]):
        with pytest.raises(ValueError, match="scale_tril must be"):
            check_scale_tril(bad, P)
    for v in (float("nan"), float("inf")):
        t = good.clone()
        t[2, 0] = v
        with pytest.raises(ValueError, match="non-finite"):
            check_scale_tril(t, P)
    for v in (0.0, -0.5):
        t = torch.stack([good, good.clone()])
        t[1, 1, 1] = v
        with pytest.raises(ValueError, match="positive diagonal"):
            check_scale_tril(t, P)


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ey_mh_tril_step", "ey_mh_tril_run"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name), name
    assert "only the lower triangle" in hdr


def test_argument_errors_without_gpu():
    lib = L.lib()
    p = ct.c_void_p(1)
    assert lib.ey_mh_tril_step(None, p, p, p, 1, None, None, None, None, 1, 0, 0, 0, 0, p, None, None) == -1
    assert b"null plan" in lib.ey_last_error() and b"ey_mh_tril_step" in lib.ey_last_error()
    assert lib.ey_mh_tril_run(None, p, p, p, 1, None, None, 1, 0, 0, 0, 0, 8, None, None, None, None, p, None) == -1
    assert b"ey_mh_tril_run" in lib.ey_last_error()


def test_sampler_refuses_bad_kernels_before_any_launch():
    from torch.utils.data import DataLoader
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.kernels import IsoSEKernel, MultivariateNormalKernel
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import MetropolisHastings
    big = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[6, 14, 2, 1]))
    P = big.num_params()
    assert P > 128
    dl = DataLoader(EmptyXYDataset())
    with pytest.raises(ValueError, match="128"):
        MetropolisHastings(big, dataloader=dl, kernel=MultivariateNormalKernel(torch.zeros(P), torch.eye(P)))
    small = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[2, 2, 1]))
    with pytest.raises(ValueError, match="scale_tril must be"):
        MetropolisHastings(small, dataloader=dl, kernel=MultivariateNormalKernel(torch.zeros(4), torch.eye(4)))
    with pytest.raises(ValueError, match="NormalKernel"):
        MetropolisHastings(small, dataloader=dl, kernel=IsoSEKernel())


def test_seed_table_of_the_gpu_test_keeps_the_restatement_decided():
    """The one-step GPU test allows at most 3 chains of a case inside the decision margin; for its seeds the restatement
    alone leaves none there, with ten times the tolerance to spare, in f64 and on the inputs rounded to f32."""
    from tests import test_mh_mvn_gpu as T
    for name in T.PLANS:
        for C in T.CS:
            seed = T.SEEDS.get((name, C), 0)
            for f32 in (False, True):
                assert T._undecided(name, C, seed, f32, slack=10.0) == 0, (name, C, f32)
