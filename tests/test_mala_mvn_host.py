"""MALA with a MultivariateNormalKernel proposal, without a GPU: the numpy restatement against the reference's own traces
(tests/golden/g17_mala_mvn_traces.npz), its forward substitution, the C-ABI surface and the sampler's refusals."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import MultivariateNormal

from eeyore_amd import _lib as L
from tests.helpers import load
from tests.mala_mvn_restatement import forward_solve, group_value_grad, mala_mvn_draw, mvn_log_prob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _groups():
    z = load("g17_mala_mvn_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abcd"}


@pytest.mark.parametrize("name", list("abcd"))
def test_restatement_reproduces_reference_traces(name):
    rec = _groups()[name]
    vg = group_value_grad(rec)
    th, tv, g = rec["theta0"].copy(), float(rec["init_target"]), rec["init_grad"].copy()
    t0, g0 = vg(th)
    assert abs(t0 - tv) <= 1e-12 * max(1.0, abs(tv))
    np.testing.assert_allclose(g0, g, rtol=1e-12, atol=1e-12)
    assert rec["z"].shape[0] <= 300
    for it in range(rec["z"].shape[0]):
        th, tv, g, acc, _ = mala_mvn_draw(vg, th, tv, g, rec["L"], rec["z"][it], rec["u"][it], float(rec["step"]))
        assert acc == bool(rec["accepted"][it]), it
        np.testing.assert_allclose(th, rec["sample"][it], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(tv, rec["target_val"][it], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(g, rec["grad_val"][it], rtol=1e-9, atol=1e-9)


def test_fixture_groups_mix_accepts_and_rejects():
    g = _groups()
    for name, rec in g.items():
        assert 0 < rec["accepted"].sum() < len(rec["accepted"]), name
        assert float(rec["step"]) > 0
    assert np.array_equal(g["a"]["L"], np.eye(2)) and g["c"]["z"].shape == (120, 20)
    for name in "bcd":  # dense factors
        Lg = g[name]["L"]
        assert (Lg[np.tril_indices_from(Lg, -1)] != 0).all(), name
    here = os.path.join(ROOT, "tests", "golden")
    assert (os.path.getsize(os.path.join(here, "g17_mala_mvn_traces.npz"))
            <= os.path.getsize(os.path.join(here, "g16_mh_mvn_traces.npz")))


def test_restatement_reads_the_lower_triangle_only():
    rng = np.random.default_rng(0)
    L0 = np.tril(rng.standard_normal((4, 4))) + 2 * np.eye(4)
    dirty = L0 + np.triu(np.full((4, 4), np.nan), 1)
    th, g, z = rng.standard_normal(4), rng.standard_normal(4), rng.standard_normal(4)
    vg = lambda v: (-0.5 * float(v @ v), -v)  # noqa: E731
    a = mala_mvn_draw(vg, th, vg(th)[0], g, L0, z, 0.5, 0.3)
    b = mala_mvn_draw(vg, th, vg(th)[0], g, dirty, z, 0.5, 0.3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[1] == b[1] and a[3:] == b[3:]
    assert np.isfinite(a[4])


def test_forward_substitution_and_log_prob_agree_with_torch():
    rng = np.random.default_rng(1)
    for P in (1, 2, 7):
        A = rng.standard_normal((P, P))
        Lf = np.linalg.cholesky(A @ A.T + np.eye(P))
        r, loc = rng.standard_normal(P), rng.standard_normal(P)
        np.testing.assert_allclose(np.tril(Lf) @ forward_solve(Lf, r), r, rtol=1e-12, atol=1e-12)
        ref = MultivariateNormal(torch.tensor(loc), scale_tril=torch.tensor(Lf)).log_prob(torch.tensor(r))
        np.testing.assert_allclose(mvn_log_prob(Lf, loc, r), float(ref), rtol=1e-12, atol=1e-12)
    # the arithmetic runs in the dtype of its input
    assert mvn_log_prob(Lf.astype(np.float32), loc.astype(np.float32), r.astype(np.float32)).dtype == np.float32


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ey_mala_tril_step", "ey_mala_tril_run"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name), name
    comment = hdr[:hdr.index("int ey_mala_tril_step")].rsplit("/*", 1)[1]
    assert "only the lower triangle" in comment
    assert "ey_mala_tril_*" in hdr[:hdr.index("int ey_plan_create_mixture")].rsplit("/*", 1)[1]  # a mixture plan serves it


def test_argument_errors_without_gpu():
    lib = L.lib()
    p = ct.c_void_p(1)
    assert lib.ey_mala_tril_step(None, p, p, p, p, 1, None, None, None, 0.1, None, None, 1, 0, 0, 0, 0, p, None,
                                 None) == -1
    assert b"null plan" in lib.ey_last_error() and b"ey_mala_tril_step" in lib.ey_last_error()
    assert lib.ey_mala_tril_run(None, p, p, p, p, 1, None, 0.1, None, None, 1, 0, 0, 0, 0, 8, None, None, None, None, p,
                                None) == -1
    assert b"ey_mala_tril_run" in lib.ey_last_error()


def test_sampler_refuses_bad_kernels_before_any_launch():
    from torch.utils.data import DataLoader
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.kernels import IsoSEKernel, MultivariateNormalKernel, NormalKernel
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import MALA
    big = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[6, 14, 2, 1]))
    P = big.num_params()
    assert P > 128
    dl = DataLoader(EmptyXYDataset())
    with pytest.raises(ValueError, match="MALA.*128"):
        MALA(big, dataloader=dl, kernel=MultivariateNormalKernel(torch.zeros(P), torch.eye(P)))
    small = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[2, 2, 1]))
    with pytest.raises(ValueError, match="scale_tril must be"):
        MALA(small, dataloader=dl, kernel=MultivariateNormalKernel(torch.zeros(4), torch.eye(4)))
    Ps = small.num_params()
    with pytest.raises(ValueError, match="positive diagonal"):
        MALA(small, dataloader=dl, kernel=MultivariateNormalKernel(torch.zeros(Ps), torch.eye(Ps)))._set_tril(
            torch.tril(torch.ones(Ps, Ps), -1))
    for other in (IsoSEKernel(), NormalKernel(torch.zeros(Ps), torch.ones(Ps))):
        with pytest.raises(ValueError, match="MultivariateNormalKernel"):
            MALA(small, dataloader=dl, kernel=other)


def test_seed_table_of_the_gpu_test_keeps_the_restatement_decided():
    """The one-step GPU test allows at most 3 chains of a case inside the decision margin; for its seeds the restatement
    alone leaves none there, with ten times the tolerance to spare, in f64 and on the inputs rounded to f32."""
    from tests import test_mala_mvn_gpu as T
    for name in T.PLANS:
        for C in T.CS:
            seed = T.SEEDS.get((name, C), 0)
            for f32 in (False, True):
                assert T._undecided(name, C, seed, f32, slack=10.0) == 0, (name, C, f32)
