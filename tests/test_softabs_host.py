"""softabs without a GPU: ``stats.softabs`` (the eigh form), the numpy restatement of the kernel's one-sided Jacobi against
it (tests/softabs_restatement.py, yardstick in tests/softabs_cases.py), the reference's AM traces with the softabs
transform (tests/golden/g22_am_softabs_traces.npz), the symbols, ``SoftAbs`` and the routing of ``AM``."""
import ctypes as ct
import importlib.util
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests.helpers import load
from tests.softabs_cases import FACTOR, ONE_STEP_MODELS, SIZES, largest_lr, matrices, one_step_margins, yardstick
from tests.softabs_restatement import MAX_SWEEPS, f, replay, round_pairs, softabs_jacobi, softabs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1000.0


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------ stats.softabs
def test_stats_softabs_properties():
    from eeyore_amd import stats
    rng = np.random.default_rng(0)
    B = rng.standard_normal((6, 6))
    sym = B + B.T
    S = stats.softabs(_t(sym), A)
    assert torch.equal(S, S.mT) or (S - S.mT).abs().max() <= 1e-13 * S.abs().max()
    lam = np.linalg.eigvalsh(sym)
    np.testing.assert_allclose(np.linalg.eigvalsh(S.numpy()), np.sort(f(np.abs(lam), A)), rtol=1e-12)
    np.testing.assert_allclose(S.numpy(), softabs_ref(sym, A), rtol=0, atol=1e-12 * np.abs(sym).max())
    for a in (1000.0, 2.5):
        assert torch.equal(stats.softabs(torch.zeros(4, 4, dtype=torch.float64), a),
                           torch.eye(4, dtype=torch.float64) / a)
    v = rng.standard_normal(5)
    R = stats.softabs(_t(np.outer(v, v)), A).numpy()
    w = np.linalg.qr(np.column_stack([v, rng.standard_normal((5, 4))]))[0][:, 1:]  # a basis of v's complement
    np.testing.assert_allclose(w.T @ R @ w, np.eye(4) / A, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v @ R @ v / (v @ v), f(v @ v, A), rtol=1e-12)
    assert torch.isfinite(stats.softabs(torch.diag(_t([0.0, 1.0, -2.0])), A)).all()  # the reference gives NaN here
    batch = _t(np.stack([sym, 2 * sym, np.zeros((6, 6))]))
    got = stats.softabs(batch, A)
    assert got.shape == (3, 6, 6)
    for k in range(3):  # a batched call equals a loop (to rounding: torch's batched eigh and matmul are other code)
        torch.testing.assert_close(got[k], stats.softabs(batch[k], A), rtol=0, atol=1e-13 * float(batch[k].abs().max() + 1))
    assert stats.softabs(batch.reshape(1, 3, 6, 6), A).shape == (1, 3, 6, 6)
    assert stats.softabs(_t(sym).float()).dtype == torch.float32


# ------------------------------------------------------------------------------- the Jacobi restatement against eigh
def test_round_robin_schedule_meets_every_pair_once():
    for P in (1, 2, 3, 5, 27, 64, 65, 128):
        rounds = 2 * ((P + 1) // 2) - 1 if P > 1 else 0
        seen = []
        for r in range(rounds):
            pairs = round_pairs(P, r)
            cols = [c for pq in pairs for c in pq]
            assert len(cols) == len(set(cols)) and len(pairs) <= 64  # disjoint: one pair per lane
            seen += pairs
        assert sorted(seen) == [(p, q) for p in range(P) for q in range(p + 1, P)]


RATIOS = {}


@pytest.mark.parametrize("P", SIZES)
def test_jacobi_restatement_against_eigh(P):
    for name, M in matrices(P).items():
        S, sweeps = softabs_jacobi(np.tril(M) + np.triu(np.full((P, P), np.nan), 1), A)  # the upper triangle is not read
        assert np.array_equal(S, S.T) and 0 <= sweeps < MAX_SWEEPS, (name, sweeps)
        err, unit = np.linalg.norm(S - softabs_ref(M, A)), yardstick(M, A)
        RATIOS[(P, name)] = err / unit
        print(f"P={P} {name}: sweeps {sweeps} error / yardstick {err / unit:.3f}")
        assert err <= FACTOR * unit, (name, err, unit)
        if name == "zero":
            assert np.array_equal(S, np.eye(P) / A) and sweeps == (1 if P > 1 else 0)
        if name == "3I":
            assert np.allclose(S, 3.0 * np.eye(P), rtol=1e-15, atol=0)
    assert np.linalg.eigvalsh(S).min() > 0.5 / A  # the rank-deficient covariance became positive definite


def test_jacobi_restatement_leaves_a_non_finite_matrix():
    M = np.eye(3)
    M[2, 0] = np.nan
    S, sweeps = softabs_jacobi(M, A)
    assert sweeps == -1 and np.isnan(S[2, 0]) and np.isnan(S[0, 2]) and S[1, 1] == 1.0


# -------------------------------------------------------------------------------------------------- the g22 fixture
def _g22():
    z = load("g22_am_softabs_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abc"}


@pytest.mark.parametrize("name", list("abc"))
def test_fixture_replay(name):
    """Every draw from the recorded state before it: the flags equal; the state within the softabs yardstick of the raw
    covariance plus the roundings of that covariance itself ((cov_sum - n m m^T) / (n - 1): four roundings of entries of
    the size of its terms on either side), the sample to 1e-10 as in tests/test_am_host.py (the factorisation is not
    LAPACK's)."""
    rec = _g22()[name]
    assert rec["z"].shape[0] == dict(a=200, b=120, c=60)[name] and float(rec["a"]) == A
    transformed = factored = 0
    for it, got, want in replay(rec):
        assert abs(np.log(rec["u"][it]) - got["log_rate"]) >= 1e-6, it  # no near-tie to excuse
        assert got["accepted"] == bool(rec["accepted"][it]), it
        assert got["branch"] != 2, it
        factored += int(got["branch"] == 1)
        np.testing.assert_allclose(got["theta"], want["theta"], rtol=1e-10, atol=1e-10 * np.abs(want["theta"]).max())
        np.testing.assert_allclose(got["target"], want["target"], rtol=1e-10)
        assert got["num_accepted"] == want["num_accepted"]
        np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-12, atol=1e-14)
        if not got["transformed"]:
            assert np.array_equal(got["cov"], want["cov"]), it
            continue
        transformed += 1
        n = int(rec["n"][it])
        carried = 8 * 2.0 ** -52 * (np.linalg.norm(got["cov_sum"]) + n * got["mean"] @ got["mean"]) / (n - 1)
        err = np.linalg.norm(got["cov"] - want["cov"])
        assert err <= FACTOR * yardstick(got["raw_cov"], A) + carried, (it, err)
    assert transformed >= rec["z"].shape[0] // 2 and factored >= 3
    if name == "a":  # the covariance of the first states is rank deficient: the point of the transform
        first = next(got for _, got, _ in replay(rec) if got["transformed"])
        lam = np.linalg.eigvalsh(first["raw_cov"])
        assert lam[0] <= 1e-12 * lam[-1] and np.linalg.eigvalsh(first["cov"])[0] >= 0.9 / A


@pytest.mark.parametrize("name", ONE_STEP_MODELS)
def test_one_step_seeds_leave_no_tie(name):
    """The scenarios of tests/test_am_softabs_gpu.py::test_one_step_against_the_restatement put no chain within twice the
    f32 decision band of a tie, so that test skips no decision (it asserts that)."""
    assert (largest_lr(8), largest_lr(4)) == (73, 114)
    for f64 in ((True, False) if name == "largest" else (False,)):  # the other models are the same for both dtypes
        for C in (1, 3, 65):
            worst, band = one_step_margins(name, f64, C)
            print(f"{name} f64={f64} C={C}: smallest margin {worst:.4g} (band {band})")
            assert worst > band, (name, f64, C, worst)


# -------------------------------------------------------------------------------------------------------- the symbols
NEW = ("ey_am_softabs_step", "ey_am_softabs_run", "ey_am_softabs_fits", "ey_softabs")


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    lib = L.lib()
    for name in NEW:
        assert name + "(" in header and name in L.SYMBOLS and hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert all(f" T {name}\n" in exported for name in NEW)
    p = ct.c_void_p(1)
    assert lib.ey_am_softabs_step(None, p, p, p, p, p, p, p, 0, 0.05, 1.0, 1.0, 1000.0, 2, 0, 0, None, None, None, None, 1,
                                  0, 0, 0, 0, p, None, None, p, None) == -1
    assert b"null plan" in lib.ey_last_error()
    assert lib.ey_am_softabs_run(None, p, p, p, p, p, p, p, 0, 0.05, 1.0, 1.0, 1000.0, 2, 0, 0, None, 1, 0, 0, 0, 0, 8, None,
                                 None, None, None, p, p, None) == -1
    assert b"ey_am_softabs_run" in lib.ey_last_error()
    assert lib.ey_am_softabs_fits(None) == 0
    # ey_softabs refuses before it touches the device
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ey_softabs(p, 1, 4, L.EY_F64, bad, p, None, None) == -1 and b"a must be" in lib.ey_last_error()
    assert lib.ey_softabs(None, 1, 4, L.EY_F64, A, p, None, None) == -1
    assert lib.ey_softabs(p, 1, 0, L.EY_F64, A, p, None, None) == -1
    assert lib.ey_softabs(p, 1, 4, 7, A, p, None, None) == -1
    assert lib.ey_softabs(p, 1, 129, L.EY_F64, A, p, None, None) == -2 and b"128" in lib.ey_last_error()
    assert lib.ey_softabs(p, 0, 4, L.EY_F64, A, p, None, None) == 0


# --------------------------------------------------------------------------------------------------------- host logic
def test_softabs_callable():
    from eeyore_amd import samplers, stats
    from eeyore_amd.samplers import SoftAbs
    assert samplers.SoftAbs is SoftAbs and SoftAbs().a == 1000.0 and repr(SoftAbs(2)) == "SoftAbs(2.0)"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="a must be"):
            SoftAbs(bad)
    cov = _t([[2.0, 1.0], [1.0, 0.5]])  # rank 1
    assert torch.equal(SoftAbs(10.0)(cov), stats.softabs(cov, 10.0))  # a host tensor: the torch form
    with pytest.raises(RuntimeError, match="ROCm device"):
        stats.batched.softabs(cov)


def _small():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[2, 2, 1]))


def _am(**kw):
    from eeyore_amd.datasets import DataCounter
    from eeyore_amd.samplers import AM
    return AM(_small(), counter=DataCounter(1, 1), **kw)


class _Plan:
    def __init__(self, fits):
        self.fits = fits

    def am_softabs_fits(self):
        return self.fits


def test_am_routing():
    from eeyore_amd.samplers import Ridge, SoftAbs
    tr = SoftAbs(50.0)
    s = _am(transform=tr, cov0=torch.zeros(9, 9))
    assert not s._generic and s._softabs_a == 50.0 and s._eps == 0.0 and s._am_args()["softabs_a"] == 50.0
    assert torch.allclose(s.cov0.cpu().double(), torch.eye(9, dtype=torch.float64) / 50.0)  # transformed once, here
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s._route(_Plan(True))  # it fits: the fused path, no word
    assert not s._generic and s._softabs_a == 50.0
    with pytest.warns(RuntimeWarning, match="does not fit in LDS"):
        s._route(_Plan(False))
    assert s._generic and s._softabs_a is None and s.transform is tr and s._am_args()["softabs_a"] is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s._route(_Plan(False))  # said once
    lam = _am(transform=lambda m: SoftAbs(50.0)(m))  # a user's callable keeps today's path
    assert lam._generic and lam._softabs_a is None
    lam._route(_Plan(False))
    rid = _am(transform=Ridge(0.5))
    assert not rid._generic and rid._softabs_a is None and rid._eps == 0.5 and rid._am_args()["softabs_a"] is None
    assert _am()._softabs_a is None


def test_example_imports():
    path = os.path.join(ROOT, "examples", "bivariate_normal_mixture_am.py")
    spec = importlib.util.spec_from_file_location("bivariate_normal_mixture_am", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # nothing runs on import
    assert callable(mod.main) and callable(mod.run)
