"""AM without a GPU: the numpy restatement against the reference's own traces (tests/golden/g13_am_traces.npz), the
kernel's left-looking factorisation against numpy's, Ridge, and argument errors."""
import ctypes as ct

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from eeyore_amd.samplers import AM, Ridge
from tests.am_restatement import am_draw, chol_left, spec_target
from tests.helpers import load


def _groups():
    z = load("g13_am_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abcd"}


@pytest.mark.parametrize("name", list("abcd"))
def test_restatement_reproduces_reference_traces(name):
    rec = _groups()[name]
    tf = spec_target(rec)
    P = rec["theta0"].shape[0]
    st = dict(theta=rec["theta0"].copy(), target=float(rec["init_target"]), mean=np.zeros(P), cov_sum=np.zeros((P, P)),
              cov=rec["cov0"].copy(), num_accepted=0)
    assert abs(tf(st["theta"]) - st["target"]) <= 1e-12 * max(1.0, abs(st["target"]))
    par = {k: float(rec[k]) for k in ("l", "b", "c", "eps")}
    k = 0
    for it in range(rec["z"].shape[0]):
        n = int(rec["n"][it])
        assert n == int(rec["idx"][it]) + 1 - int(rec["offset"])
        assert np.isnan(rec["u_mix"][it]) == (n <= int(rec["t0"]))  # two uniforms past t0, one before
        out = am_draw(tf, *(st[key] for key in ("theta", "target", "mean", "cov_sum", "cov", "num_accepted")),
                      rec["cov0"], rec["z"][it], rec["u_mix"][it], rec["u"][it], int(rec["idx"][it]),
                      int(rec["offset"]), t0=int(rec["t0"]), **par)
        assert out["branch"] != 2, it
        assert out["accepted"] == bool(rec["accepted"][it]), it
        # rtol 1e-10 elementwise, and 1e-10 of the vector's largest element for the elements near zero: chol_left is not
        # LAPACK's factorisation, and the factor of a covariance of condition 1e4..1e6 carries that times 2^-53
        np.testing.assert_allclose(out["theta"], rec["sample"][it], rtol=1e-10,
                                   atol=1e-10 * np.abs(rec["sample"][it]).max())
        np.testing.assert_allclose(out["target"], rec["target_val"][it], rtol=1e-10)
        st = {key: out[key] for key in st}
        if k < len(rec["state_it"]) and rec["state_it"][k] == it:
            scale = np.abs(rec["cov"][k]).max()
            np.testing.assert_allclose(np.tril(st["cov"]), rec["cov"][k], rtol=1e-9, atol=1e-9 * scale)
            # the samples agree to 1e-10 (the factorisation is not LAPACK's); what is summed from them no closer
            np.testing.assert_allclose(st["mean"], rec["running_mean"][k], rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(np.tril(st["cov_sum"]), rec["cov_sum"][k], rtol=1e-9,
                                       atol=1e-10 * np.abs(rec["cov_sum"][k]).max())
            assert st["num_accepted"] == int(rec["num_accepted"][k])
            k += 1
    assert k == len(rec["state_it"])


def test_fixture_groups_reach_both_branches():
    for name, rec in _groups().items():
        acc, after = rec["accepted"], rec["n"] > int(rec["t0"])
        assert 0 < acc.sum() < len(acc), name
        iso = int((rec["u_mix"][after] < float(rec["l"])).sum())
        assert iso >= 3 and int(after.sum()) - iso >= 3, name
    d = _groups()["d"]
    assert (d["n"] == np.arange(6, 46)).all() and (d["idx"] == np.arange(10, 50)).all()  # counter 10.. with offset 5


@pytest.mark.parametrize("P", [1, 5, 27, 65, 128])
def test_chol_left_equals_numpy(P):
    rng = np.random.default_rng(P)
    B = rng.standard_normal((P, P)) / np.sqrt(P)
    A = B @ B.T + 0.5 * np.eye(P)
    got, broke = chol_left(np.tril(A) + np.triu(np.full((P, P), np.nan), 1))  # the upper triangle is never read
    want = np.linalg.cholesky(A)
    assert not broke and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_chol_left_flags_indefinite_and_nan():
    A = np.diag([1.0, -1.0, 1.0, 1.0])
    assert chol_left(A)[1]
    A = np.eye(4)
    A[2, 0] = np.nan
    assert chol_left(A)[1]
    A = np.eye(4)
    A[3, 3] = 0.0  # a zero pivot is not > 0
    assert chol_left(A)[1]
    assert not chol_left(np.eye(4))[1]


def test_ridge():
    cov = torch.arange(9, dtype=torch.float64).reshape(3, 3)
    r = Ridge(1e-3)
    assert torch.equal(r(cov), cov + 1e-3 * torch.eye(3, dtype=torch.float64))
    batch = torch.stack([cov, 2 * cov])
    assert torch.equal(r(batch)[1], 2 * cov + 1e-3 * torch.eye(3, dtype=torch.float64))
    assert r(cov.float()).dtype == torch.float32
    assert torch.equal(Ridge(0)(cov), cov)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            Ridge(bad)


def test_lib_declares_the_entry_points():
    assert "ey_am_step" in L.SYMBOLS and "ey_am_run" in L.SYMBOLS
    lib = L.lib()
    p = ct.c_void_p(1)
    assert lib.ey_am_step(None, p, p, p, p, p, p, p, 0, 0.05, 1.0, 1.0, 0.0, 2, 0, 0, None, None, None, None, 1, 0, 0, 0,
                          0, p, None, None, p, None) == -1
    assert b"null plan" in lib.ey_last_error()
    assert lib.ey_am_run(None, p, p, p, p, p, p, p, 0, 0.05, 1.0, 1.0, 0.0, 2, 0, 0, None, 1, 0, 0, 0, 0, 8, None, None,
                         None, None, p, p, None) == -1
    assert b"ey_am_run" in lib.ey_last_error()


def _am(model, **kw):
    from eeyore_amd.datasets import DataCounter
    return AM(model, counter=DataCounter(1, 1), **kw)


def _small():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[2, 2, 1]))


def test_sampler_rejects_bad_arguments_before_any_launch():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import logistic_regression as lr
    big = lr.LogisticRegression(loss_functions['binary_classification'], hparams=lr.Hyperparameters(input_size=128))
    assert big.num_params() == 129
    with pytest.raises(ValueError, match="at most 128"):
        AM(big)
    small = _small()
    P = small.num_params()
    for t0 in (1, 0, -3, 2.5):
        with pytest.raises(ValueError, match="t0"):
            _am(small, t0=t0)
    for l in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            _am(small, l=l)
    for kw in (dict(b=float("inf")), dict(c=float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            _am(small, **kw)
    with pytest.raises(ValueError, match="eps"):
        _am(small, transform=Ridge(-1.0))
    for shape in ((P,), (P, P + 1), (2, P, P), (P - 1, P - 1)):
        with pytest.raises(ValueError, match="covariance"):
            _am(small, cov0=torch.ones(*shape))
    with pytest.raises(ValueError, match="on_breakdown"):
        _am(small, on_breakdown="ignore")
    with pytest.raises(ValueError, match="transform"):
        _am(small, transform=1e-6)


def test_constructor_transforms_cov0_once():
    small = _small()
    P = small.num_params()
    s = _am(small, transform=Ridge(0.5))
    assert torch.equal(s.cov0.cpu(), 1.5 * torch.eye(P, dtype=s.cov0.dtype)) and s._eps == 0.5 and not s._generic
    s = _am(small, cov0=2 * torch.eye(P), transform=lambda cov: 3 * cov)
    assert torch.equal(s.cov0.cpu(), 6 * torch.eye(P, dtype=s.cov0.dtype)) and s._eps == 0.0 and s._generic
    assert _am(small)._eps == 0.0
