"""RAM without a GPU: the numpy restatement against the reference's own traces (tests/golden/g11_ram_traces.npz),
the closed-form factor update the kernel implements against the full re-factorisation, and argument errors."""
import ctypes as ct

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests.helpers import load
from tests.ram_restatement import closed_form_update, ram_draw, refactorised, spec_target


def _groups():
    z = load("g11_ram_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abcd"}


@pytest.mark.parametrize("name", list("abcd"))
def test_restatement_reproduces_reference_traces(name):
    rec = _groups()[name]
    tf = spec_target(rec)
    th, tv = rec["theta0"].copy(), float(rec["init_target"])
    assert abs(tf(th) - tv) <= 1e-12 * max(1.0, abs(tv))
    chol = np.linalg.cholesky(rec["cov0"])
    k = 0
    for it in range(rec["z"].shape[0]):
        th, tv, chol, acc, _ = ram_draw(tf, th, tv, chol, rec["z"][it], rec["u"][it], int(rec["n"][it]),
                                        float(rec["a"]), float(rec["g"]))
        assert acc == bool(rec["accepted"][it]), it
        np.testing.assert_allclose(th, rec["sample"][it], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(tv, rec["target_val"][it], rtol=1e-12)
        if k < len(rec["chol_it"]) and rec["chol_it"][k] == it:
            np.testing.assert_allclose(chol, rec["chol"][k], rtol=1e-12, atol=1e-12)
            k += 1
    assert k == len(rec["chol_it"])


def test_fixture_groups_mix_accepts_and_rejects():
    for name, rec in _groups().items():
        acc = rec["accepted"]
        assert 0 < acc.sum() < len(acc), name
    assert (_groups()["d"]["n"] == np.arange(6, 46)).all()  # counter.idx 10.. with offset 5


@pytest.mark.parametrize("P", [1, 2, 5, 64, 128])
@pytest.mark.parametrize("beta", [-0.234, 0.766, -0.1, 0.3])
def test_closed_form_update_equals_refactorisation(P, beta):
    rng = np.random.default_rng(P)
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    S = np.linalg.cholesky(A @ A.T + np.eye(P))
    z = rng.standard_normal(P)
    want = refactorised(S, z, beta)
    got = closed_form_update(S, z, beta)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_closed_form_cannot_break_down():
    # t_k >= 1 - a > 0 whatever z: the extreme beta = -a with all of |z| in the first coordinate
    a = 0.999
    z = np.zeros(8)
    z[0] = 3.0
    S = closed_form_update(np.eye(8), z, -a)
    assert np.isfinite(S).all() and S[0, 0] == pytest.approx(np.sqrt(1 - a))


def test_ram_import_and_argument_errors_without_gpu():
    from eeyore_amd.samplers import RAM  # noqa: F401
    lib = L.lib()
    acc = ct.c_void_p(1)
    assert lib.ey_ram_step(None, acc, acc, acc, None, None, 0.234, 0.7, 1, None, 1, 0, 0, 0, 0, acc, None, None) == -1
    assert b"null plan" in lib.ey_last_error()
    assert lib.ey_ram_run(None, acc, acc, acc, 0.234, 0.7, 1, None, 1, 0, 0, 0, 0, 8, None, None, None, None, acc,
                          None) == -1
    assert b"ey_ram_run" in lib.ey_last_error()


def test_sampler_rejects_out_of_range_arguments_before_any_launch():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import RAM
    hp = mlp.Hyperparameters(dims=[6, 14, 2, 1])
    big = mlp.MLP(loss=loss_functions['binary_classification'], hparams=hp)
    assert big.num_params() > 128
    with pytest.raises(ValueError, match="at most 128"):
        RAM(big)
    small = mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=[2, 2, 1]))
    for a in (0.0, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            RAM(small, a=a)
    with pytest.raises(ValueError, match="finite"):
        RAM(small, g=float("nan"))
