"""Laplace, Student-t and Cauchy priors in the generic kernels (the tail of eval_target in eeyore_amd/csrc/ey_generic.hip,
ey_plan_set_prior_family) against the reference's recorded values and traces (g18_prior_traces.npz) and against
torch.distributions in f64 on the CPU (tests/prior_restatement.py).

Tolerances are those tests/test_gpu_parity.py uses for the same quantities under a Normal prior: values and gradients rtol
1e-10 / atol 1e-11 in f64 (atol x 10 for the sums), 2e-4 / 2e-4 in f32; trace samples rtol 1e-8 / atol 1e-9."""
import numpy as np
import pytest
import torch
from torch.distributions import Cauchy, Laplace, StudentT

from eeyore_amd import _lib as L
from tests import prior_restatement as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
FAMILY = {"laplace": L.EY_PRIOR_LAPLACE, "studentt": L.EY_PRIOR_STUDENT_T, "cauchy": L.EY_PRIOR_STUDENT_T}
TRACE = dict(rtol=1e-8, atol=1e-9)


def _tol(dtype, sums=False):
    return dict(rtol=1e-10, atol=1e-10 if sums else 1e-11) if dtype == F64 else dict(rtol=2e-4, atol=2e-4)


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


def _plan(dims, acts, lik, x, y, dtype):
    from eeyore_amd.plan import Plan
    pl = Plan(dims, [1] * (len(dims) - 1), acts, lik, dtype, DEV)
    if x is not None:
        pl.set_data(_t(x, dtype), _t(y, dtype))
    return pl


def _set(pl, family, loc, scale, df=None):
    """Uploads the family's tables; returns them as the device holds them (f32: rounded), in f64 numpy."""
    lo, sc = _t(loc, pl.dtype), _t(scale, pl.dtype)
    d = None if family == "laplace" else torch.ones_like(sc) if family == "cauchy" else _t(df, pl.dtype)
    pl.set_prior_family(FAMILY[family], lo, sc, d)
    assert pl.prior_family == FAMILY[family] and pl.kernel == "generic"
    return _np(lo), _np(sc), None if family != "studentt" else _np(d)


def _data(dims, lik, N, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, dims[0]))
    if lik == 0:
        y = (rng.random((N, dims[-1])) < 0.5).astype(np.float64)
    else:
        y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    return x, y


G18 = pr.load_g18()


# ------------------------------------------------------------------------------------------------ 1. values and gradients
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("key", sorted(k for k in G18 if k.startswith("values/")))
def test_values_against_the_reference(key, dtype):
    rec = G18[key]
    pl = _plan(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], dtype)
    _set(pl, rec["family"], rec["loc"], rec["scale"], rec.get("df"))
    th = _t(rec["theta"], dtype)
    lik, prior = pl.log_target(th)
    tv, gr = pl.log_target_grad(th)
    print(key, "errors: lik", np.abs(_np(lik) - rec["log_lik"]).max(), "prior", np.abs(_np(prior) - rec["log_prior"]).max(),
          "target", np.abs(_np(tv) - rec["log_target"]).max(), "grad", np.abs(_np(gr) - rec["grad"]).max())
    np.testing.assert_allclose(_np(lik), rec["log_lik"], **_tol(dtype, True))
    np.testing.assert_allclose(_np(prior), rec["log_prior"], **_tol(dtype, True))
    np.testing.assert_allclose(_np(tv), rec["log_target"], **_tol(dtype, True))
    np.testing.assert_allclose(_np(gr), rec["grad"], **_tol(dtype))


# (dims, activations, likelihood, rows): the tiny register path; the smallest plan; one partial lane pass; a full lane pass
# plus a partial one; exactly one full pass (63 inputs and a bias)
CASES = {
    "mlp221": ([2, 2, 1], [1, 1], 0, 40),
    "lr5": ([4, 1], [1], 0, 40),
    "mlp433": ([4, 3, 3], [1, 0], 1, 150),
    "mlp483": ([4, 8, 3], [1, 0], 1, 150),
    "lr64": ([63, 1], [1], 0, 40),
}


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("family", pr.FAMILIES)
@pytest.mark.parametrize("name", list(CASES))
def test_values_against_torch(name, family, dtype, C):
    dims, acts, lik, N = CASES[name]
    x, y = _data(dims, lik, N)
    pl = _plan(dims, acts, lik, x, y, dtype)
    P = pl.P
    assert P == {"mlp221": 9, "lr5": 5, "mlp433": 27, "mlp483": 67, "lr64": 64}[name]
    loc, scale, df = _set(pl, family, *pr.distinct_tables(P, P))
    rng = np.random.default_rng(10 * P + C)
    th = _t((0.1 if name == "lr64" else 0.5) * rng.standard_normal((C, P)), dtype)
    temps = _t(0.2 + 0.8 * rng.random(C), dtype)
    xd, yd = _np(_t(x, dtype)), _np(_t(y, dtype))  # what the device holds
    tgt = pr.Target(dims, acts, lik, xd, yd, pr.make_prior(family, loc, scale, df))
    want = [tgt.parts(t) for t in _np(th)]
    w_lik, w_pri, w_tv = (np.array([w[i] for w in want]) for i in range(3))
    w_gr = np.array([w[3] for w in want])
    lik_, prior = pl.log_target(th)
    tv, gr = pl.log_target_grad(th)
    np.testing.assert_allclose(_np(lik_), w_lik, **_tol(dtype, True))
    np.testing.assert_allclose(_np(prior), w_pri, **_tol(dtype, True))
    np.testing.assert_allclose(_np(tv), w_tv, **_tol(dtype, True))
    np.testing.assert_allclose(_np(gr), w_gr, **_tol(dtype))
    # a per-chain temperature multiplies everything
    tl, tp = pl.log_target(th, temp=temps)
    ttv, tgr = pl.log_target_grad(th, temp=temps)
    tt = _np(temps)
    np.testing.assert_allclose(_np(tl), tt * _np(lik_), **_tol(dtype, True))
    np.testing.assert_allclose(_np(tp), tt * _np(prior), **_tol(dtype, True))
    np.testing.assert_allclose(_np(ttv), tt * _np(tv), **_tol(dtype, True))
    np.testing.assert_allclose(_np(tgr), tt[:, None] * _np(gr), **_tol(dtype))
    np.testing.assert_allclose(_np(tp), tt * w_pri, **_tol(dtype, True))
    # the prior alone, on a plan that has no data
    bare = _plan(dims, acts, lik, None, None, dtype)
    _set(bare, family, loc, scale, df)
    assert torch.equal(bare.log_target(th, prior_only=True)[1], prior)
    assert torch.equal(bare.log_target(th, temp=temps, prior_only=True)[1], tp)


@pytest.mark.parametrize("family", pr.FAMILIES)
def test_row_waves_give_the_same_prior(family):
    dims, acts, lik = CASES["mlp221"][:3]
    x, y = _data(dims, lik, 128)
    res = {}
    for mode in ("off", "on"):
        pl = _plan(dims, acts, lik, x, y, F64)
        pl.row_waves = mode
        _set(pl, family, *pr.distinct_tables(pl.P, 3))
        th = _t(0.5 * np.random.default_rng(2).standard_normal((11, pl.P)), F64)
        res[mode] = pl.log_target(th) + pl.log_target_grad(th)
    (l0, p0, t0, g0), (l1, p1, t1, g1) = res["off"], res["on"]
    assert torch.equal(p0, p1)  # the prior's sum does not depend on the waves
    np.testing.assert_allclose(_np(l1), _np(l0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(_np(t1), _np(t0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(_np(g1), _np(g0), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. edge inputs
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["mlp221", "mlp483"])
def test_laplace_gradient_at_the_kink_is_the_likelihood_gradient(name, dtype):
    dims, acts, lik, N = CASES[name]
    x, y = _data(dims, lik, N)
    pl = _plan(dims, acts, lik, x, y, dtype)
    P, C = pl.P, 3
    loc, scale, _ = _set(pl, "laplace", *pr.distinct_tables(P, 11))
    th = _np(_t(0.4 * np.random.default_rng(4).standard_normal((C, P)), dtype))
    at = [0, P // 2, P - 1]  # also the last parameter: the lane the idle lanes of a partial pass repeat
    th[:, at] = loc[at]
    tv, gr = pl.log_target_grad(_t(th, dtype))
    tgt = pr.Target(dims, acts, lik, _np(_t(x, dtype)), _np(_t(y, dtype)), Laplace(torch.tensor(loc), torch.tensor(scale)))
    for c in range(C):
        _, _, w_tv, w_gr = tgt.parts(th[c])
        np.testing.assert_allclose(_np(gr)[c], w_gr, **_tol(dtype))
        np.testing.assert_allclose(_np(gr)[c, at], tgt.lik_grad(th[c])[at], **_tol(dtype))
        np.testing.assert_allclose(_np(tv)[c], w_tv, **_tol(dtype, True))
    assert torch.isfinite(gr).all() and torch.isfinite(tv).all()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_student_t_far_out_and_with_one_degree_of_freedom(dtype):
    dims, acts, lik, N = CASES["mlp433"]
    x, y = _data(dims, lik, N)
    pl = _plan(dims, acts, lik, x, y, dtype)
    P = pl.P
    loc0, scale0, df0 = pr.distinct_tables(P, 12)
    th = np.zeros((2, P))
    for df_in, dist in ((df0, None), (np.ones(P), Cauchy)):
        loc, scale, df = _set(pl, "studentt", loc0, scale0, df_in)
        th[0] = loc + 1e3 * scale * np.where(np.arange(P) % 2 == 0, 1.0, -1.0)  # |d| / s = 1e3 at every parameter
        th[1] = loc + 1e-3 * scale
        thd = _t(th, dtype)
        prior = pl.log_target(thd, prior_only=True)[1]
        tv, gr = pl.log_target_grad(thd)
        prior_d = StudentT(torch.tensor(df), torch.tensor(loc), torch.tensor(scale)) if dist is None else \
            dist(torch.tensor(loc), torch.tensor(scale))
        tgt = pr.Target(dims, acts, lik, _np(_t(x, dtype)), _np(_t(y, dtype)), prior_d)
        assert torch.isfinite(prior).all() and torch.isfinite(gr).all()
        for c in range(2):
            _, w_pri, w_tv, w_gr = tgt.parts(_np(thd)[c])
            np.testing.assert_allclose(_np(prior)[c], w_pri, **_tol(dtype, True))
            if np.isfinite(w_tv):  # (the likelihood of a point 1e3 scales out may have saturated: the prior is the subject)
                np.testing.assert_allclose(_np(tv)[c], w_tv, **_tol(dtype, True))
                np.testing.assert_allclose(_np(gr)[c], w_gr, **_tol(dtype))


# ------------------------------------------------------------------------------------------------ 3. the reference's traces
@pytest.mark.parametrize("family", pr.FAMILIES)
def test_fixture_replay(family):
    rec = G18[f"trace/{family}"]
    pl = _plan(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], F64)
    _set(pl, family, rec["loc"], rec["scale"], rec.get("df"))
    th = _t(rec["theta0"], F64)[None].clone()
    tv = _t([rec["init_target"]], F64)
    gr = _t(rec["init_grad"], F64)[None].clone()
    kind = rec["sampler"]
    if kind != "mh":  # the start is the reference's own
        t0, g0 = pl.log_target_grad(th)
        np.testing.assert_allclose(_np(t0), _np(tv), **_tol(F64, True))
        np.testing.assert_allclose(_np(g0), _np(gr), **_tol(F64))
    for it in range(rec["z"].shape[0]):
        z, u = _t(rec["z"][it], F64)[None], _t([rec["u"][it]], F64)
        if kind == "hmc":
            out = pl.hmc_step(th, tv, gr, float(rec["step"]), int(rec["L"]), p0=z, u=u)
        elif kind == "mala":
            out = pl.mala_step(th, tv, gr, float(rec["step"]), z=z, u=u)
        else:
            out = pl.mh_step(th, tv, float(rec["scale_mh"]), z=z, u=u)
        assert int(out["accepted"].item()) == int(rec["accepted"][it]), it
        np.testing.assert_allclose(_np(th)[0], rec["sample"][it], **TRACE)
        np.testing.assert_allclose(tv.item(), rec["target_val"][it], **TRACE)
    assert 0 < rec["accepted"].sum() < len(rec["accepted"])


# ------------------------------------------------------------------------------------------------ 4. the other generic samplers
@pytest.mark.parametrize("family", ["laplace", "studentt", "cauchy"])
@pytest.mark.parametrize("sampler", pr.OTHER_SAMPLERS)
def test_the_other_generic_samplers(sampler, family):
    d = pr.other_case(sampler, family)
    par = d["par"]
    pl = _plan(pr.OTHER_DIMS, pr.OTHER_ACTS, pr.OTHER_LIK, d["x"], d["y"], F64)
    _set(pl, family, d["loc"], d["scale"], d["df"])
    steps, C, P = d["z"].shape
    th = _t(d["th0"], F64)
    tv, gr = pl.log_target_grad(th)
    tv, gr = tv.contiguous(), gr.contiguous()
    if sampler == "ram":
        chol = _t(np.stack([par["chol0"] * np.eye(P)] * C), F64)
    elif sampler == "am":
        mean, cs = torch.zeros(C, P, dtype=F64, device=DEV), torch.zeros(C, P, P, dtype=F64, device=DEV)
        c0 = _t(par["cov0"] * np.eye(P), F64)
        cov = c0[None].repeat(C, 1, 1).contiguous()
        nacc, bd = (torch.zeros(C, dtype=torch.int32, device=DEV) for _ in range(2))
    elif sampler == "gibbs":
        tb = pl.gibbs_table(pr.OTHER_BLOCKS, [par["scale"]] * len(pr.OTHER_BLOCKS))
    else:
        tril = _t(d["L"], F64)
    left_out = 0
    for it in range(steps):
        z, u = _t(d["z"][it], F64), _t(d["u"][it], F64)
        if sampler == "ram":
            out = pl.ram_step(th, tv, chol, it + 1, a=par["a"], g=par["g"], z=z, u=u)
        elif sampler == "am":
            out = pl.am_step(th, tv, mean, cs, cov, nacc, c0, it, l=par["l"], b=par["b"], c=par["c"], eps=par["eps"],
                             t0=par["t0"], offset=0, z=z, u_mix=_t(d["u_mix"][it], F64), u=u, breakdowns=bd)
            assert np.array_equal(out["branch"].cpu().numpy(), d["branch"][it]), it
        elif sampler == "gibbs":
            out = pl.gibbs_step(th, tv, tb, z=z, u=u, mode="intended")
        elif sampler == "mh_tril":
            out = pl.mh_tril_step(th, tv, tril, z=z, u=u)
        else:
            out = pl.mala_tril_step(th, tv, gr, par["step"], tril, z=z, u=u)
        clear = d["margin"][it] > 1e-9
        left_out += int((~clear).sum())
        acc = out["accepted"].cpu().numpy()
        assert np.array_equal(acc[clear], d["accepted"][it][clear]), (it, acc, d["accepted"][it])
        np.testing.assert_allclose(_np(th), d["theta"][it], **TRACE)
        np.testing.assert_allclose(_np(tv), d["target"][it], **TRACE)
    assert left_out <= 1
    if sampler == "am":
        assert int(bd.sum()) == 0


# ------------------------------------------------------------------------------------------------ 5. routing
def test_routing_follows_the_prior_family():
    dims, acts, lik = [4, 32, 32, 3], [1, 1, 0], 1
    x, y = _data(dims, lik, 150)
    pl = _plan(dims, acts, lik, x, y, F32)
    P = pl.P
    mu, sigma = torch.zeros(P), torch.full((P,), 1.5)
    pl.set_prior(mu, sigma)
    assert pl.kernel == "mfma32" and pl.prior_family == L.EY_PRIOR_NORMAL
    th = _t(0.2 * np.random.default_rng(0).standard_normal((5, P)), F32)
    before = pl.log_target_grad(th)
    loc, scale, _ = _set(pl, "laplace", *pr.distinct_tables(P, 1))
    assert pl.kernel == "generic"
    tv, gr = pl.log_target_grad(th)
    tgt = pr.Target(dims, acts, lik, _np(_t(x, F32)), _np(_t(y, F32)), Laplace(torch.tensor(loc), torch.tensor(scale)))
    for c in range(th.shape[0]):
        _, _, w_tv, w_gr = tgt.parts(_np(th)[c])
        np.testing.assert_allclose(_np(tv)[c], w_tv, **_tol(F32, True))
        np.testing.assert_allclose(_np(gr)[c], w_gr, **_tol(F32))
    # EY_PRIOR_NORMAL through the new entry point is ey_plan_set_prior
    pl.set_prior_family(L.EY_PRIOR_NORMAL, mu, sigma)
    assert pl.kernel == "mfma32" and pl.prior_family == L.EY_PRIOR_NORMAL
    again = pl.log_target_grad(th)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])
    _set(pl, "cauchy", loc, scale)
    pl.set_prior(mu, sigma)
    assert pl.kernel == "mfma32"
    again = pl.log_target_grad(th)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])


def test_a_model_beyond_lds_is_refused_before_any_launch():
    from eeyore_amd.plan import _stream
    dims, acts, lik = [784, 128, 10], [1, 0], 1
    x, y = _data(dims, lik, 64)
    pl = _plan(dims, acts, lik, x, y, F32)
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    assert pl.kernel == "bgemm"
    pl.set_prior_family(L.EY_PRIOR_LAPLACE, torch.zeros(pl.P), torch.ones(pl.P))
    assert pl.kernel == "generic"
    C = 2
    th = torch.zeros(C, pl.P, dtype=F32, device=DEV)
    tv = torch.full((C,), -7.0, dtype=F32, device=DEV)
    gr = torch.full((C, pl.P), 0.5, dtype=F32, device=DEV)
    rc = L.lib().ey_log_target_grad(pl.handle, L.ptr(th), None, C, L.ptr(tv), L.ptr(gr), _stream(pl.device))
    msg = L.lib().ey_last_error().decode()
    assert rc == -2 and "Laplace" in msg and "generic kernels" in msg, msg
    torch.cuda.synchronize()
    assert bool((tv == -7.0).all()) and bool((gr == 0.5).all())
    for call in (lambda: pl.log_target_grad(th), lambda: pl.log_target(th), lambda: pl.log_target(th, prior_only=True),
                 lambda: pl.hmc_step(th, tv, gr, 0.01, 2), lambda: pl.mala_step(th, tv, gr, 0.01),
                 lambda: pl.mh_step(th, tv, 0.1)):
        with pytest.raises(RuntimeError, match="Laplace prior is served only for models the generic kernels can hold"):
            call()
    torch.cuda.synchronize()
    assert bool((tv == -7.0).all()) and bool((gr == 0.5).all()) and bool((th == 0).all())
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))  # a Normal prior again: the layerwise kernels serve it
    assert pl.kernel == "bgemm" and torch.isfinite(pl.log_target_grad(th)[0]).all()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_invalid_tables_are_refused_and_leave_the_prior_alone(dtype):
    dims, acts, lik, N = CASES["mlp433"]
    x, y = _data(dims, lik, N)
    pl = _plan(dims, acts, lik, x, y, dtype)
    P = pl.P
    loc, scale, df = pr.distinct_tables(P, 2)
    _set(pl, "studentt", loc, scale, df)
    th = _t(0.3 * np.random.default_rng(1).standard_normal((3, P)), dtype)
    before = pl.log_target_grad(th)

    def bad(a, i, v):
        a = np.array(a)
        a[i] = v
        return a
    for fam, lo, sc, d, word in (("laplace", loc, bad(scale, 3, 0.0), None, "scale"),
                                 ("laplace", loc, bad(scale, 0, -1.0), None, "scale"),
                                 ("laplace", loc, bad(scale, P - 1, np.inf), None, "scale"),
                                 ("studentt", loc, scale, bad(df, 5, -1.0), "df"),
                                 ("studentt", loc, scale, bad(df, 5, np.nan), "df"),
                                 ("studentt", bad(loc, 7, np.nan), scale, df, "loc"),
                                 ("laplace", bad(loc, 7, np.inf), scale, None, "loc")):
        with pytest.raises(ValueError, match=word):
            pl.set_prior_family(FAMILY[fam], _t(lo, dtype), _t(sc, dtype), None if d is None else _t(d, dtype))
    with pytest.raises(ValueError, match="family"):
        pl.set_prior_family(7, _t(loc, dtype), _t(scale, dtype))
    with pytest.raises(ValueError, match="df"):
        pl.set_prior_family(L.EY_PRIOR_STUDENT_T, _t(loc, dtype), _t(scale, dtype))
    assert pl.prior_family == L.EY_PRIOR_STUDENT_T
    after = pl.log_target_grad(th)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ------------------------------------------------------------------------------------------------ 6. the sampler surface
def _iris(dtype):
    from torch.utils.data import DataLoader

    from eeyore_amd.datasets import XYDataset
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=dtype, device=DEV)
    return iris, DataLoader(iris, batch_size=len(iris), shuffle=False)


def _mlp483(prior_of):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    m = mlp.MLP(loss=loss_functions['multiclass_classification'],
                hparams=mlp.Hyperparameters(dims=[4, 8, 3], bias=2 * [True], activations=[torch.sigmoid, None]),
                dtype=F32, device=DEV)
    P = m.num_params()
    loc, scale, _ = pr.distinct_tables(P, 5)
    m.prior = prior_of(torch.tensor(loc, dtype=F32, device=DEV), torch.tensor(scale, dtype=F32, device=DEV))
    return m, P


def test_hmc_run_under_a_cauchy_prior():
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.samplers import HMC
    iris, loader = _iris(F32)
    m, P = _mlp483(Cauchy)
    C = 64
    th0 = 0.1 * torch.randn(C, P, generator=torch.Generator().manual_seed(0)).to(DEV)
    s = HMC(m, theta0=th0, dataloader=loader, step=0.02, num_steps=5, seed=1,
            chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    assert s._can_fuse(False)
    s.run(num_epochs=40, num_burnin_epochs=0)
    plan = m._plan(iris.x, iris.y)
    assert plan.kernel == "generic" and plan.prior_family == L.EY_PRIOR_STUDENT_T
    chain = s.get_chain()
    smp, tvs = chain.get_samples(), chain.get_target_vals()
    assert smp.shape == (40, C, P) and torch.isfinite(smp).all()
    want = torch.stack([m.log_target(smp[i].contiguous(), iris.x, iris.y) for i in range(smp.shape[0])])
    np.testing.assert_allclose(_np(tvs), _np(want), **_tol(F32, True))
    rate = chain.get_accepted().float().mean().item()
    print("HMC under a Cauchy prior: acceptance", rate)
    assert 0.0 < rate < 1.0
    # the summary names the prior
    assert "Cauchy" in str(m.prior)


def test_power_posterior_on_the_device_under_a_laplace_prior():
    from eeyore_amd.samplers import PowerPosteriorSampler
    iris, loader = _iris(F32)
    m, P = _mlp483(Laplace)
    K, R = 3, 4
    th0 = 0.1 * torch.randn(R, P, generator=torch.Generator().manual_seed(1)).to(DEV)
    s = PowerPosteriorSampler(m, loader, [['MALA', {'step': 0.002}] for _ in range(K)], theta0=th0, between_step=5, seed=2,
                              keys=['sample', 'target_val', 'accepted'], between='device')
    s.run(num_epochs=40, num_burnin_epochs=0)
    plan = m._plan(iris.x, iris.y)
    assert plan.kernel == "generic" and plan.prior_family == L.EY_PRIOR_LAPLACE
    rates = []
    for k in range(K):
        chain = s.get_chain(k)
        smp, tvs = chain.get_samples(), chain.get_target_vals()
        assert smp.shape == (40, R, P) and torch.isfinite(smp).all()
        want = torch.stack([m.log_target(smp[i].contiguous(), iris.x, iris.y) for i in range(smp.shape[0])])
        np.testing.assert_allclose(_np(tvs), s.temperature[k] * _np(want), **_tol(F32, True))
        rates.append(chain.get_accepted().float().mean().item())
    print("MALA ladder under a Laplace prior: acceptance per temperature", rates)
    assert 0.0 < np.mean(rates) < 1.0


# ------------------------------------------------------------------------------------------------ the example
def test_example_runs():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="40", EEYORE_EXAMPLE_CHAINS="32", PYTHONPATH=root)
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "iris_laplace_prior.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Laplace prior (generic kernels): mean acceptance rate" in out.stdout and "share of posterior means" in out.stdout
