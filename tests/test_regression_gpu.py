"""The regression likelihoods (EY_LIK_GAUSS_SUM, _LAPLACE_SUM, _POISSON_SUM: the likelihood blocks of eval_target and
tiny_rows in eeyore_amd/csrc/ey_generic.hip, k_loss in ey_large.hip) and the network outputs (ey_forward) against the
reference's recorded values and traces (g19_regression_traces.npz) and against torch in f64 on the CPU
(tests/regression_restatement.py).

Tolerances are those tests/test_prior_gpu.py states for the same quantities: values and gradients rtol 1e-10 / atol 1e-11 in
f64 (atol x 10 for the sums), 2e-4 / 2e-4 in f32; trace samples rtol 1e-8 / atol 1e-9.  On the layerwise path ("bgemm") they
are those of tests/test_gpu_parity.py's test_bgemm_path_on_small_models_vs_oracle (f32, either product form: value rtol 2e-4 /
atol 2e-3, gradient rtol 2e-3 / atol 2e-4 max(1, |g|)) and test_bgemm_path_f64_vs_oracle (value 1e-10 / 1e-10, gradient
rtol 1e-9 / atol 1e-11 max(1, |g|))."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from eeyore_amd import _lib as L
from tests import regression_restatement as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
TRACE = dict(rtol=1e-8, atol=1e-9)
SCALE = {"gauss": 0.5, "laplace": 0.8, "poisson": 1.0}
SIGMA = 2.0


def _tol(dtype, sums=False):
    return dict(rtol=1e-10, atol=1e-10 if sums else 1e-11) if dtype == F64 else dict(rtol=2e-4, atol=2e-4)


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


def _plan(dims, acts, loss, x, y, dtype, scale=None, sigma=SIGMA):
    """A plan of a regression code with its data, scale and a N(0, sigma^2) prior."""
    from eeyore_amd.plan import Plan
    pl = Plan(dims, [1] * (len(dims) - 1), acts, rr.CODE[loss], dtype, DEV)
    pl.set_data(_t(x, dtype), _t(y, dtype))
    pl.set_prior(torch.zeros(pl.P), torch.full((pl.P,), sigma))
    if scale is not None and loss != "poisson":
        pl.set_lik_scale(scale)
    return pl


def _target(dims, acts, loss, x, y, dtype, scale=1.0, sigma=SIGMA):
    """The restated target on the data the device holds (f32: rounded)."""
    return rr.Target(dims, acts, loss, _np(_t(x, dtype)), _np(_t(y, dtype)), scale=scale, sigma=sigma)


def _want(tgt, th):
    want = [tgt.parts(t) for t in th]
    return tuple(np.array([w[i] for w in want]) for i in range(4))


G19 = rr.load_g19()


# ------------------------------------------------------------------------------------------------ 1. values and gradients
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("key", sorted(k for k in G19 if k.startswith("values/")))
def test_values_against_the_reference(key, dtype):
    rec = G19[key]
    pl = _plan(rec["dims"].tolist(), rec["acts"].tolist(), rec["loss"], rec["x"], rec["y"], dtype, scale=rec["lik_scale"],
               sigma=rec["sigma"])
    assert pl.kernel == "generic"
    th = _t(rec["theta"], dtype)
    lik, prior = pl.log_target(th)
    tv, gr = pl.log_target_grad(th)
    print(key, "errors: lik", np.abs(_np(lik) - rec["log_lik"]).max(), "prior", np.abs(_np(prior) - rec["log_prior"]).max(),
          "target", np.abs(_np(tv) - rec["log_target"]).max(), "grad", np.abs(_np(gr) - rec["grad"]).max())
    np.testing.assert_allclose(_np(lik), rec["log_lik"], **_tol(dtype, True))
    np.testing.assert_allclose(_np(prior), rec["log_prior"], **_tol(dtype, True))
    np.testing.assert_allclose(_np(tv), rec["log_target"], **_tol(dtype, True))
    np.testing.assert_allclose(_np(gr), rec["grad"], **_tol(dtype))


# name: (dims, activations, rows, row waves, variant of Plan.set_variant): the tiny register path with compile-time extents;
# two outputs and a tanh OUTPUT activation on one partial tile of the LDS tile loop (40 rows: below the 128 from which a
# shape without compile-time extents is evaluated in registers); the same model forced onto the register path with
# run-time extents (variant bit 9), one wave; the LDS tile loop over two full tiles and one of 22 rows (relu hidden layer);
# one row; the row-wave form (the register path with run-time extents, several waves)
GENERIC = {
    "mlp221": ([2, 2, 1], [2, 0], 40, "off", 0),
    "mlp342": ([3, 4, 2], [1, 2], 40, "off", 0),
    "mlp342_tiny": ([3, 4, 2], [1, 2], 40, "off", 512),
    "mlp482": ([4, 8, 2], [3, 0], 150, "off", 0),
    "mlp482_one_row": ([4, 8, 2], [3, 0], 1, "off", 0),
    "mlp231_row_waves": ([2, 3, 1], [2, 0], 150, "on", 0),
}


def _generic_cases():
    for name in GENERIC:
        for C in ([1] if name == "mlp482_one_row" else [1, 11]):
            yield name, C


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("loss", rr.LOSSES)
@pytest.mark.parametrize("name,C", list(_generic_cases()))
def test_generic_values_against_torch(name, C, loss, dtype):
    dims, acts, N, waves, variant = GENERIC[name]
    x, y = rr.synthetic(dims, loss, N, seed=len(name))
    pl = _plan(dims, acts, loss, x, y, dtype, scale=SCALE[loss])
    pl.row_waves = waves
    pl.set_variant(variant)
    assert pl.kernel == "generic"
    rng = np.random.default_rng(10 * pl.P + C)
    th = _t(0.5 * rng.standard_normal((C, pl.P)), dtype)
    temps = _t(0.2 + 0.8 * rng.random(C), dtype)
    tgt = _target(dims, acts, loss, x, y, dtype, scale=SCALE[loss])
    w_lik, w_pri, w_tv, w_gr = _want(tgt, _np(th))
    lik, prior = pl.log_target(th)
    tv, gr = pl.log_target_grad(th)
    rows = pl.log_lik_rows(th)
    print(name, loss, "errors: lik", np.abs(_np(lik) - w_lik).max(), "target", np.abs(_np(tv) - w_tv).max(), "grad",
          np.abs(_np(gr) - w_gr).max())
    np.testing.assert_allclose(_np(lik), w_lik, **_tol(dtype, True))
    np.testing.assert_allclose(_np(prior), w_pri, **_tol(dtype, True))
    np.testing.assert_allclose(_np(tv), w_tv, **_tol(dtype, True))
    np.testing.assert_allclose(_np(gr), w_gr, **_tol(dtype))
    np.testing.assert_allclose(_np(rows), np.array([tgt.rows(t) for t in _np(th)]), **_tol(dtype))
    # a per-chain temperature multiplies everything
    tt = _np(temps)
    tl, tp = pl.log_target(th, temp=temps)
    ttv, tgr = pl.log_target_grad(th, temp=temps)
    np.testing.assert_allclose(_np(tl), tt * w_lik, **_tol(dtype, True))
    np.testing.assert_allclose(_np(tp), tt * w_pri, **_tol(dtype, True))
    np.testing.assert_allclose(_np(ttv), tt * w_tv, **_tol(dtype, True))
    np.testing.assert_allclose(_np(tgr), tt[:, None] * w_gr, **_tol(dtype))
    np.testing.assert_allclose(_np(pl.log_lik_rows(th, temp=temps)), tt[:, None] * _np(rows), **_tol(dtype))


# the layerwise path: where k_tail would have been taken, where k_mid32 would have been, f64 (a sigmoid OUTPUT activation),
# and the two models the fused families would serve under a classification code
BGEMM = {
    "mlp_10_64_2": ([10, 64, 2], [2, 0], F32),
    "mlp_16_32_32_2": ([16, 32, 32, 2], [1, 2, 0], F32),
    "mlp_6_40_2_f64": ([6, 40, 2], [2, 1], F64),
    "mlp_4_32_32_1": ([4, 32, 32, 1], [1, 1, 0], F32),
    "mlp_4_32_32_3": ([4, 32, 32, 3], [1, 1, 0], F32),
}


def _bgemm_close(dtype, got_t, got_g, want_t, want_g):
    gs = max(1.0, np.abs(want_g).max())
    if dtype == F32:
        np.testing.assert_allclose(got_t, want_t, rtol=2e-4, atol=2e-3)
        np.testing.assert_allclose(got_g, want_g, rtol=2e-3, atol=2e-4 * gs)
    else:
        np.testing.assert_allclose(got_t, want_t, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(got_g, want_g, rtol=1e-9, atol=1e-11 * gs)


def _bgemm_cases():
    for name, (_, _, dtype) in BGEMM.items():
        for products in (("bf16x3", "exact") if dtype == F32 else ("exact",)):
            yield name, products


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("loss", rr.LOSSES)
@pytest.mark.parametrize("name,products", list(_bgemm_cases()))
def test_bgemm_values_against_torch(name, products, loss, C):
    dims, acts, dtype = BGEMM[name]
    N = 70
    x, y = rr.synthetic(dims, loss, N, seed=len(name))
    pl = _plan(dims, acts, loss, x, y, dtype, scale=SCALE[loss])
    if dtype == F32:
        pl.f32_products = products
    assert pl.kernel == "bgemm"  # not fused16, mfma32, k_tail or k_mid32: they carry the classification losses only
    rng = np.random.default_rng(pl.P + C)
    th = _t(0.3 * rng.standard_normal((C, pl.P)), dtype)
    temps = _t(0.2 + 0.8 * rng.random(C), dtype)
    tgt = _target(dims, acts, loss, x, y, dtype, scale=SCALE[loss])
    w_lik, w_pri, w_tv, w_gr = _want(tgt, _np(th))
    lik, prior = pl.log_target(th)
    tv, gr = pl.log_target_grad(th)
    ttv, tgr = pl.log_target_grad(th, temp=temps)
    rows = pl.log_lik_rows(th)
    tt = _np(temps)
    print(name, products, loss, "errors: target", np.abs(_np(tv) - w_tv).max(), "grad", np.abs(_np(gr) - w_gr).max())
    for c in range(C):
        _bgemm_close(dtype, _np(tv)[c], _np(gr)[c], w_tv[c], w_gr[c])
        _bgemm_close(dtype, _np(ttv)[c], _np(tgr)[c], tt[c] * w_tv[c], tt[c] * w_gr[c])
        _bgemm_close(dtype, _np(lik)[c], _np(gr)[c], w_lik[c], w_gr[c])
        _bgemm_close(dtype, _np(prior)[c], _np(gr)[c], w_pri[c], w_gr[c])
        _bgemm_close(dtype, _np(rows)[c].sum(), _np(gr)[c], w_lik[c], w_gr[c])
    want_rows = np.array([tgt.rows(t) for t in _np(th)])
    np.testing.assert_allclose(_np(rows), want_rows, **(dict(rtol=2e-4, atol=2e-3) if dtype == F32 else dict(rtol=1e-10, atol=1e-10)))
    # an HMC draw on the separate launches (no k_tail in the trajectory): finite, and a rejected chain keeps its state
    th1, tv1, gr1 = th.clone(), tv.clone(), gr.clone()
    out = pl.hmc_step(th1, tv1, gr1, 0.01, 3, seed=1, it=0)
    acc = out["accepted"].bool()
    assert torch.isfinite(out["h_prop"]).all() and torch.equal(th1[~acc], th[~acc])
    fresh = pl.log_target_grad(th1)[0]
    _bgemm_close(dtype, _np(tv1), 0.0, _np(fresh), 0.0)


# ------------------------------------------------------------------------------------------------ 2. edge inputs
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["mlp221", "mlp482", "mlp_10_64_2"])
def test_laplace_delta_is_zero_where_the_output_equals_the_response(name, dtype):
    """A zero last layer and y = 0: out == y exactly in every row, and sign(0) = 0 -- the likelihood contributes no gradient
    at all, so the gradient of the log-target is the prior's, -theta / sigma^2 (what autograd gives at the kink)."""
    dims, acts = (GENERIC[name][:2] if name in GENERIC else BGEMM[name][:2])
    N = 70
    x, _ = rr.synthetic(dims, "laplace", N)
    y = np.zeros((N, dims[-1]))
    pl = _plan(dims, acts, "laplace", x, y, dtype, scale=0.8)
    assert pl.kernel == ("generic" if name in GENERIC else "bgemm")
    P, C = pl.P, 3
    th = 0.4 * np.random.default_rng(4).standard_normal((C, P))
    last = dims[-2] * dims[-1] + dims[-1]
    th[:, P - last:] = 0.0  # the last layer's weights and bias
    thd = _t(th, dtype)
    assert bool((pl.forward(thd) == 0).all())
    tv, gr = pl.log_target_grad(thd)
    tgt = _target(dims, acts, "laplace", x, y, dtype, scale=0.8)
    _, _, w_tv, w_gr = _want(tgt, _np(thd))
    np.testing.assert_allclose(w_gr, -_np(thd) / SIGMA ** 2, rtol=1e-12, atol=1e-15)  # the restatement agrees
    if name in GENERIC:
        np.testing.assert_allclose(_np(gr), -_np(thd) / SIGMA ** 2, **_tol(dtype))
        np.testing.assert_allclose(_np(tv), w_tv, **_tol(dtype, True))
    else:
        for c in range(C):
            _bgemm_close(dtype, _np(tv)[c], _np(gr)[c], w_tv[c], w_gr[c])
    assert bool((gr[:, P - last:] == 0).all())  # exactly: no row pushes the last layer either way


@pytest.mark.parametrize("name", ["mlp482", "mlp_10_64_2"])
def test_poisson_overflow_gives_a_target_the_accept_step_rejects(name):
    """f32, an output of 100: exp overflows, the row term is -inf, nothing is clamped.  The target is not finite and an HMC
    draw from there rejects, leaving the state alone; the chain beside it is untouched by its neighbour."""
    dims, acts = (GENERIC[name][:2] if name in GENERIC else BGEMM[name][:2])
    N = 70
    x, y = rr.synthetic(dims, "poisson", N)
    pl = _plan(dims, acts, "poisson", x, y, F32)
    P, C = pl.P, 2
    th = 0.1 * np.random.default_rng(5).standard_normal((C, P))
    th[0, P - dims[-1]:] = 100.0  # the output bias of chain 0
    thd = _t(th, F32)
    out_ = pl.forward(thd)
    assert bool((out_[0] > 88.8).all()) and bool((out_[1].abs() < 5).all())
    lik, _ = pl.log_target(thd)
    tv, gr = pl.log_target_grad(thd)
    assert not np.isfinite(_np(lik)[0]) and not np.isfinite(_np(tv)[0]) and np.isfinite(_np(tv)[1])
    w_tv = _target(dims, acts, "poisson", x, y, F32).log_target(_np(thd)[1])
    np.testing.assert_allclose(_np(tv)[1], w_tv, rtol=2e-4, atol=2e-3)
    th1, tv1, gr1 = thd.clone(), tv.clone(), gr.clone()
    o = pl.hmc_step(th1, tv1, gr1, 0.01, 3, seed=2, it=0)
    torch.cuda.synchronize()
    assert int(o["accepted"][0]) == 0 and torch.equal(th1[0], thd[0])
    assert torch.isfinite(th1[1]).all() and torch.isfinite(tv1[1])


def test_the_scale_is_validated_and_enters_the_value():
    from eeyore_amd.plan import Plan
    dims, acts, N = GENERIC["mlp221"][:3]
    x, y = rr.synthetic(dims, "gauss", N)
    th = _t(0.5 * np.random.default_rng(0).standard_normal((3, 9)), F64)
    for loss in ("gauss", "laplace"):
        pl = _plan(dims, acts, loss, x, y, F64)
        assert pl.lik_scale == 1.0  # the default
        np.testing.assert_allclose(_np(pl.log_target(th)[0]), _want(_target(dims, acts, loss, x, y, F64), _np(th))[0],
                                   **_tol(F64, True))
        pl.set_lik_scale(0.37)
        assert pl.lik_scale == 0.37
        want = _want(_target(dims, acts, loss, x, y, F64, scale=0.37), _np(th))[0]
        np.testing.assert_allclose(_np(pl.log_target(th)[0]), want, **_tol(F64, True))
        for bad in (0.0, -2.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="finite and > 0"):
                pl.set_lik_scale(bad)
        assert pl.lik_scale == 0.37
        np.testing.assert_allclose(_np(pl.log_target(th)[0]), want, **_tol(F64, True))
    for code in (L.EY_LIK_BCE_SUM, L.EY_LIK_CE_SUM, L.EY_LIK_POISSON_SUM):
        pl = Plan(dims, [1, 1], acts, code, F64, DEV)
        with pytest.raises(ValueError, match="likelihood scale"):
            pl.set_lik_scale(2.0)
        assert pl.lik_scale == 1.0
    with pytest.raises(ValueError, match="unknown likelihood"):
        Plan(dims, [1, 1], acts, 5, F64, DEV)


# ------------------------------------------------------------------------------------------------ 3. the reference's traces
@pytest.mark.parametrize("loss", rr.LOSSES)
def test_fixture_replay(loss):
    rec = G19[f"trace/{loss}"]
    pl = _plan(rec["dims"].tolist(), rec["acts"].tolist(), loss, rec["x"], rec["y"], F64, scale=rec["lik_scale"],
               sigma=rec["sigma"])
    th = _t(rec["theta0"], F64)[None].clone()
    tv = _t([rec["init_target"]], F64)
    gr = _t(rec["init_grad"], F64)[None].clone()
    kind = rec["sampler"]
    t0, g0 = pl.log_target_grad(th)  # the start is the reference's own
    np.testing.assert_allclose(_np(t0), _np(tv), **_tol(F64, True))
    if kind != "mh":
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


# ------------------------------------------------------------------------------------------------ 4. every sampler
@pytest.mark.parametrize("sampler", rr.SAMPLERS)
def test_every_sampler_on_a_gaussian_likelihood(sampler):
    d = rr.sampler_case(sampler)
    par = d["par"]
    pl = _plan(rr.S_DIMS, rr.S_ACTS, "gauss", d["x"], d["y"], F64, scale=d["lik_scale"], sigma=d["sigma"])
    assert pl.kernel == "generic"
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
        tb = pl.gibbs_table(rr.S_BLOCKS, [par["scale"]] * len(rr.S_BLOCKS))
    left_out = 0
    for it in range(steps):
        z, u = _t(d["z"][it], F64), _t(d["u"][it], F64)
        if sampler == "hmc":
            out = pl.hmc_step(th, tv, gr, par["step"], par["L"], p0=z, u=u)
        elif sampler == "mala":
            out = pl.mala_step(th, tv, gr, par["step"], z=z, u=u)
        elif sampler == "mh":
            out = pl.mh_step(th, tv, par["scale"], z=z, u=u)
        elif sampler == "ram":
            out = pl.ram_step(th, tv, chol, it + 1, a=par["a"], g=par["g"], z=z, u=u)
        elif sampler == "am":
            out = pl.am_step(th, tv, mean, cs, cov, nacc, c0, it, l=par["l"], b=par["b"], c=par["c"], eps=par["eps"],
                             t0=par["t0"], offset=0, z=z, u_mix=_t(d["u_mix"][it], F64), u=u, breakdowns=bd)
            assert np.array_equal(out["branch"].cpu().numpy(), d["branch"][it]), it
        else:
            out = pl.gibbs_step(th, tv, tb, z=z, u=u, mode="intended")
        clear = d["margin"][it] > 1e-9
        left_out += int((~clear).sum())
        acc = out["accepted"].cpu().numpy()
        assert np.array_equal(acc[clear], d["accepted"][it][clear]), (it, acc, d["accepted"][it])
        np.testing.assert_allclose(_np(th), d["theta"][it], **TRACE)
        np.testing.assert_allclose(_np(tv), d["target"][it], **TRACE)
    assert left_out <= 1
    if sampler == "am":
        assert int(bd.sum()) == 0


def _regression_model(loss, dtype, dims=(2, 3, 1), N=40):
    """models.mlp.MLP on synthetic rows with a N(0, 2^2) prior, its data set and loader, and the restated target."""
    from torch.utils.data import DataLoader

    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.models import mlp
    dims = list(dims)
    name = {2: "gauss", 3: "laplace", 4: "poisson"}[loss.code]
    x, y = rr.synthetic(dims, name, N, seed=7)
    data = XYDataset(_t(x, dtype), _t(y, dtype))
    m = mlp.MLP(loss=loss, hparams=mlp.Hyperparameters(dims=dims, bias=2 * [True], activations=[torch.tanh, None]),
                dtype=dtype, device=DEV)
    P = m.num_params()
    m.prior = Normal(torch.zeros(P, dtype=dtype, device=DEV), torch.full((P,), SIGMA, dtype=dtype, device=DEV))
    tgt = _target(dims, [2, 0], name, x, y, dtype, scale=loss.scale or 1.0)
    return m, data, DataLoader(data, batch_size=len(data), shuffle=False), tgt


def test_power_posterior_on_the_device_under_a_gaussian_likelihood():
    """By the properties tests/test_prior_gpu.py holds the device ladder to: finite states, acceptance strictly between 0 and
    1, and every recorded target equal to a fresh log_target of the recorded sample times the temperature."""
    from eeyore_amd.constants import gaussian_loss
    from eeyore_amd.samplers import PowerPosteriorSampler
    m, data, loader, _ = _regression_model(gaussian_loss(0.5), F32)
    P = m.num_params()
    K, R = 3, 4
    th0 = 0.1 * torch.randn(R, P, generator=torch.Generator().manual_seed(1)).to(DEV)
    s = PowerPosteriorSampler(m, loader, [['MALA', {'step': 0.004}] for _ in range(K)], theta0=th0, between_step=5, seed=2,
                              keys=['sample', 'target_val', 'accepted'], between='device')
    s.run(num_epochs=40, num_burnin_epochs=0)
    plan = m._plan(data.x, data.y)
    assert plan.kernel == "generic" and plan.lik_scale == 0.5
    rates = []
    for k in range(K):
        chain = s.get_chain(k)
        smp, tvs = chain.get_samples(), chain.get_target_vals()
        assert smp.shape == (40, R, P) and torch.isfinite(smp).all()
        want = torch.stack([m.log_target(smp[i].contiguous(), data.x, data.y) for i in range(smp.shape[0])])
        np.testing.assert_allclose(_np(tvs), s.temperature[k] * _np(want), **_tol(F32, True))
        rates.append(chain.get_accepted().float().mean().item())
    print("MALA ladder under a Gaussian likelihood: acceptance per temperature", rates)
    assert 0.0 < np.mean(rates) < 1.0


# ------------------------------------------------------------------------------------------------ 5. the closed form
def test_linear_gaussian_posterior_end_to_end():
    """A one-layer plan with an identity output under a Gaussian likelihood and a Normal prior has a Gaussian posterior in
    closed form (tests/regression_restatement.py: linear_gaussian).  512 seeded HMC chains, 100 burn-in and 300 kept draws:
    every pooled mean within 5 standard errors of the exact one (the chains are independent: the standard error is the
    standard deviation of the 512 chain means / sqrt(512)), every pooled variance within 10 % of the exact one -- with at
    least 10^4 effective draws the relative standard error of a variance is sqrt(2 / 10^4) = 1.4 %, so 10 % is seven of
    them; the run's effective sample size is checked first."""
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.plan import Plan
    x, y, mean, cov = rr.linear_gaussian()
    pl = Plan([3, 1], [1], [0], L.EY_LIK_GAUSS_SUM, F64, DEV)
    pl.set_data(_t(x, F64), _t(y, F64))
    pl.set_prior(torch.zeros(4), torch.full((4,), 2.0))
    pl.set_lik_scale(0.7)
    C, burn, keep = 512, 100, 300
    th = _t(0.1 * np.random.default_rng(0).standard_normal((C, 4)), F64)
    tv, gr = pl.log_target_grad(th)
    tv, gr = tv.contiguous(), gr.contiguous()
    step, nsteps = rr.CLOSED_FORM_STEP, rr.CLOSED_FORM_L
    count = torch.zeros(C, dtype=torch.int32, device=DEV)
    pl.hmc_run(th, tv, gr, step, nsteps, burn, seed=11, it=0)
    buf = ChainBuffer()
    blk = buf.block(keep, dict(sample=th, target_val=tv, accepted=torch.zeros(C, dtype=torch.uint8, device=DEV)))
    pl.hmc_run(th, tv, gr, step, nsteps, keep, seed=11, it=burn, samples=blk["sample"], targets=blk["target_val"],
               accepted_rec=blk["accepted"], accept_count=count)
    buf.commit(keep)
    rate = count.double().mean().item() / keep
    smp = buf.get_samples()
    assert smp.shape == (keep, C, 4) and torch.isfinite(smp).all()
    ess = _np(buf.ess()).sum(0)  # per parameter, summed over the chains
    pooled = _np(smp).reshape(-1, 4)
    chain_means = _np(smp).mean(0)
    se = chain_means.std(0, ddof=1) / np.sqrt(C)
    print("closed form: acceptance", rate, "ESS per parameter", ess, "mean error / se", (pooled.mean(0) - mean) / se,
          "variance ratio", pooled.var(0, ddof=1) / np.diag(cov))
    assert 0.6 <= rate <= 0.95
    assert (ess > 1e4).all(), ess
    assert (np.abs(pooled.mean(0) - mean) < 5 * se).all()
    np.testing.assert_allclose(pooled.var(0, ddof=1), np.diag(cov), rtol=0.10)


# ------------------------------------------------------------------------------------------------ 6. the network outputs
# the tiny path; the LDS tile loop (three tiles); a wide model in f32 (the generic image still holds it); the row-wave form;
# a model beyond the generic kernels' LDS, through the layerwise forward products
FORWARD = {
    "mlp221": ([2, 2, 1], [2, 0], 40, F64, "off"),
    "mlp482": ([4, 8, 2], [3, 0], 150, F64, "off"),
    "mlp482_f32": ([4, 8, 2], [3, 0], 150, F32, "off"),
    "mlp_10_64_2": ([10, 64, 2], [2, 0], 70, F32, "off"),
    "mlp231_row_waves": ([2, 3, 1], [2, 0], 150, F64, "on"),
    "mlp_10_200_2_beyond_lds": ([10, 200, 2], [2, 1], 70, F32, "off"),
    "mlp_10_200_2_beyond_lds_f64": ([10, 200, 2], [2, 1], 70, F64, "off"),
}


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_against_torch(name, C):
    dims, acts, N, dtype, waves = FORWARD[name]
    x, y = rr.synthetic(dims, "gauss", N, seed=3)
    pl = _plan(dims, acts, "gauss", x, y, dtype)
    pl.row_waves = waves
    th = _t(0.4 * np.random.default_rng(C).standard_normal((C, pl.P)), dtype)
    out = pl.forward(th)
    assert out.shape == (C, N, dims[-1]) and out.dtype == dtype
    tgt = _target(dims, acts, "gauss", x, y, dtype)
    want = np.array([tgt.outputs(t) for t in _np(th)])
    print(name, "largest output error", np.abs(_np(out) - want).max())
    np.testing.assert_allclose(_np(out), want, **_tol(dtype))
    # the outputs are those the likelihood is evaluated on
    rows = Normal(out.double(), 1.0).log_prob(_t(y, dtype).double()).sum(2)
    np.testing.assert_allclose(_np(pl.log_lik_rows(th)), _np(rows), **(_tol(dtype) if pl.kernel == "generic" or dtype == F64
                                                                       else dict(rtol=2e-4, atol=2e-3)))


def test_forward_on_a_plan_the_fused_kernel_serves():
    """MLP(4-32-32-3) under CE-sum is mfma32's: ey_forward goes through the generic value kernel, returns the logits, and
    leaves the plan's routing alone."""
    from eeyore_amd.plan import Plan
    dims, acts = [4, 32, 32, 3], [1, 1, 0]
    rng = np.random.default_rng(0)
    x = rng.standard_normal((150, 4))
    y = np.eye(3)[rng.integers(0, 3, 150)]
    pl = Plan(dims, [1, 1, 1], acts, L.EY_LIK_CE_SUM, F32, DEV)
    pl.set_data(_t(x, F32), _t(y, F32))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    assert pl.kernel == "mfma32"
    th = _t(0.3 * rng.standard_normal((5, pl.P)), F32)
    before = pl.log_target_grad(th)
    out = pl.forward(th)
    assert pl.kernel == "mfma32"
    tgt = rr.pr.Target(dims, acts, 1, _np(_t(x, F32)), _np(_t(y, F32)), None)
    want = np.array([tgt.forward(torch.tensor(t)).numpy() for t in _np(th)])
    np.testing.assert_allclose(_np(out), want, **_tol(F32))
    after = pl.log_target_grad(th)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # BCE-sum on a sigmoid output: probabilities
    pb = Plan([4, 8, 1], [1, 1], [2, 1], L.EY_LIK_BCE_SUM, F64, DEV)
    yb = (rng.random((150, 1)) < 0.5).astype(np.float64)
    pb.set_data(_t(x, F64), _t(yb, F64))
    pb.set_prior(torch.zeros(pb.P), torch.ones(pb.P))
    thb = _t(0.5 * rng.standard_normal((3, pb.P)), F64)
    prob = pb.forward(thb)
    assert bool(((prob > 0) & (prob < 1)).all())
    want_rows = (prob.log() * _t(yb, F64) + (1 - prob).log() * (1 - _t(yb, F64))).sum(2)
    np.testing.assert_allclose(_np(pb.log_lik_rows(thb)), _np(want_rows), **_tol(F64))


def test_forward_refusals():
    from eeyore_amd.plan import Plan
    mix = Plan.mixture(np.zeros(1), np.zeros((1, 2)), np.eye(2)[None], F64, DEV)
    mix.dims, mix.N = [1, 1], 1
    with pytest.raises(ValueError, match="mixture plan has no network"):
        mix.forward(torch.zeros(2, 2, dtype=F64, device=DEV))
    bare = Plan([2, 2, 1], [1, 1], [2, 0], L.EY_LIK_GAUSS_SUM, F64, DEV)
    bare.N = 1
    with pytest.raises(RuntimeError, match="ey_plan_set_data has not been called"):
        bare.forward(torch.zeros(2, 9, dtype=F64, device=DEV))


def test_predict_batched_and_the_predictive_density():
    from eeyore_amd.constants import gaussian_loss
    s = 0.6
    m, data, _, tgt = _regression_model(gaussian_loss(s), F64)
    P = m.num_params()
    S, K = 12, 9
    rng = np.random.default_rng(8)
    samples = _t(0.5 * rng.standard_normal((S, P)), F64)
    xg, yg = _t(rng.standard_normal((K, 2)), F64), _t(rng.standard_normal((K, 1)), F64)
    # the model's surface is the restated target
    np.testing.assert_allclose(_np(m.log_target(samples, data.x, data.y)), _want(tgt, _np(samples))[2], **_tol(F64, True))
    assert m._plan(data.x, data.y).lik_scale == s and m._plan(data.x, data.y).kernel == "generic"
    out = m._plan(xg, yg).forward(samples)  # [S, K, 1]
    mean, sd, dropped = m.predict_batched(samples, xg)
    assert mean.shape == (K, 1) and sd.shape == (K, 1) and dropped.shape == (K,) and int(dropped.sum()) == 0
    np.testing.assert_allclose(_np(mean), _np(out.mean(0)), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(_np(sd), _np(out.std(0, unbiased=True)), rtol=1e-12, atol=1e-14)
    # a list of [P] samples is accepted, as predictive_posterior_batched accepts it
    mean_l, _, _ = m.predict_batched(list(samples.unbind(0)), xg)
    assert torch.equal(mean_l, mean)
    # a sample with a NaN parameter is dropped at every point, and counted
    bad = samples.clone()
    bad[5, 0] = float("nan")
    mean_b, sd_b, dropped_b = m.predict_batched(bad, xg)
    keep = [i for i in range(S) if i != 5]
    assert dropped_b.tolist() == [1] * K
    np.testing.assert_allclose(_np(mean_b), _np(out[keep].mean(0)), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(_np(sd_b), _np(out[keep].std(0, unbiased=True)), rtol=1e-12, atol=1e-14)
    # the predictive density of y: the mean over the samples of Normal(out, s).pdf(y), correctly normalised
    est, dr = m.predictive_posterior_batched(samples, xg, yg)
    want = Normal(out, s).log_prob(yg[None]).sum(2).exp().mean(0)
    np.testing.assert_allclose(_np(est), _np(want), **_tol(F64))
    assert int(dr.sum()) == 0
    # ... and the Laplace form's
    from eeyore_amd.constants import laplace_loss
    from torch.distributions import Laplace
    ml, _, _, _ = _regression_model(laplace_loss(s), F64)
    est_l, _ = ml.predictive_posterior_batched(samples, xg, yg)
    out_l = ml._plan(xg, yg).forward(samples)
    np.testing.assert_allclose(_np(est_l), _np(Laplace(out_l, s).log_prob(yg[None]).sum(2).exp().mean(0)), **_tol(F64))
    # one-dimensional quadrature of the Gaussian predictive density at one x: it integrates to 1
    grid = torch.linspace(-12, 12, 2001, dtype=F64, device=DEV).reshape(-1, 1)
    dens, _ = m.predictive_posterior_batched(samples, xg[:1].expand(grid.shape[0], 2).contiguous(), grid)
    np.testing.assert_allclose(float(torch.trapezoid(dens, grid[:, 0])), 1.0, rtol=1e-8)


# ------------------------------------------------------------------------------------------------ the example
def test_example_runs():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="40", EEYORE_EXAMPLE_CHAINS="32", PYTHONPATH=root)
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "sinusoid_regression_hmc.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mean acceptance rate" in out.stdout and "predictive mean" in out.stdout
    assert "samples dropped for a non-finite output: 0" in out.stdout
