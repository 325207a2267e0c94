"""Exponential-tilt targets on the device (ey_plan_create_exptilt, tilt_target in eeyore_amd/csrc/ey_generic.hip) against the
numpy restatement (tests/exptilt_restatement.py), the reference's own traces (g20_exptilt_traces.npz) and itself: the cases of
tests/test_dist_gpu.py on the new plan.

Tolerances are the generic family's as tests/test_dist_gpu.py states them: f64 rtol 1e-9 on values and log-rates, 1e-8 on
states; f32 F32_DECISION_TOL = 2e-3, rtol 2e-4 on values, 1e-5 on states, against the restatement on the f32-rounded inputs.
On a value or a gradient the tolerance is relative to S = sum_i (|c_i| + |a_i theta_i| + |b_i exp(s_i theta_i)|), the size of
the terms the value is summed from, not to the value: terms of both signs cancel (the f32 lane pass over 128 terms errs by
about 128 x 6e-8 x S = 8e-6 x S, far inside 2e-4 x S)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dist_restatement as dr
from tests import exptilt_restatement as er
from tests.am_restatement import am_draw
from tests.mala_mvn_restatement import mala_mvn_draw
from tests.mh_mvn_restatement import mh_mvn_draw
from tests.ram_restatement import adapt_h, alpha_of, ram_draw, refactorised
from tests.test_dist_host import replay
from tests.test_exptilt_host import TRACES, g20, target_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_DECISION_TOL = 2e-3  # as tests/test_dist_gpu.py
SHAPES = [1, 2, 63, 64, 65, 128]  # one lane, a partial wave, the edges of the first lane pass, two full passes
STEP_SHAPES = [1, 65, 128]
DTYPES = [torch.float64, torch.float32]
SAMPLERS = ["hmc", "mala", "mh", "ram", "am", "mh_tril", "mala_tril"]


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


def _rounded(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == torch.float32 else a


@functools.lru_cache(maxsize=None)
def _tables(P):
    return er.random_tilt(P, seed=100 + P)


def _plan(P, dtype):
    """(plan, tables as the device holds them: rounded once to the plan's dtype)."""
    from eeyore_amd.plan import Plan
    tab = _tables(P)
    pl = Plan.exp_tilt(*tab, dtype, DEV)
    assert pl.kernel == "dist" and pl.P == P
    return pl, tuple(_rounded(t, dtype) for t in tab)


def _points(P, C, seed, big):
    """C points mode + 0.7 z / |s|; when C > 2 row 1 has one coordinate at s theta = big (its exp overflows), row 2 a NaN,
    row 3 one coordinate at s theta = -800 (its exp underflows to 0)."""
    tab = _tables(P)
    s = tab[3]
    rng = np.random.default_rng(seed)
    th = er.mode(tab) + 0.7 * rng.standard_normal((C, P)) / np.abs(s)
    k = P // 2
    if C > 2:
        th[1, k] = big / s[k]
        th[2, k] = np.nan
        th[3, k] = -800 / s[k]
    return th, k


# ------------------------------------------------------------------------------------------------ value and gradient
@pytest.mark.parametrize("temp", [False, True], ids=["plain", "tempered"])
@pytest.mark.parametrize("C", [11, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("P", SHAPES)
def test_value_and_gradient_against_the_restatement(P, dtype, C, temp):
    pl, tab = _plan(P, dtype)
    f64 = dtype == torch.float64
    pts, k = _points(P, C, seed=P + C, big=800.0 if f64 else 100.0)
    th = _t(pts, dtype)
    tt = _t(0.2 + 0.8 * np.random.default_rng(5).random(C), dtype) if temp else None
    lik, prior = pl.log_target(th, temp=tt)
    tv, gr = pl.log_target_grad(th, temp=tt)
    assert (prior == 0).all()
    rtol = 1e-9 if f64 else 2e-4
    th0, lik, tv, gr = _np(th), _np(lik), _np(tv), _np(gr)
    sk = tab[3][k]
    for ch in range(C):
        v, g, S = er.tilt_value_grad(*tab, th0[ch], None if tt is None else float(_np(tt)[ch]))
        with np.errstate(invalid="ignore"):
            g_err = np.abs(np.where(np.isfinite(g), gr[ch] - g, 0.0)).max()
        print(f"P={P} chain {ch}: value {tv[ch]:.9g} (restatement {v:.9g}), S {S:.4g}, gradient error {g_err:.3g}")
        if C > 2 and ch == 1:  # the overflow: -inf, an infinite component of the right sign, no NaN anywhere
            assert lik[ch] == -np.inf and tv[ch] == -np.inf
            assert v == -np.inf or not f64  # (exp(100) overflows f32 alone: the f64 restatement of that row is finite)
            assert not np.isnan(gr[ch]).any() and np.isinf(gr[ch][k]) and np.sign(gr[ch][k]) == -np.sign(sk)
            rest = np.arange(P) != k  # the other coordinates: their own terms' size
            if rest.any():
                S_rest = er.tilt_value_grad(*(t[rest] for t in tab), th0[ch][rest])[2]
                assert np.all(np.abs(gr[ch][rest] - g[rest]) <= rtol * S_rest)
            continue
        if C > 2 and ch == 2:  # the NaN
            assert np.isnan(v) and np.isnan(lik[ch]) and np.isnan(tv[ch]) and np.isnan(gr[ch][k])
            continue
        assert np.isfinite(v) and np.isfinite(g).all()
        assert abs(lik[ch] - v) <= rtol * S and abs(tv[ch] - v) <= rtol * S
        assert np.all(np.abs(gr[ch] - g) <= rtol * S)
        if C > 2 and ch == 3:  # the underflow: the component is the table's a, bit for bit
            want = torch.tensor(tab[1][k], dtype=dtype)
            if tt is not None:
                want = want * tt[ch].cpu()  # one rounded product in the plan's dtype, as the kernel forms it
            assert gr[ch][k] == want.item()


# ------------------------------------------------------------------------------------------------ one recorded-random step
# per P: HMC step, MALA step, MH scale, factor scale (RAM, AM, the two MultivariateNormalKernel proposals)
PAR = {1: (0.5, 0.3, 0.8, 0.5), 65: (0.06, 0.02, 0.08, 0.06), 128: (0.04, 0.01, 0.06, 0.04)}
L_HMC, N_RAM, A_RAM, G_RAM = 3, 7, 0.234, 0.7
AM = dict(idx=20, offset=2, t0=6, l=0.25, eps=1e-3)
# seeds for which the restatement's own |log u - log_rate| (HMC: |u - rate|) exceeds ten times the decision tolerance of both
# dtypes for every chain of every sampler (searched on the CPU: find_seed below)
SEEDS = {(1, 11): 4, (1, 1): 0, (65, 11): 3, (65, 1): 0, (128, 11): 3, (128, 1): 0}


def _spd(C, P, rng, scale):
    out = np.empty((C, P, P))
    for ch in range(C):
        A = rng.standard_normal((P, P)) / np.sqrt(P)
        S = A @ A.T + 0.5 * np.eye(P)
        out[ch] = scale * (S + S.T) / 2
    return out


def _step_inputs(P, C, seed):
    tab = _tables(P)
    rng = np.random.default_rng(seed)
    sc = PAR[P][3]
    d = dict(th=er.mode(tab) + 0.7 * rng.standard_normal((C, P)) / np.abs(tab[3]), z=rng.standard_normal((C, P)),
             u=rng.random(C), um=rng.random(C), chol=np.linalg.cholesky(_spd(C, P, rng, sc * sc)),
             cov=_spd(C, P, rng, sc * sc), cov0=_spd(C, P, rng, sc * sc), mean=0.1 * rng.standard_normal((C, P)))
    d["cs"] = np.einsum("ci,cj->cij", d["th"], d["th"]) * (AM["idx"] - AM["offset"])
    return d


def _want(sampler, tab, P, d, ch, target, grad):
    """The restatement's draw of chain ch from the given start: (theta, target, accepted, decision margin, log_rate or
    rate, extras)."""
    vg = er.tilt_value_grad_fn(*tab)
    tf = er.tilt_target_fn(*tab)
    hs, ms, mhs, sc = PAR[P]
    th, z, u = d["th"][ch], d["z"][ch], float(d["u"][ch])
    if sampler == "hmc":
        o = dr.hmc_draw(vg, th, target, grad, z, u, hs, L_HMC)
        return o[0], o[1], o[3], abs(u - o[4]), o[4], o[2]
    if sampler == "mala":
        o = dr.mala_draw(vg, th, target, grad, z, u, ms)
        return o[0], o[1], o[3], abs(np.log(u) - o[4]), o[4], o[2]
    if sampler == "mh":
        o = dr.mh_draw(tf, th, target, z, u, mhs)
        return o[0], o[1], o[2], abs(np.log(u) - o[3]), o[3], None
    if sampler == "ram":
        o = ram_draw(tf, th, target, d["chol"][ch], z, u, N_RAM, A_RAM, G_RAM)
        return o[0], o[1], o[3], abs(np.log(u) - o[4]), o[4], o[2]
    if sampler == "mh_tril":
        o = mh_mvn_draw(tf, th, target, d["chol"][ch], z, u)
        return o[0], o[1], o[2], abs(np.log(u) - o[3]), o[3], None
    if sampler == "mala_tril":
        o = mala_mvn_draw(vg, th, target, grad, d["chol"][ch], z, u, ms)
        return o[0], o[1], o[3], abs(np.log(u) - o[4]), o[4], o[2]
    o = am_draw(tf, th, target, d["mean"][ch], d["cs"][ch], d["cov"][ch], 3, d["cov0"][ch], z, d["um"][ch], u, AM["idx"],
                AM["offset"], AM["l"], 2.38 / np.sqrt(P), sc, AM["t0"], AM["eps"])
    return o["theta"], o["target"], o["accepted"], abs(np.log(u) - o["log_rate"]), o["log_rate"], o


def _decision_tol(f32, dec):
    return F32_DECISION_TOL * max(1.0, abs(dec)) if f32 else 1e-9


def _margins(P, C, seed, f32):
    """The smallest decision margin over the samplers and chains, relative to the decision tolerance (CPU only)."""
    tab = tuple(_rounded(t, torch.float32 if f32 else torch.float64) for t in _tables(P))
    d = _step_inputs(P, C, seed)
    if f32:
        d = {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}
    worst = np.inf
    for ch in range(C):
        t0, g0 = er.tilt_value_grad(*tab, d["th"][ch])[:2]
        for s in SAMPLERS:
            o = _want(s, tab, P, d, ch, t0, g0)
            worst = min(worst, o[3] / _decision_tol(f32, o[4]))
    return worst


def find_seed(P, C):
    """The first seed whose margins exceed twelve decision tolerances in both dtypes (how SEEDS was made): ten are asserted,
    and the test starts from the device's own value and gradient, which differ from the restatement's by their rounding."""
    return next(s for s in range(1000) if min(_margins(P, C, s, True), _margins(P, C, s, False)) > 12)


@pytest.mark.parametrize("C", [11, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("P", STEP_SHAPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_one_step_against_the_restatement(sampler, P, dtype, C):
    pl, tab = _plan(P, dtype)
    f64 = dtype == torch.float64
    d = _step_inputs(P, C, SEEDS[(P, C)])
    dev = {k: _t(v, dtype) for k, v in d.items()}
    d = {k: _np(v) for k, v in dev.items()}  # the restatement starts from the values the device holds (f32: rounded)
    th = dev["th"]
    tv, gr = pl.log_target_grad(th)
    tv0, gr0 = _np(tv), _np(gr)
    hs, ms, mhs, sc = PAR[P]
    if sampler == "hmc":
        out = pl.hmc_step(th, tv, gr, hs, L_HMC, p0=dev["z"], u=dev["u"])
        dec = _np(out["rate"])
    elif sampler == "mala":
        out = pl.mala_step(th, tv, gr, ms, z=dev["z"], u=dev["u"])
    elif sampler == "mh":
        out = pl.mh_step(th, tv, mhs, z=dev["z"], u=dev["u"])
    elif sampler == "ram":
        out = pl.ram_step(th, tv, dev["chol"], N_RAM, a=A_RAM, g=G_RAM, z=dev["z"], u=dev["u"])
    elif sampler == "mh_tril":
        out = pl.mh_tril_step(th, tv, dev["chol"], z=dev["z"], u=dev["u"])
    elif sampler == "mala_tril":
        out = pl.mala_tril_step(th, tv, gr, ms, dev["chol"], z=dev["z"], u=dev["u"])
    else:
        nacc = torch.full((C,), 3, dtype=torch.int32, device=DEV)
        out = pl.am_step(th, tv, dev["mean"], dev["cs"], dev["cov"], nacc, dev["cov0"], AM["idx"], l=AM["l"],
                         b=2.38 / np.sqrt(P), c=sc, eps=AM["eps"], t0=AM["t0"], offset=AM["offset"], z=dev["z"],
                         u_mix=dev["um"], u=dev["u"])
        assert (out["breakdowns"] == 0).all()
    if sampler != "hmc":
        dec = _np(out["log_rate"])
    acc, th1, tv1 = out["accepted"].cpu().numpy(), _np(th), _np(tv)
    for ch in range(C):
        w_th, w_tv, w_acc, margin, w_dec, extra = _want(sampler, tab, P, d, ch, float(tv0[ch]), gr0[ch])
        S = er.tilt_value_grad(*tab, w_th)[2]
        tol = _decision_tol(not f64, w_dec)
        assert margin > 10 * tol, (ch, margin, tol)  # the seed was chosen so: no chain is left undecided
        np.testing.assert_allclose(dec[ch], w_dec, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
        assert bool(acc[ch]) == w_acc, (ch, w_dec)
        np.testing.assert_allclose(th1[ch], w_th, rtol=1e-8 if f64 else 1e-5, atol=1e-8 if f64 else 1e-5)
        assert abs(tv1[ch] - w_tv) <= (1e-9 if f64 else 2e-4) * S
        if sampler in ("hmc", "mala", "mala_tril") and w_acc:
            assert np.all(np.abs(_np(gr)[ch] - extra) <= (1e-8 if f64 else 2e-4) * S)
        if sampler == "ram":
            beta = adapt_h(P, N_RAM, G_RAM) * (alpha_of(w_dec if f64 else np.float32(dec[ch])) - A_RAM)
            want = refactorised(d["chol"][ch], d["z"][ch], beta)
            assert np.linalg.norm(_np(dev["chol"])[ch] - want) / np.linalg.norm(want) <= (1e-12 if f64 else 1e-5)
        if sampler == "am":
            assert out["branch"][ch].item() == extra["branch"]
            np.testing.assert_allclose(_np(dev["mean"])[ch], extra["mean"], rtol=1e-8 if f64 else 1e-5,
                                       atol=1e-8 if f64 else 1e-5)


# ------------------------------------------------------------------------------------------------ overflow is a rejection
@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_an_overflowing_proposal_is_rejected(dtype, C):
    P = 5
    pl, tab = _plan(P, dtype)
    f64 = dtype == torch.float64
    big = 800.0 if f64 else 100.0
    th = _t(_step_inputs_small(P, C), dtype)
    tv, _ = pl.log_target_grad(th)
    assert torch.isfinite(tv).all()
    th_before, tv_before = th.clone(), tv.clone()
    k, scale = 2, 0.5
    z = np.random.default_rng(7).standard_normal((C, P))
    z[:, k] = (big / tab[3][k] - _np(th)[:, k]) / scale  # the proposal's coordinate k lands at s theta' = big
    out = pl.mh_step(th, tv, scale, z=_t(z, dtype), u=_t(np.full(C, 0.5), dtype))
    assert (out["accepted"] == 0).all()
    assert (out["log_rate"] == -float("inf")).all()
    assert torch.equal(th.view(torch.uint8), th_before.view(torch.uint8))
    assert torch.equal(tv.view(torch.uint8), tv_before.view(torch.uint8))


def _step_inputs_small(P, C):
    tab = _tables(P)
    return er.mode(tab) + 0.3 * np.random.default_rng(1).standard_normal((C, P)) / np.abs(tab[3])


# ------------------------------------------------------------------------------------------------ run vs step
# per P: HMC step, MALA step, MH scale, factor scale at which the restatement accepts between a fifth and four fifths of its
# proposals from such starts, so that the 77 draws below hold accepts and rejects
RUN_PAR = {1: (0.55, 0.5, 2.5, 2.0), 65: (0.35, 0.12, 0.2, 0.15), 128: (0.3, 0.09, 0.1, 0.1)}


def _start(pl, C, P, dtype, seed=3):
    th = _t(_step_inputs(P, C, seed)["th"], dtype)
    tv, gr = pl.log_target_grad(th)
    return th, tv, gr


@pytest.mark.parametrize("P,dtype", [(1, torch.float64), (65, torch.float32), (128, torch.float32)])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_run_equals_steps_bit_for_bit(sampler, P, dtype):
    pl, _ = _plan(P, dtype)
    C, K = 11, 7
    hs, ms, mhs, sc = RUN_PAR[P]
    th_a, tv_a, gr_a = _start(pl, C, P, dtype)
    th_b, tv_b, gr_b = th_a.clone(), tv_a.clone(), gr_a.clone()
    rec = dict(samples=torch.empty(K, C, P, dtype=dtype, device=DEV), targets=torch.empty(K, C, dtype=dtype, device=DEV),
               accepted_rec=torch.empty(K, C, dtype=torch.uint8, device=DEV),
               accept_count=torch.zeros(C, dtype=torch.int32, device=DEV))
    kw = dict(seed=9, it=11)
    extra_a = extra_b = ()
    eye = torch.eye(P, dtype=dtype, device=DEV)
    tril = (sc * (eye + 0.1 * torch.tril(torch.ones(P, P, dtype=dtype, device=DEV), -1) / P)).contiguous()
    if sampler == "mala_tril":  # MALA's own scale sqrt(step) on the same shape of factor
        tril = (tril * (np.sqrt(ms) / sc)).contiguous()
    if sampler == "ram":
        extra_a = ((sc * eye).expand(C, P, P).contiguous(),)
        extra_b = (extra_a[0].clone(),)
    if sampler == "am":
        def state():
            e = (sc * sc * eye).expand(C, P, P).contiguous()
            return (torch.zeros(C, P, dtype=dtype, device=DEV), torch.zeros(C, P, P, dtype=dtype, device=DEV), e.clone(),
                    torch.zeros(C, dtype=torch.int32, device=DEV), e[0].clone().contiguous())
        extra_a, extra_b = state(), state()
        amkw = dict(l=0.25, b=2.38 / np.sqrt(P), c=sc, eps=1e-3, t0=3)
    if sampler == "hmc":
        pl.hmc_run(th_a, tv_a, gr_a, hs, L_HMC, K, **kw, **rec)
    elif sampler == "mala":
        pl.mala_run(th_a, tv_a, gr_a, ms, K, **kw, **rec)
    elif sampler == "mh":
        pl.mh_run(th_a, tv_a, mhs, K, **kw, **rec)
    elif sampler == "ram":
        pl.ram_run(th_a, tv_a, extra_a[0], 3, K, **kw, **rec)
    elif sampler == "mh_tril":
        pl.mh_tril_run(th_a, tv_a, tril, K, **kw, **rec)
    elif sampler == "mala_tril":
        pl.mala_tril_run(th_a, tv_a, gr_a, ms, tril, K, **kw, **rec)
    else:
        pl.am_run(th_a, tv_a, *extra_a, 0, K, **amkw, **kw, **rec)
    for k in range(K):
        kk = dict(seed=9, it=11 + k)
        if sampler == "hmc":
            out = pl.hmc_step(th_b, tv_b, gr_b, hs, L_HMC, **kk)
        elif sampler == "mala":
            out = pl.mala_step(th_b, tv_b, gr_b, ms, **kk)
        elif sampler == "mh":
            out = pl.mh_step(th_b, tv_b, mhs, **kk)
        elif sampler == "ram":
            out = pl.ram_step(th_b, tv_b, extra_b[0], 3 + k, **kk)
        elif sampler == "mh_tril":
            out = pl.mh_tril_step(th_b, tv_b, tril, **kk)
        elif sampler == "mala_tril":
            out = pl.mala_tril_step(th_b, tv_b, gr_b, ms, tril, **kk)
        else:
            out = pl.am_step(th_b, tv_b, *extra_b, k, **amkw, **kk)
        assert torch.equal(rec["samples"][k], th_b) and torch.equal(rec["targets"][k], tv_b), k
        assert torch.equal(rec["accepted_rec"][k], out["accepted"]), k
    assert torch.equal(th_a, th_b) and torch.equal(tv_a, tv_b)
    if sampler in ("hmc", "mala", "mala_tril"):
        assert torch.equal(gr_a, gr_b)
    for a, b in zip(extra_a, extra_b):
        assert torch.equal(a, b)
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0))
    print(f"{sampler} P={P}: {int(rec['accept_count'].sum())} accepts of {C * K}")
    assert 0 < int(rec["accept_count"].sum()) < C * K


# ------------------------------------------------------------------------------------------------ the reference's traces
@pytest.mark.parametrize("name,sampler", TRACES)
def test_reference_traces_through_the_c_abi(name, sampler):
    from eeyore_amd.plan import Plan
    tab, _, recs = g20()[name]
    rec = recs[sampler]
    f64 = torch.float64
    pl = Plan.exp_tilt(*tab, f64, DEV)
    P = pl.P
    th = _t(rec["theta0"], f64)[None].clone()
    tv, gr = pl.log_target_grad(th)
    np.testing.assert_allclose(tv.item(), float(rec["init_target"]), rtol=1e-9)
    if sampler == "ram":
        chol = _t(np.linalg.cholesky(rec["cov0"]), f64)[None].contiguous()
    if sampler == "am":
        st = (torch.zeros(1, P, dtype=f64, device=DEV), torch.zeros(1, P, P, dtype=f64, device=DEV),
              _t(rec["cov0"], f64)[None].contiguous(), torch.zeros(1, dtype=torch.int32, device=DEV), _t(rec["cov0"], f64))
    for it in range(rec["z"].shape[0]):
        z, u = _t(rec["z"][it], f64)[None], _t([rec["u"][it]], f64)
        if sampler == "hmc":
            out = pl.hmc_step(th, tv, gr, float(rec["step"]), int(rec["L"]), p0=z, u=u)
        elif sampler == "mala":
            out = pl.mala_step(th, tv, gr, float(rec["step"]), z=z, u=u)
        elif sampler == "mh":
            out = pl.mh_step(th, tv, float(rec["scale"]), z=z, u=u)
        elif sampler == "ram":
            out = pl.ram_step(th, tv, chol, int(rec["n"][it]), a=float(rec["a"]), g=float(rec["g"]), z=z, u=u)
        else:
            um = None if np.isnan(rec["u_mix"][it]) else _t([rec["u_mix"][it]], f64)
            out = pl.am_step(th, tv, *st, int(rec["idx"][it]), l=float(rec["l"]), b=float(rec["b"]), c=float(rec["c"]),
                             eps=float(rec["eps"]), t0=int(rec["t0"]), z=z, u_mix=um, u=u)
        assert int(out["accepted"].item()) == int(rec["accepted"][it]), it
        np.testing.assert_allclose(_np(th)[0], rec["sample"][it], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(tv.item(), float(rec["target_val"][it]), rtol=1e-9)
    if sampler == "ram":
        np.testing.assert_allclose(_np(chol)[0], rec["chol"], rtol=1e-8, atol=1e-9)
    if sampler == "am":
        np.testing.assert_allclose(np.tril(_np(st[2])[0]), rec["cov"], rtol=1e-8, atol=1e-9)


# ------------------------------------------------------------------------------------------------ the sampler surface
def _model(name, dtype, temperature=None):
    from eeyore_amd.models import DistributionModel
    tab, args, _ = g20()[name]
    tgt = target_of(name, args)
    return DistributionModel(tgt, tgt.P, temperature=temperature, dtype=dtype, device=DEV), tab


def _loader():
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    return DataLoader(EmptyXYDataset())


KEYS = ['sample', 'target_val', 'accepted']


def test_single_chain_samplers_and_tuner_run():
    from eeyore_amd.samplers import AM, HMC, MALA, RAM, MetropolisHastings
    from eeyore_amd.tuners import HMCDATuner
    torch.manual_seed(1)
    th0 = torch.tensor([-1.0], dtype=torch.float64)
    for make in (lambda m: HMC(m, theta0=th0, dataloader=_loader(), step=0.5, num_steps=3),
                 lambda m: HMC(m, theta0=th0, dataloader=_loader(), tuner=HMCDATuner(1.5)),
                 lambda m: MALA(m, theta0=th0, dataloader=_loader(), step=0.25),
                 lambda m: MetropolisHastings(m, theta0=th0, dataloader=_loader()),
                 lambda m: RAM(m, theta0=th0, dataloader=_loader()),
                 lambda m: AM(m, theta0=th0, dataloader=_loader())):
        m, tab = _model("u", torch.float64)
        s = make(m)
        assert m._plan().kernel == "dist"
        s.run(num_epochs=40, num_burnin_epochs=10)
        smp = torch.stack(list(s.get_chain().get_samples())) if not torch.is_tensor(s.get_chain().get_samples()) \
            else s.get_chain().get_samples()
        assert smp.shape == (30, 1) and torch.isfinite(smp).all()
        want = er.tilt_value_grad(*tab, _np(s.current['sample']))[0]
        np.testing.assert_allclose(float(s.current['target_val']), want, rtol=1e-9)
        assert torch.equal(m.get_params().detach(), s.current['sample'])


def _pps(between, fused_block, R=3):
    from eeyore_amd.samplers import PowerPosteriorSampler
    m, tab = _model("m", torch.float64)
    th0 = torch.tensor(er.mode(tab), dtype=torch.float64)[None].repeat(R, 1) + 0.1
    s = PowerPosteriorSampler(m, _loader(), [['MALA', {'step': 0.3}] for _ in range(4)], theta0=th0.to(DEV), between_step=3,
                              rng='philox', seed=3, between=between, keys=KEYS)
    s.sampler.fused_block = fused_block
    s.run(num_epochs=30, num_burnin_epochs=0)
    return s, tab


@pytest.mark.parametrize("between", ["host", "device"])
def test_power_posterior_records_the_tempered_density(between):
    torch.manual_seed(0)
    s, tab = _pps(between, 256)
    for k in range(4):
        ch = s.get_chain(k)
        smp, tvs = _np(ch.get_samples()), _np(ch.get_target_vals())
        assert smp.shape == (30, 3, 4) and tvs.shape == (30, 3)
        for it in range(30):
            for r in range(3):
                v, _, S = er.tilt_value_grad(*tab, smp[it, r])
                assert abs(tvs[it, r] - float(s.temperature[k]) * v) <= 1e-9 * float(s.temperature[k]) * S
    if between == "device":
        ref, _ = _pps(between, 0)
        assert s.sampler._can_fuse(False) and not ref.sampler._can_fuse(False)
        for key in KEYS:
            a, b = s._backing.bufs[key][:30], ref._backing.bufs[key][:30]
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), key
        assert torch.equal(s.sampler._theta, ref.sampler._theta) and torch.equal(s.sampler._grad, ref.sampler._grad)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_entry_points_write_nothing():
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import _stream
    pl, _ = _plan(5, torch.float64)
    C, P = 4, 5
    th = torch.zeros(C, P, dtype=torch.float64, device=DEV)
    lib = L.lib()
    s = _stream(pl.device)
    x = torch.full((3, 2), 7.0, dtype=torch.float64, device=DEV)
    assert lib.ey_plan_set_data(pl.handle, L.ptr(x), L.ptr(x), 3, s) == -1
    assert "distribution plan" in lib.ey_last_error().decode()
    mu = torch.zeros(P, dtype=torch.float64, device=DEV)
    assert lib.ey_plan_set_prior(pl.handle, L.ptr(mu), L.ptr(mu + 1), s) == -1
    assert "distribution plan" in lib.ey_last_error().decode()
    assert lib.ey_plan_set_prior_family(pl.handle, L.EY_PRIOR_LAPLACE, L.ptr(mu), L.ptr(mu + 1), None, s) == -1
    assert "distribution plan" in lib.ey_last_error().decode()
    rows = torch.full((C, 3), 7.0, dtype=torch.float64, device=DEV)
    assert lib.ey_log_lik_rows(pl.handle, L.ptr(th), None, C, L.ptr(rows), s) == -2
    assert "distribution plan" in lib.ey_last_error().decode()
    fwd = torch.full((C, 3), 7.0, dtype=torch.float64, device=DEV)
    assert lib.ey_forward(pl.handle, L.ptr(th), C, L.ptr(fwd), s) == -1
    assert "distribution plan" in lib.ey_last_error().decode()
    from eeyore_amd.plan import GibbsTable
    tb = GibbsTable(pl, [[0, 1], [2, 3, 4]], [0.1, 0.2])
    tv = torch.full((C,), 7.0, dtype=torch.float64, device=DEV)
    acc = torch.full((C, 2), 7, dtype=torch.uint8, device=DEV)
    assert lib.ey_gibbs_step(pl.handle, tb.handle, L.ptr(th), L.ptr(tv), None, None, None, C, 0, 0, 0, 0, L.ptr(acc), None,
                             s) == -2
    assert "distribution plan" in lib.ey_last_error().decode()
    assert lib.ey_gibbs_run(pl.handle, tb.handle, L.ptr(th), L.ptr(tv), None, C, 0, 0, 0, 0, 2, None, None, None, None,
                            L.ptr(acc), s) == -2
    st = torch.full((C, 3), 7.0, dtype=torch.float64, device=DEV)
    stepv = torch.full((C,), 7.0, dtype=torch.float64, device=DEV)
    table = torch.ones(4, 3, dtype=torch.float64, device=DEV)
    assert lib.ey_plan_attach_da(pl.handle, L.ptr(st), L.ptr(stepv), L.ptr(table), 4, C, 0.65, float('nan'), 1) == -2
    assert "distribution plan" in lib.ey_last_error().decode()
    torch.cuda.synchronize()
    assert (rows == 7).all() and (tv == 7).all() and (acc == 7).all() and (th == 0).all() and (st == 7).all()
    assert (stepv == 7).all() and (fwd == 7).all()
    # still the plan it was: data and prior "set", the options and EY_FORCE_GENERIC accepted without effect
    a = pl.log_target_grad(th + 0.25)
    pl.row_waves, pl.f32_products = "on", "exact"
    pl.set_variant(0x310)
    b = pl.log_target_grad(th + 0.25)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and pl.kernel == "dist"
    t1, g1 = pl.log_target_grad(th + 0.25)
    o1 = pl.mala_step(th + 0.25, t1, g1, 0.1, seed=1, flags=L.EY_FORCE_GENERIC)
    t2, g2 = pl.log_target_grad(th + 0.25)
    o2 = pl.mala_step(th + 0.25, t2, g2, 0.1, seed=1)
    assert torch.equal(o1["log_rate"], o2["log_rate"])
    pl.detach_da()  # detaching nothing stays allowed: the run loop does it before every run


def test_a_mixture_plan_keeps_its_messages():
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import Plan, _stream
    pl = Plan.mixture(np.zeros(1), np.zeros((1, 2)), np.eye(2)[None], torch.float64, DEV)
    x = torch.zeros(3, 2, dtype=torch.float64, device=DEV)
    assert L.lib().ey_plan_set_data(pl.handle, L.ptr(x), L.ptr(x), 3, _stream(pl.device)) == -1
    assert L.lib().ey_last_error().decode() == \
        "ey_plan_set_data: a mixture plan takes no data (its tables are fixed at creation)"
    assert L.lib().ey_forward(pl.handle, L.ptr(x), 3, L.ptr(x), _stream(pl.device)) == -1
    assert L.lib().ey_last_error().decode() == "ey_forward: a mixture plan has no network"


# ------------------------------------------------------------------------------------------------ MLP plans unaffected
def test_an_mlp_plan_after_a_tilt_plan_gives_the_same_bits():
    from eeyore_amd.plan import Plan

    def mlp_bits():
        rng = np.random.default_rng(0)
        x, y = rng.standard_normal((70, 4)), np.eye(3)[rng.integers(0, 3, 70)]
        pl = Plan([4, 3, 3], [1, 1], [1, 0], 1, torch.float32, DEV)
        pl.set_data(_t(x, torch.float32), _t(y, torch.float32))
        pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
        th = _t(0.3 * rng.standard_normal((7, pl.P)), torch.float32)
        tv, gr = pl.log_target_grad(th)
        rs = torch.empty(5, 7, pl.P, dtype=torch.float32, device=DEV)
        pl.hmc_run(th, tv, gr, 0.05, 3, 5, seed=1, samples=rs)
        chol = (0.1 * torch.eye(pl.P, device=DEV)).expand(7, pl.P, pl.P).contiguous()
        pl.ram_run(th, tv, chol, 3, 5, seed=2)
        return pl.kernel, tv.clone(), gr.clone(), rs, th.clone(), chol

    before = mlp_bits()
    pl, _ = _plan(65, torch.float32)
    th, tv, gr = _start(pl, 5, 65, torch.float32)
    pl.hmc_run(th, tv, gr, 0.05, 3, 4, seed=1)
    after = mlp_bits()
    assert before[0] == after[0] == "generic"
    for a, b in zip(before[1:], after[1:]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ moments
# The largest deviation of the pooled mean / variance of exp(theta) from the truth (2 and 2) that the restatement
# (dist_restatement.mala_draw's arithmetic for all chains at once, exptilt_restatement.mala_chains, on LogGamma(2, 1): 256
# chains, 100 burn-in + 400 draws, step 0.25, starts mode + 0.5 z) shows over the seeds 0..19, measured on the CPU:
RESTATEMENT_MEAN_DEV, RESTATEMENT_VAR_DEV = 2.87e-2, 4.01e-2


def test_pooled_moments_of_mala_on_log_gamma():
    from eeyore_amd.models import DistributionModel, LogGamma
    from eeyore_amd.samplers import MALA
    tgt = LogGamma(2.0, 1.0)
    m = DistributionModel(tgt, 1, dtype=torch.float64, device=DEV)
    C = 256
    g = torch.Generator().manual_seed(11)
    th0 = (float(np.log(2.0)) + 0.5 * torch.randn(C, 1, generator=g, dtype=torch.float64)).to(DEV)
    s = MALA(m, theta0=th0, dataloader=_loader(), step=0.25, seed=5)
    s.run(num_epochs=500, num_burnin_epochs=100)
    x = np.exp(_np(s.get_chain().get_samples()).reshape(-1))
    assert x.shape == (400 * C,)
    mean_dev, var_dev = abs(x.mean() - 2.0), abs(x.var(ddof=1) - 2.0)
    print(f"pooled mean deviation {mean_dev:.3e}, variance deviation {var_dev:.3e}")
    # one device seed against the worst of twenty restatement seeds: four times, as test_pooled_moments_of_hmc_on_target_a
    assert mean_dev <= 4 * RESTATEMENT_MEAN_DEV and var_dev <= 4 * RESTATEMENT_VAR_DEV


# ------------------------------------------------------------------------------------------------ examples
@pytest.mark.parametrize("script", ["gamma_mala_unnormalized_target.py", "gamma_mala_normalized_target.py"])
def test_gamma_example_runs(script):
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="60", EEYORE_EXAMPLE_CHAINS="64", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "kernel family: dist" in out.stdout and "cceptance rate" in out.stdout and "true mean" in out.stdout
