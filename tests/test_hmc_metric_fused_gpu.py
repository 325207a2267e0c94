"""HMC under a diagonal metric and its warm-up on the matrix cores (EY_HMC_METRIC_FUSED, k_hmc_metric_mfma in
eeyore_amd/csrc/ey_hmc_metric_mfma.hip) on the MLP(4-32-32-dK) plans of tests/hmc_metric_fused_cases.py: against
the f64 restatement, against the parent's path on the same plan (no bit: k_hmc_metric on the generic f32 evaluation), against
k_mfma32 under identity scales, and against itself.

The plans are f32, so the comparison with the restatement cannot be to rounding of f64.  The tolerances are MEASURED, not
chosen: tests/tools/hmc_metric_fused_margin_probe.py runs the parent's path on every case, each draw from the restatement's f32
state, and prints per quantity the largest error against the restatement -- target, H_cur, H_prop and the rate absolutely
(H_prop and the rate over the pairs that are not blown, tests/hmc_metric_fused_cases.py), theta and the gradient relative to
the chain's largest entry.  TAU of a quantity is 8 times that figure rounded up to one digit; the factor is
tests/test_nuts_fused_gpu.py's and covers the other order of summation over the row tiles and the bf16x3 pieces.  Every (draw,
chain) pair of every case has a decision margin above MARGIN_FLOOR by the restatement (tests/test_hmc_metric_fused_host.py),
and the TAUs of the quantities decisions are made on must not exceed it, so every pair is compared: decisions exactly,
values within TAU.

Measured on the device (the probe), the parent's path, the largest over the eight cases: target 1.36e-4 (the
BCE case, at a target near -970), H_cur 1.78e-4, H_prop 1.70e-4, rate 1.22e-4, theta 1.55e-7 and the gradient 5.19e-7 of the
largest entry; so TAU = 2e-3, 2e-3, 2e-3, 1e-3, 2e-6 and 5e-6.  The fused kernel's own largest errors on the same draws are
1.36e-4, 1.37e-4, 1.48e-4, 1.22e-4, 1.55e-7 and 5.52e-7, and neither path decides any of the 264 pairs otherwise than the
restatement.  Under identity scales the accepted proposals of this kernel and of k_mfma32 came out bit-equal on n150/bce-tanh
and not bit-equal on n33 (the step enters the updates folded into the scale here, (eps s) v, and as eps v there)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import hmc_metric_fused_cases as hc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
FUSED, PARENT = getattr(L, "EY_HMC_METRIC_FUSED", 32), 0
SEED, IT0, K_RUN = 37, 5, 6
# the probe's figures (the parent's path against the f64 restatement, the largest over the eight cases) and 8 x each, rounded up
E_PARENT = dict(target=1.36e-4, h_cur=1.78e-4, h_prop=1.70e-4, rate=1.22e-4, theta=1.55e-7, grad=5.19e-7)
TAU = dict(target=2e-3, h_cur=2e-3, h_prop=2e-3, rate=1e-3, theta=2e-6, grad=5e-6)
VALUES = hc.VALUES


def _t(a, dtype=F32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


def test_the_tolerances_are_eight_times_the_probes_figures_and_below_the_floor():
    import math
    for key, e in E_PARENT.items():
        digit = 10.0 ** math.floor(math.log10(8 * e))
        assert math.isclose(TAU[key], math.ceil(8 * e / digit - 1e-9) * digit, rel_tol=1e-9), key
    assert max(TAU["target"], TAU["h_cur"], TAU["h_prop"]) <= hc.MARGIN_FLOOR


@functools.lru_cache(maxsize=None)
def plan_of(name):
    from eeyore_amd.plan import Plan
    d, model = hc.setup(name), hc.model_of(name)
    pl = Plan(model["dims"], [1, 1, 1], model["acts"], model["lik"], F32, DEV)
    pl.f32_products = d["products"]
    pl.set_data(_t(d["x"]), _t(d["y"]))
    pl.set_prior(torch.tensor(d["prior"][0]), torch.tensor(d["prior"][1]))
    assert pl.kernel == "mfma32" and pl.f32_products == d["products"] and pl.P == d["P"]
    return pl


def device_args(name, chains=slice(None)):
    d = hc.setup(name)
    if d["index"] is None:
        M, index = _t(d["tables"][0]), None
    else:
        M, index = _t(d["tables"]), torch.tensor(d["index"][chains], dtype=torch.int32, device=DEV)
    return dict(M=M, index=index, steps=_t(d["steps"][chains]), temp=None if d["temps"] is None else _t(d["temps"][chains]),
                L=d["L"])


def _start(pl, dev, theta):
    th = _t(theta)
    tv, gr = pl.log_target_grad(th, temp=dev["temp"])
    return th, tv.contiguous(), gr.contiguous()


def draws_on_device(name, flags):
    """Each of the case's draws on the device from the restatement's f32 state, the target and the gradient from
    log_target_grad there.  Returns per draw a dict of numpy arrays: the decision, the values, the state left and the bits of
    the state the draw started from."""
    pl, dev = plan_of(name), device_args(name)
    v0, u, ref = hc.restate(name)
    got = []
    for k, o in enumerate(ref):
        th, tv, gr = _start(pl, dev, o["start_theta"])
        start = (th.clone(), tv.clone(), gr.clone())
        out = pl.hmc_metric_step(th, tv, gr, 0.0, dev["L"], dev["M"], "diag", index=dev["index"], v0=_t(v0[k]), u=_t(u[k]),
                                 step_vec=dev["steps"], temp=dev["temp"], flags=flags)
        g = dict(accepted=out["accepted"].cpu().numpy().astype(int), theta=_np(th), target=_np(tv), grad=_np(gr),
                 h_cur=_np(out["h_cur"]), h_prop=_np(out["h_prop"]), rate=_np(out["rate"]),
                 kept=np.array([all(torch.equal(a[c], b[c]) for a, b in zip(start, (th, tv, gr))) for c in range(hc.C)]))
        got.append(g)
    return got


def errors(got, want, calm=None):
    """Per quantity the largest error of one draw's values: absolute, or relative to the chain's largest entry; H_prop and
    the rate over the ``calm`` chains."""
    errs = {}
    for key in VALUES:
        w, g = want[key], got[key]
        if calm is not None and key in ("h_prop", "rate"):
            w, g = w[calm], g[calm]
        err = np.abs(g - w)
        if w.ndim == 2:
            err = err / np.abs(w).max(axis=1, keepdims=True)
        errs[key] = float(err.max()) if err.size else 0.0
    return errs


def check_blown(g, bl, where):
    """What is asked of the blown pairs: rejected, a rate that is 0 or NaN, an H_prop that is not below BLOWN / 2."""
    assert not g["accepted"][bl].any(), where
    with np.errstate(invalid="ignore"):
        assert not (g["rate"][bl] > 0).any(), (where, g["rate"][bl])
        assert not (np.abs(g["h_prop"][bl]) < hc.BLOWN / 2).any(), (where, g["h_prop"][bl])


def _parity(name, flags):
    _, _, ref = hc.restate(name)
    got = draws_on_device(name, flags)
    worst = dict.fromkeys(VALUES, 0.0)
    for o, g in zip(ref, got):
        for key, e in errors(g, o, ~hc.blown(o)).items():
            worst[key] = max(worst[key], e)
    print(f"{name} flags {flags}: largest errors " + ", ".join(f"{key} {worst[key]:.3g} (TAU {TAU[key]:.1g})" for key in VALUES))
    for k, (o, g) in enumerate(zip(ref, got)):
        assert np.array_equal(g["accepted"], o["accepted"].astype(int)), (name, flags, k, g["accepted"], o["accepted"], o["margin"])
        bl = hc.blown(o)
        for key, e in errors(g, o, ~bl).items():
            assert e <= TAU[key], (name, flags, k, key, e)
        check_blown(g, bl, (name, flags, k))
        stay = o["accepted"] == 0
        assert g["kept"][stay].all()   # a chain that does not move keeps the bits of theta, target and gradient
        assert np.array_equal(g["theta"][stay], o["start_theta"][stay])
    return got


# ------------------------------------------------------------------------------------------------ the kernel that serves
def test_hmc_metric_kernel_names_the_fused_path():
    """Fails on the parent commit: there is no Plan.hmc_metric_kernel."""
    from tests.test_nuts_gpu import _plan as generic_plan
    for name in hc.CASES:
        pl = plan_of(name)
        assert pl.hmc_metric_kernel(FUSED) == "mfma32" and pl.hmc_metric_kernel(FUSED | L.EY_RECOMPUTE_INITIAL_GRAD) == "mfma32"
        assert pl.hmc_metric_kernel() == "generic" and pl.hmc_metric_kernel(L.EY_RECOMPUTE_INITIAL_GRAD) == "generic"
        assert pl.hmc_metric_kernel(FUSED | L.EY_FORCE_GENERIC) == "generic"
    xor = generic_plan("xor/diag", F32)
    assert xor.kernel == "generic" and xor.hmc_metric_kernel(FUSED) == "generic" and xor.hmc_metric_kernel() == "generic"
    th = torch.zeros(3, xor.P, dtype=F32, device=DEV)
    tv, gr = xor.log_target_grad(th)
    before = (th.clone(), tv.clone(), gr.clone())
    with pytest.raises(RuntimeError, match="status -2"):
        xor.hmc_metric_step(th, tv, gr, 0.1, 3, torch.ones(xor.P, dtype=F32, device=DEV), "diag", seed=SEED, flags=FUSED)
    assert b"ey_plan_kernel" in L.lib().ey_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((th, tv, gr), before))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(hc.CASES))
def test_parity_with_given_randoms(name):
    """The fused path against the restatement on every pair, the parent's path against the restatement the same way, and the
    two against each other."""
    _, _, ref = hc.restate(name)
    fused = _parity(name, FUSED)
    parent = _parity(name, PARENT)
    for k, (a, b) in enumerate(zip(fused, parent)):
        assert np.array_equal(a["accepted"], b["accepted"]), (name, k)
        for key, e in errors(a, b, ~hc.blown(ref[k])).items():
            assert e <= TAU[key], (name, k, key, e)


@pytest.mark.parametrize("name", ["n150", "n33/prior/temp", "n150/bce-tanh"])
def test_on_the_streams_both_paths_consume_the_same_variates(name):
    """v0 = u = NULL: the restatement on the Philox oracle's normals and uniforms.  The chains whose margin exceeds the floor
    must agree in decision on both paths; at least a third of the 11 are decided."""
    from oracle import philox_oracle as po
    pl, dev, d = plan_of(name), device_args(name), hc.setup(name)
    v0 = hc.f32(po.normal(hc.C, pl.P, SEED, IT0, dtype=np.float32))
    u = hc.f32(po.uniform(hc.C, SEED, IT0, dtype=np.float32))
    t, g = hc.evaluate(name, d["theta"])
    ref = hc.restate_draw(name, d["theta"], t, g, v0, u)
    live = ref["margin"] > hc.MARGIN_FLOOR
    for flags in (FUSED, PARENT):
        th, tv, gr = _start(pl, dev, d["theta"])
        out = pl.hmc_metric_step(th, tv, gr, 0.0, dev["L"], dev["M"], "diag", index=dev["index"], step_vec=dev["steps"],
                                 temp=dev["temp"], seed=SEED, it=IT0, flags=flags)
        got = out["accepted"].cpu().numpy().astype(int)
        assert np.array_equal(got[live], ref["accepted"][live].astype(int)), (name, flags, got, ref["accepted"], ref["margin"])
        err = np.abs(_np(th) - ref["theta"]) / np.abs(ref["theta"]).max(axis=1, keepdims=True)
        assert (err[live] <= TAU["theta"]).all(), (name, flags, float(err[live].max()))
        calm = live & ~hc.blown(ref)
        assert (np.abs(_np(out["h_cur"]) - ref["h_cur"])[live] <= TAU["h_cur"]).all(), (name, flags)
        assert (np.abs(_np(out["h_prop"]) - ref["h_prop"])[calm] <= TAU["h_prop"]).all(), (name, flags)
    print(f"{name} on the streams: {int(live.sum())} of {hc.C} chains decided")
    assert live.sum() >= (hc.C + 2) // 3


@pytest.mark.parametrize("name", ["n33", "n150/bce-tanh"])
def test_identity_scales_are_the_plain_fused_draw(name):
    """s = 1: hmc_metric_step with the bit against hmc_step (k_mfma32) on the same plan with p0 = v0 and the same u."""
    pl, dev, d = plan_of(name), device_args(name), hc.setup(name)
    v0 = hc.restate(name)[0][0]
    u, ref = hc.restate_identity(name)
    one = torch.ones(pl.P, dtype=F32, device=DEV)
    a, b = _start(pl, dev, d["theta"]), _start(pl, dev, d["theta"])
    kw = dict(u=_t(u), step_vec=dev["steps"], temp=dev["temp"])
    oa = pl.hmc_metric_step(*a, 0.0, dev["L"], one, "diag", v0=_t(v0), flags=FUSED, **kw)
    ob = pl.hmc_step(*b, 0.0, dev["L"], p0=_t(v0), **kw)
    assert torch.equal(oa["accepted"], ob["accepted"])
    assert np.array_equal(oa["accepted"].cpu().numpy().astype(int), ref["accepted"].astype(int))
    assert 0 < int(oa["accepted"].sum()) < hc.C
    ga = dict(theta=_np(a[0]), target=_np(a[1]), grad=_np(a[2]), **{k: _np(oa[k]) for k in ("h_cur", "h_prop", "rate")})
    gb = dict(theta=_np(b[0]), target=_np(b[1]), grad=_np(b[2]), **{k: _np(ob[k]) for k in ("h_cur", "h_prop", "rate")})
    bl = hc.blown(ref)
    for key, e in errors(ga, gb, ~bl).items():
        assert e <= TAU[key], (name, key, e)
    for g in (ga, gb):
        for key, e in errors(g, ref, ~bl).items():
            assert e <= TAU[key], (name, key, e)
    acc = oa["accepted"].bool()
    same = all(torch.equal(x[acc], y[acc]) for x, y in zip(a, b))
    print(f"{name}, identity scales: the {int(acc.sum())} accepted proposals of the two kernels are "
          f"{'bit-equal' if same else 'NOT bit-equal'} in theta, target and gradient")


# ------------------------------------------------------------------------------------------------ run against steps
def _run_records(C, P, n):
    return dict(samples=torch.empty(n, C, P, dtype=F32, device=DEV), targets=torch.empty(n, C, dtype=F32, device=DEV),
                accepted_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV),
                accept_count=torch.zeros(C, dtype=torch.int32, device=DEV))


def _bits_equal(xs, ys):
    for x, y in zip(xs, ys):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("name", ["n33/prior/temp", "n150/bce-tanh"])
def test_run_is_its_steps_bit_for_bit(name, C):
    chains = slice(1, 2) if C == 1 else slice(None)
    pl, dev = plan_of(name), device_args(name, chains)
    a = _start(pl, dev, hc.setup(name)["theta"][chains])
    b = tuple(t.clone() for t in a)
    rec = _run_records(C, pl.P, K_RUN)
    kw = dict(index=dev["index"], step_vec=dev["steps"], temp=dev["temp"], seed=SEED, flags=FUSED)
    oa = pl.hmc_metric_run(*a, 0.0, dev["L"], dev["M"], "diag", K_RUN, it=IT0, **kw, **rec)
    moved = 0
    for k in range(K_RUN):
        ob = pl.hmc_metric_step(*b, 0.0, dev["L"], dev["M"], "diag", it=IT0 + k, **kw)
        assert torch.equal(rec["samples"][k], b[0]) and torch.equal(rec["targets"][k], b[1]), k
        assert torch.equal(rec["accepted_rec"][k], ob["accepted"]), k
        moved += int(ob["accepted"].sum())
    _bits_equal(list(a) + [oa["accepted"]], list(b) + [ob["accepted"]])
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0)) and moved > 0
    assert torch.isfinite(rec["samples"]).all()


# ------------------------------------------------------------------------------------------------ the warm-up
def test_warmup_with_nothing_attached_is_the_run():
    name = "n33/index"
    pl, dev = plan_of(name), device_args(name)
    a = _start(pl, dev, hc.setup(name)["theta"])
    b = tuple(t.clone() for t in a)
    ra, rb = _run_records(hc.C, pl.P, K_RUN), _run_records(hc.C, pl.P, K_RUN)
    kw = dict(index=dev["index"], step_vec=dev["steps"], seed=SEED, it=IT0, flags=FUSED)
    oa = pl.hmc_metric_run(*a, 0.0, dev["L"], dev["M"], "diag", K_RUN, **kw, **ra)
    ob = pl.hmc_metric_warmup(*b, 0.0, dev["L"], dev["M"], "diag", K_RUN, **kw, **rb)
    _bits_equal(list(a) + [ra[k] for k in ra] + [oa[k] for k in oa], list(b) + [rb[k] for k in ra] + [ob[k] for k in oa])
    assert int(ra["accepted_rec"].sum()) > 0


def test_warmup_epilogues_against_the_host():
    """tests/test_nuts_fused_gpu.py's test of the two epilogues and its bounds, on this kernel: the steps recorded are
    ey_da_update's recurrence replayed on the host from the recorded rates (rtol 1e-6), the moments numpy's Welford of the
    recorded samples (1e-12 relative to the largest entry)."""
    from eeyore_amd.tuners import WindowedAdaptation
    from tests import hmc_warmup_restatement as R
    from tests import test_nuts_gpu as G
    from tests.hmc_metric_restatement import DIAG
    name = "n33"
    pl, dev = plan_of(name), device_args(name)
    C, P, K_WARM, D_TARGET = hc.C, pl.P, G.K_WARM, G.D_TARGET
    steps0 = dev["steps"][4].expand(C).contiguous().clone()   # every chain from a step that moves
    state = _start(pl, dev, hc.setup(name)["theta"])
    rec = _run_records(C, P, K_WARM)
    steps_rec, rate_rec = torch.empty(K_WARM, C, dtype=F32, device=DEV), torch.empty(K_WARM, C, dtype=F32, device=DEV)
    step_vec = steps0.clone()
    tuner = WindowedAdaptation(num_steps=1)
    da_state = tuner.restart(step_vec)
    mean, M2 = torch.zeros(C, P, dtype=F64, device=DEV), torch.zeros(C, P, dtype=F64, device=DEV)
    pl.hmc_metric_warmup(*state, 0.0, dev["L"], dev["M"], "diag", K_WARM, step_vec=step_vec, seed=SEED, it=IT0, flags=FUSED,
                         da_state=da_state, da_table=tuner.table(1, K_WARM, DEV), d=D_TARGET, final_avg=True, mean=mean, M2=M2,
                         count=0, steps_rec=steps_rec, rate_rec=rate_rec, **rec)
    assert torch.equal(steps_rec[0], steps0)
    rates, steps = _np(rate_rec), _np(steps_rec)
    for c in range(C):
        st = R.da_restart(float(steps0[c]))
        for k in range(K_WARM):
            st, nxt = R.da_update(st, k + 1, rates[k, c], D_TARGET, averaged=k == K_WARM - 1)
            got = steps[k + 1, c] if k + 1 < K_WARM else float(step_vec[c])
            assert abs(got - nxt) <= 1e-6 * nxt, (c, k, got, nxt)
        np.testing.assert_allclose(_np(da_state[c, :2]), st[:2], rtol=1e-9, atol=1e-12)
    assert len(np.unique(steps[-1])) > 1 and (rates >= 0).all() and (rates <= 1).all()
    want_mean, want_M2 = R.welford_chains(_np(rec["samples"]), DIAG)
    np.testing.assert_allclose(_np(M2), want_M2, rtol=1e-12, atol=1e-12 * np.abs(want_M2).max())
    np.testing.assert_allclose(_np(mean), want_mean, rtol=1e-12, atol=1e-12 * np.abs(want_mean).max())
    acc = rec["accepted_rec"]
    assert 0 < int(acc.sum()) < acc.numel()   # the moments saw chains that moved and chains left where they were


# ------------------------------------------------------------------------------------------------ every wave slot and round
@pytest.mark.parametrize("name", ["n330", "n33/index", "n150/bce-tanh"])
def test_every_wave_slot_and_chain_round(name):
    """The 11 chains tiled over C = 8 CUs + 11 with tiled v0 and u, as tests/test_persistent_slots.py does: every replica
    equals its original bit for bit, and replica 0 the same chains launched alone.  (H_prop and the rate are compared as
    bits: the hundredfold step's are not finite.)"""
    from tests.test_persistent_slots import Replicas, slot
    pl, dev, d = plan_of(name), device_args(name), hc.setup(name)
    v0, u, _ = hc.restate(name)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    C = 8 * n_cu + hc.C
    assert slot(C - 1, n_cu, 8)[2] == 1   # a second round, ragged
    rep = Replicas(C, n_cu, 8)
    assert hc.C == 11 == int(rep.idx.max()) + 1

    def fn(th, v0, u, steps, temp, index):
        tv, gr = pl.log_target_grad(th, temp=temp)
        tv, gr = tv.contiguous(), gr.contiguous()
        out = pl.hmc_metric_step(th, tv, gr, 0.0, dev["L"], dev["M"], "diag", index=index, v0=v0, u=u, step_vec=steps, temp=temp,
                                 flags=FUSED)
        return dict(theta=th, target=tv, grad=gr, accepted=out["accepted"], h_cur=out["h_cur"],
                    h_prop=out["h_prop"].view(torch.int32), rate=out["rate"].view(torch.int32))
    small = rep.both(f"hmc_metric_step fused {name}", fn, _t(d["theta"]), _t(v0[0]), _t(u[0]), dev["steps"], dev["temp"],
                     dev["index"])
    assert 0 < int(small["accepted"].sum()) < hc.C


# ------------------------------------------------------------------------------------------------ non-finite, refusals
def test_a_chain_that_starts_at_a_nan_state_is_rejected_and_keeps_it():
    name = "n150"
    pl, dev, theta = plan_of(name), device_args(name), hc.setup(name)["theta"]
    a = _start(pl, dev, theta)
    bad = theta.copy()
    bad[4] = np.nan
    b = _start(pl, dev, bad)
    assert torch.isnan(b[1][4])
    kept = tuple(t.clone() for t in b)
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0, flags=FUSED)
    oa = pl.hmc_metric_step(*a, 0.0, dev["L"], dev["M"], "diag", **kw)
    ob = pl.hmc_metric_step(*b, 0.0, dev["L"], dev["M"], "diag", **kw)
    assert int(ob["accepted"][4]) == 0 and torch.isnan(ob["rate"][4]) and torch.isnan(b[0][4]).all()
    for x, y in zip(b, kept):   # the bits of the NaN state as they were
        assert torch.equal(x[4].view(torch.int32), y[4].view(torch.int32))
    others = torch.arange(hc.C, device=DEV) != 4
    for x, y in list(zip(a, b)) + [(oa[key].view(torch.int32) if oa[key].dtype == F32 else oa[key],
                                    ob[key].view(torch.int32) if ob[key].dtype == F32 else ob[key]) for key in oa]:
        assert torch.equal(x[others], y[others])
    assert int(oa["accepted"].sum()) > 0


def test_refusals_leave_everything_untouched():
    from eeyore_amd.plan import Plan, _stream
    lib = L.lib()
    name = "n33"
    pl, dev = plan_of(name), device_args(name)
    C, nL = hc.C, dev["L"]
    th, tv, gr = _start(pl, dev, hc.setup(name)["theta"])
    before = tuple(t.clone() for t in (th, tv, gr))
    acc = torch.full((C,), 7, dtype=torch.uint8, device=DEV)
    rate = torch.full((C,), -3.0, dtype=F32, device=DEV)
    tril = torch.eye(4, dtype=F32, device=DEV)   # (refused before it is looked at)
    s = _stream(pl.device)

    def raw_step(plan, M, form, flags):
        return lib.ey_hmc_metric_step(plan.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(M), form, 1, None, None, None, 0.05,
                                      None, nL, None, C, SEED, 0, 0, flags, L.ptr(acc), L.ptr(rate), None, None, s)

    def raw_run(plan, M, form, flags, warm):
        lead = (plan.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(M), form, 1, None, 0.05, None, nL, None, C, SEED, 0, 0,
                flags, 2, None, None, None, None, L.ptr(acc))
        if warm:
            return lib.ey_hmc_metric_warmup(*lead, None, None, 0, 0.8, float("nan"), 0, None, None, 0, None, L.ptr(rate), s)
        return lib.ey_hmc_metric_run(*lead, s)

    def untouched():
        torch.cuda.synchronize()
        return (all(torch.equal(x, y) for x, y in zip((th, tv, gr), before)) and bool((acc == 7).all())
                and bool((rate == -3.0).all()))

    out = dict(accepted=acc, rate=rate, h_cur=rate, h_prop=rate)
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0)
    # the bit with a dense metric, and with EY_FORCE_GENERIC: step, run and warm-up, raw and through Plan
    for call in (lambda: raw_step(pl, tril, L.EY_METRIC_TRIL, FUSED), lambda: raw_run(pl, tril, L.EY_METRIC_TRIL, FUSED, False),
                 lambda: raw_run(pl, tril, L.EY_METRIC_TRIL, FUSED, True)):
        assert call() == -1
        assert b"diagonal metric only" in lib.ey_last_error() and untouched()
    for call in (lambda: raw_step(pl, dev["M"], L.EY_METRIC_DIAG, FUSED | L.EY_FORCE_GENERIC),
                 lambda: raw_run(pl, dev["M"], L.EY_METRIC_DIAG, FUSED | L.EY_FORCE_GENERIC, False),
                 lambda: raw_run(pl, dev["M"], L.EY_METRIC_DIAG, FUSED | L.EY_FORCE_GENERIC, True)):
        assert call() == -1
        assert b"EY_FORCE_GENERIC" in lib.ey_last_error() and untouched()
    with pytest.raises(ValueError, match="EY_FORCE_GENERIC"):
        pl.hmc_metric_step(th, tv, gr, 0.0, nL, dev["M"], "diag", flags=FUSED | L.EY_FORCE_GENERIC, out=out, **kw)
    with pytest.raises(ValueError, match="EY_FORCE_GENERIC"):
        pl.hmc_metric_run(th, tv, gr, 0.0, nL, dev["M"], "diag", 2, flags=FUSED | L.EY_FORCE_GENERIC, out=out, **kw)
    with pytest.raises(ValueError, match="EY_FORCE_GENERIC"):
        pl.hmc_metric_warmup(th, tv, gr, 0.0, nL, dev["M"], "diag", 2, flags=FUSED | L.EY_FORCE_GENERIC, out=out, **kw)
    assert untouched()
    # the refusals a call without the bit makes come first, and unchanged: num_steps 0 with the bit and a dense metric
    assert lib.ey_hmc_metric_step(pl.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(tril), L.EY_METRIC_TRIL, 1, None, None, None,
                                  0.05, None, 0, None, C, SEED, 0, 0, FUSED, L.ptr(acc), L.ptr(rate), None, None, s) == -1
    assert b"num_steps must be >= 1" in lib.ey_last_error() and untouched()
    # a batch beyond the row limit of the family: the plan is no longer served, status -2 naming ey_plan_kernel
    model = hc.model_of(name)
    wide = Plan(model["dims"], [1, 1, 1], model["acts"], model["lik"], F32, DEV)
    rows = 32 * 24 + 1
    wide.set_data(torch.zeros(rows, 4, dtype=F32, device=DEV), torch.eye(3, dtype=F32, device=DEV)[torch.zeros(rows, dtype=torch.long)])
    wide.set_prior(torch.zeros(wide.P), torch.ones(wide.P))
    assert wide.kernel != "mfma32" and wide.hmc_metric_kernel(FUSED) == "generic"
    for call in (lambda: raw_step(wide, dev["M"], L.EY_METRIC_DIAG, FUSED), lambda: raw_run(wide, dev["M"], L.EY_METRIC_DIAG, FUSED, False),
                 lambda: raw_run(wide, dev["M"], L.EY_METRIC_DIAG, FUSED, True)):
        assert call() == -2
        assert b"ey_plan_kernel" in lib.ey_last_error() and wide.kernel.encode() in lib.ey_last_error() and untouched()
    with pytest.raises(RuntimeError, match="status -2"):
        wide.hmc_metric_step(th, tv, gr, 0.0, nL, dev["M"], "diag", flags=FUSED, out=out, **kw)
    assert b"ey_plan_kernel" in lib.ey_last_error() and untouched()
    # ... and the plan that is served still is
    o = pl.hmc_metric_step(*(t.clone() for t in before), 0.0, nL, dev["M"], "diag", flags=FUSED, **kw)
    assert int(o["accepted"].sum()) > 0


# ------------------------------------------------------------------------------------------------ the sampler
def _iris_model(dims=(4, 32, 32, 3)):
    from torch.distributions import Normal
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    n = len(dims) - 1
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=list(dims), bias=n * [True],
                                                activations=(n - 1) * [torch.sigmoid] + [None]),
                    dtype=F32, device=DEV)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEV), torch.ones(P, device=DEV))
    return model, P


def _iris_loader():
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import XYDataset
    iris = XYDataset.from_eeyore('iris', yndmin=1, dtype=F32, yonehot=True, device=DEV)
    return DataLoader(iris, batch_size=len(iris), shuffle=False)


def test_the_sampler_warms_up_and_samples_the_iris_network():
    """HMC(metric='diag', tuner=WindowedAdaptation, metric_kernel='fused') on MLP(4-32-32-3) on Iris: 64 chains, a warm-up of
    30 draws, 20 stored."""
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.samplers import HMC, DiagMetric
    from eeyore_amd.tuners import WindowedAdaptation
    C, BURN, KEEP = 64, 30, 20
    model, P = _iris_model()
    gen = torch.Generator().manual_seed(4)
    theta0 = (0.1 * torch.randn(C, P, generator=gen)).to(DEV)
    s = HMC(model, theta0=theta0, dataloader=_iris_loader(), metric='diag', tuner=WindowedAdaptation(num_steps=1), seed=2,
            rng='philox', metric_kernel='fused', chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    s.run(num_epochs=BURN + KEEP, num_burnin_epochs=BURN)
    torch.cuda.synchronize()
    chain = s.get_chain()
    assert len(chain) == KEEP and tuple(chain.get_samples().shape) == (KEEP, C, P)
    assert tuple(s.step.shape) == (C,) and bool(torch.isfinite(s.step).all()) and bool((s.step > 0).all())
    assert bool(torch.isfinite(chain.get_samples()).all()) and bool(torch.isfinite(chain.get_target_vals()).all())
    assert isinstance(s.metric, DiagMetric) and bool(torch.isfinite(s._metric).all())
    plan = model._plan(*next(iter(s.dataloader)))
    assert plan.kernel == "mfma32" and plan.hmc_metric_kernel(s._metric_flags(plan)) == "mfma32"


def test_sampler_on_the_streams_reproduces_hmc_metric_run():
    """HMC(metric=DiagMetric, rng='philox', metric_kernel='fused') on the headline model: 8 chains, 8 draws, 3 of them
    burn-in, against plan.hmc_metric_run with the bit."""
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.samplers import HMC, DiagMetric
    n, burn, C, NL, STEP = 8, 3, 8, 4, 0.02
    model, P = _iris_model()
    th0 = _t(0.3 * np.random.default_rng(2).standard_normal((C, P)))
    scale = (0.5 + torch.rand(P, generator=torch.Generator().manual_seed(3))).to(DEV)
    s = HMC(model, theta0=th0, dataloader=_iris_loader(), metric=DiagMetric(scale), step=STEP, num_steps=NL, rng='philox',
            seed=SEED, metric_kernel='fused', chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    assert s._can_fuse(False)
    s.run(num_epochs=n, num_burnin_epochs=burn)
    plan = s.model._plan(*next(iter(s.dataloader)))
    assert plan.hmc_metric_kernel(FUSED) == "mfma32"
    th = th0.clone()
    tv, gr = plan.log_target_grad(th)
    rec = _run_records(C, P, n)
    plan.hmc_metric_run(th, tv.contiguous(), gr.contiguous(), STEP, NL, scale.contiguous(), "diag", n, seed=SEED, it=0,
                        flags=FUSED, **rec)
    ch = s.get_chain()
    assert len(ch) == n - burn
    assert torch.equal(ch.get_samples(), rec["samples"][burn:]) and torch.equal(ch.get_target_vals(), rec["targets"][burn:])
    assert torch.equal(ch.get_accepted(), rec["accepted_rec"][burn:])
    assert torch.equal(s._theta, th) and int(rec["accepted_rec"].sum()) > 0


def test_fused_on_a_plan_that_is_not_mfma32_names_plan_kernel():
    from eeyore_amd.samplers import HMC
    model, P = _iris_model(dims=(4, 16, 3))
    th0 = torch.zeros(4, P, dtype=F32, device=DEV)
    s = HMC(model, theta0=th0, dataloader=_iris_loader(), metric='diag', step=0.01, num_steps=2, rng='philox',
            metric_kernel='fused')
    x, y = next(iter(s.dataloader))
    plan = model._plan(x, y)
    assert plan.kernel != "mfma32"
    with pytest.raises(ValueError, match=f"plan.kernel\\) is '{plan.kernel}'"):
        s.draw(x, y)


def test_iris_hmc_windowed_warmup_example_runs():
    """examples/iris_hmc_windowed_warmup.py at reduced size, through the environment tests/test_examples.py uses."""
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="20", EEYORE_EXAMPLE_CHAINS="64", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "iris_hmc_windowed_warmup.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "metric_kernel='fused': HMC runs on the mfma32 kernel" in out.stdout
    assert "64 chains, 1315 parameters" in out.stdout and "Acceptance rate of the stored draws" in out.stdout
