"""The windowed warm-up of HMC under a metric on the device (ey_hmc_metric_warmup -- k_hmc_metric_warmup in
eeyore_amd/csrc/ey_generic.hip --, ey_metric_from_moments in eeyore_amd/csrc/ey_warmup.hip, tuners.WindowedAdaptation)
against ey_hmc_metric_run / ey_hmc_metric_step, the host tuner's recurrence, the numpy restatement
(tests/hmc_warmup_restatement.py) and itself.  Plans, inputs and steps are those of tests/test_hmc_metric_gpu.py.

Sizes: K = 7 draws of L = 3 leapfrog steps for C in {1, 3, 11} chains on the plans at which lane ownership changes (P = 1,
a full wave, a lane's second row, the dense limit), the plan with a temperature vector and a register-resident one."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from eeyore_amd.tuners import PerChainDATuner, WindowedAdaptation  # (every test of this file needs the feature)
from tests import hmc_warmup_restatement as R
from tests import test_hmc_metric_gpu as MT
from tests.hmc_metric_restatement import DIAG, TRIL
from tests.test_dist_gpu import _loader
from tests.test_hmc_metric_gpu import _mvn2, _theta0
from tests.test_mala_mvn_gpu import _np, _start
from tests.test_mh_mvn_gpu import CS, _num_params, _plan
from tests.test_ram_gpu import CASES, _data
from tests.test_ram_gpu import _plan as _mlp_plan

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
PLANS = ["mix1_1", "mix64_1", "mix65_2", "mix128_16", "mlp433", "mlp2321"]
FORM_OF = {"mix65_2": "per_chain", "mlp433": "indexed"}  # how a plan's chains find their metric (the others share one)
KINDS = ["dense", "diag"]
CODE = {"dense": TRIL, "diag": DIAG}
K, L_STEPS, IT0, D_TARGET = 7, 3, 11, 0.7
# (plan, kind, dtype id, C) -> Philox seed of the launch.  Its K draws must mix accepts and rejects and reach the upper bound
# of the step; seed 9 does for every case but the one listed (one chain, which accepts all seven draws), found on the device
# by trying seeds in turn.
SEEDS = {('mix65_2', 'diag', 'f64', 1): 0}

grid = lambda f: functools.reduce(lambda g, d: d(g), [  # noqa: E731
    pytest.mark.parametrize("C", CS), pytest.mark.parametrize("kind", KINDS),
    pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"]), pytest.mark.parametrize("name", PLANS)], f)


def _case(name, dtype, kind, C):
    """The plan, its inputs on the device (per-chain steps for every plan: dual averaging adapts a vector) and the state."""
    pl = _plan(name, dtype)
    d, dev = MT._device_inputs(name, C, FORM_OF.get(name, "shared"), kind, dtype)
    rng = np.random.default_rng(C + 13)
    dev["steps"] = torch.tensor(d["step"] * (0.5 + rng.random(C)), dtype=dtype, device=DEV)
    dev["seed"] = SEEDS.get((name, kind, "f64" if dtype == F64 else "f32", C), 9)
    return pl, dev


def _records(C, P, dtype, n=K):
    return dict(samples=torch.empty(n, C, P, dtype=dtype, device=DEV), targets=torch.empty(n, C, dtype=dtype, device=DEV),
                accepted_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV),
                accept_count=torch.zeros(C, dtype=torch.int32, device=DEV))


def _moments(C, P, kind):
    mean = torch.zeros(C, P, dtype=F64, device=DEV)
    M2 = torch.zeros((C, P) if kind == "diag" else (C, P, P), dtype=F64, device=DEV)
    if kind == "dense":  # the strict upper triangle is never read or written: it keeps what the test puts there
        M2[:, torch.triu(torch.ones(P, P, dtype=torch.bool, device=DEV), 1)] = float("nan")
    return mean, M2


def _table(t, k):
    return WindowedAdaptation(num_steps=L_STEPS).table(t, k, DEV)


def _eub(dev):
    return 2.0 * dev["step"]


def _warm(pl, dev, kind, state, n, it, step_vec, da_state, mean, M2, count, t, final_avg, rec=None, extra=None):
    th, tv, gr = state
    return pl.hmc_metric_warmup(th, tv, gr, 0.0, L_STEPS, dev["M"], kind, n, index=dev["idx"], step_vec=step_vec,
                                temp=dev["temp"], seed=dev["seed"], it=it, da_state=da_state, da_table=_table(t, n),
                                d=D_TARGET, log_eub=np.log(_eub(dev)), final_avg=final_avg, mean=mean, M2=M2, count=count,
                                **(rec or {}), **(extra or {}))


@functools.lru_cache(maxsize=None)
def _launch(name, dtype, kind, C):
    """ONE warm-up launch of K draws with dual averaging, moments and every record, shared by the tests below."""
    pl, dev = _case(name, dtype, kind, C)
    P = _num_params(name)
    start = _start(pl, dev)
    state = tuple(t.clone() for t in start)
    rec = _records(C, P, dtype)
    steps_rec, rate_rec = torch.empty(K, C, dtype=dtype, device=DEV), torch.empty(K, C, dtype=dtype, device=DEV)
    step_vec = dev["steps"].clone()
    da_state = WindowedAdaptation(num_steps=L_STEPS).restart(step_vec)
    mean, M2 = _moments(C, P, kind)
    out = _warm(pl, dev, kind, state, K, IT0, step_vec, da_state, mean, M2, 0, 1, True, rec,
                dict(steps_rec=steps_rec, rate_rec=rate_rec))
    torch.cuda.synchronize()
    return dict(pl=pl, dev=dev, start=start, state=state, rec=rec, steps_rec=steps_rec, rate_rec=rate_rec, step_vec=step_vec,
                da_state=da_state, mean=mean, M2=M2, out=out)


# ------------------------------------------------------------------------------------------------ 1. nothing attached
@grid
def test_nothing_attached_is_hmc_metric_run(name, dtype, kind, C):
    pl, dev = _case(name, dtype, kind, C)
    P = _num_params(name)
    a, b = _start(pl, dev), None
    b = tuple(t.clone() for t in a)
    ra, rb = _records(C, P, dtype), _records(C, P, dtype)
    kw = dict(index=dev["idx"], step_vec=dev["steps"], temp=dev["temp"], seed=dev["seed"], it=IT0)
    oa = pl.hmc_metric_run(*a, 0.0, L_STEPS, dev["M"], kind, K, **kw, **ra)
    ob = pl.hmc_metric_warmup(*b, 0.0, L_STEPS, dev["M"], kind, K, **kw, **rb)
    for x, y in list(zip(a, b)) + [(ra[k], rb[k]) for k in ra] + [(oa["accepted"], ob["accepted"])]:
        assert torch.equal(x, y)
    assert torch.isfinite(rb["samples"]).all()


# ------------------------------------------------------------------------------------------------ 2. replay
@grid
def test_replay_with_the_recorded_steps(name, dtype, kind, C):
    r = _launch(name, dtype, kind, C)
    pl, dev, rec = r["pl"], r["dev"], r["rec"]
    th, tv, gr = (t.clone() for t in r["start"])
    for k in range(K):
        out = pl.hmc_metric_step(th, tv, gr, 0.0, L_STEPS, dev["M"], kind, index=dev["idx"],
                                 step_vec=r["steps_rec"][k].contiguous(), temp=dev["temp"], seed=dev["seed"], it=IT0 + k)
        assert torch.equal(rec["samples"][k], th) and torch.equal(rec["targets"][k], tv), k
        assert torch.equal(rec["accepted_rec"][k], out["accepted"]), k
        bits = torch.int64 if dtype == F64 else torch.int32  # (a trajectory that left the finite numbers has a NaN rate)
        assert torch.equal(r["rate_rec"][k].contiguous().view(bits), out["rate"].view(bits)), k
    assert all(torch.equal(a, b) for a, b in zip(r["state"], (th, tv, gr)))
    total = int(rec["accepted_rec"].sum())
    print(f"{name} {kind} C={C}: {total} of {C * K} draws accepted")
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0))
    assert 0 < total < C * K


# ------------------------------------------------------------------------------------------------ 3. dual averaging
@grid
def test_dual_averaging_equals_the_host_recurrence(name, dtype, kind, C):
    r = _launch(name, dtype, kind, C)
    dev = r["dev"]
    tuner = PerChainDATuner(dev["steps"].clone(), num_steps=L_STEPS, d=D_TARGET, eub=_eub(dev))
    assert torch.equal(r["steps_rec"][0], dev["steps"])
    bound = 0
    for k in range(K):
        step, _ = tuner.tune(r["rate_rec"][k], k, return_e=k != K - 1)
        nxt = r["steps_rec"][k + 1] if k + 1 < K else r["step_vec"]
        np.testing.assert_allclose(_np(nxt), _np(step), rtol=1e-6, atol=0)
        bound += int(np.isclose(_np(nxt), _eub(dev), rtol=1e-6, atol=0).sum()) if k + 1 < K else 0
    np.testing.assert_allclose(_np(r["da_state"][:, 0]), _np(tuner.barh), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(_np(r["da_state"][:, 1]), _np(tuner.logbare), rtol=1e-9, atol=1e-12)
    assert torch.equal(r["da_state"][:, 2], torch.log(10 * dev["steps"].double()))
    # final_avg: the last draw leaves the averaged step
    np.testing.assert_allclose(_np(r["step_vec"]), np.exp(_np(r["da_state"][:, 1])), rtol=1e-6, atol=0)
    print(f"{name} {kind} C={C}: {bound} of {C * (K - 1)} adapted steps at the upper bound")
    assert bound > 0


# ------------------------------------------------------------------------------------------------ 4. moments
@grid
def test_moments_equal_welford_of_the_recorded_samples(name, dtype, kind, C):
    """Measured on an MI355X: see DESIGN.md 4.23."""
    r = _launch(name, dtype, kind, C)
    P = _num_params(name)
    want_mean, want_M2 = R.welford_chains(_np(r["rec"]["samples"]), CODE[kind])
    mean, M2 = _np(r["mean"]), _np(r["M2"])
    if kind == "dense":
        upper = np.triu(np.ones((P, P), bool), 1)
        assert np.isnan(M2[:, upper]).all()
        M2, want_M2 = np.where(upper, 0.0, M2), np.where(upper, 0.0, want_M2)
    scale = np.abs(want_M2).max()
    print(f"{name} {kind} C={C}: largest error of M2 {np.abs(M2 - want_M2).max():.3e} (largest entry {scale:.3e}), of the "
          f"mean {np.abs(mean - want_mean).max():.3e} (largest entry {np.abs(want_mean).max():.3e})")
    np.testing.assert_allclose(M2, want_M2, rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(mean, want_mean, rtol=1e-12, atol=1e-12 * np.abs(want_mean).max())


# ------------------------------------------------------------------------------------------------ 5. launch splits
@grid
def test_a_split_launch_leaves_the_same_bits(name, dtype, kind, C):
    r = _launch(name, dtype, kind, C)
    pl, dev = r["pl"], r["dev"]
    P = _num_params(name)
    state = tuple(t.clone() for t in r["start"])
    step_vec = dev["steps"].clone()
    da_state = WindowedAdaptation(num_steps=L_STEPS).restart(step_vec)
    mean, M2 = _moments(C, P, kind)
    _warm(pl, dev, kind, state, 4, IT0, step_vec, da_state, mean, M2, 0, 1, False)
    _warm(pl, dev, kind, state, 3, IT0 + 4, step_vec, da_state, mean, M2, 4, 5, True)
    for a, b in zip(state + (step_vec, da_state, mean), r["state"] + (r["step_vec"], r["da_state"], r["mean"])):
        assert torch.equal(a, b)
    assert torch.equal(torch.nan_to_num(M2, nan=-1.0), torch.nan_to_num(r["M2"], nan=-1.0))


# ------------------------------------------------------------------------------------------------ 6. metric_from_moments
def _host_moments(P, C, n, kind, seed=0):
    """Moments of n draws of C chains from a Gaussian whose covariance has condition number 1e3 (numpy f64)."""
    rng = np.random.default_rng(seed + 7 * P + C)
    q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    A = q * np.sqrt(0.05 * np.logspace(0, 3, P))
    draws = rng.standard_normal((n, C, P)) @ A.T + 0.3 * rng.standard_normal((1, C, P))
    return R.welford_chains(draws, CODE[kind])


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "per_chain"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 128])
def test_metric_from_moments_against_the_restatement(P, C, kind, pooled):
    """Measured on an MI355X: see DESIGN.md 4.23.  The bounds are taken against the table's largest entry as well as each
    entry's own size: nine draws per chain in up to 128 dimensions give a covariance of low rank plus the shrinkage, and
    the entries of its factor pass through zero."""
    from eeyore_amd.plan import Plan
    n = 9
    mean, M2 = _host_moments(P, C, n, kind)
    want = R.metric_from_moments(mean, M2, n, CODE[kind], pooled)
    mean_d, M2_d = torch.tensor(mean, device=DEV), torch.tensor(M2, device=DEV)
    if kind == "dense":
        M2_d[:, torch.triu(torch.ones(P, P, dtype=torch.bool, device=DEV), 1)] = float("nan")  # never read
    tables = {}
    for dtype, rtol in ((F64, 1e-9), (F32, 1e-6)):
        pl = Plan.mixture(np.zeros(1), np.zeros((1, P)), np.eye(P)[None], dtype, DEV)
        table, status = pl.metric_from_moments(mean_d, M2_d, n, kind, pooled=pooled)
        again, _ = pl.metric_from_moments(mean_d, M2_d, n, kind, pooled=pooled)
        assert torch.equal(table, again) and table.dtype == dtype and tuple(table.shape) == want.shape
        assert int(status.sum()) == 0 and status.numel() == (1 if pooled else C)
        err = np.abs(_np(table) - want).max()
        print(f"P={P} C={C} {kind} {'pooled' if pooled else 'per chain'} {dtype}: largest error {err:.3e} of "
              f"{np.abs(want).max():.3e}")
        np.testing.assert_allclose(_np(table), want, rtol=rtol, atol=rtol * np.abs(want).max())
        if kind == "dense":
            assert (torch.triu(table, 1) == 0).all() and (torch.diagonal(table, dim1=-2, dim2=-1) > 0).all()
        tables[dtype] = table
    assert torch.equal(tables[F32], tables[F64].float())  # the f64 result rounded once
    if not pooled and C > 1:
        pl = Plan.mixture(np.zeros(1), np.zeros((1, P)), np.eye(P)[None], F64, DEV)
        # two chains with equal moments give equal entries
        mean_d[1], M2_d[1] = mean_d[0], M2_d[0]
        table, status = pl.metric_from_moments(mean_d, M2_d, n, kind, pooled=False)
        assert torch.equal(table[0], table[1]) and torch.equal(table[0], tables[F64][0]) and int(status.sum()) == 0
        # a chain whose M2 is NaN: its status is 1, its entry keeps the sentinel, every other entry is as before
        M2_d[1] = float("nan")
        sentinel = torch.full_like(table, -3.0)
        got, status = pl.metric_from_moments(mean_d, M2_d, n, kind, pooled=False, table=sentinel)
        assert status.tolist() == [0, 1] + [0] * (C - 2)
        assert (got[1] == -3.0).all() and torch.equal(got[0], table[0]) and torch.equal(got[2:], tables[F64][2:])
        # a pivot that is not positive (a negative M2), and the pooled estimate of the poisoned moments
        M2_d[1] = -1.0 - M2_d[0].nan_to_num(0.0).abs()
        _, status = pl.metric_from_moments(mean_d, M2_d, n, kind, pooled=False, table=sentinel)
        assert status.tolist() == [0, 1] + [0] * (C - 2) and (sentinel[1] == -3.0).all()
        M2_d[1] = float("nan")
        keep = torch.full(want.shape[1:], -3.0, dtype=F64, device=DEV)
        _, status = pl.metric_from_moments(mean_d, M2_d, n, kind, pooled=True, table=keep)
        assert status.tolist() == [1] and (keep == -3.0).all()


def test_metric_from_moments_refuses_fewer_than_two_draws():
    from eeyore_amd.plan import Plan
    pl = Plan.mixture(np.zeros(1), np.zeros((1, 2)), np.eye(2)[None], F64, DEV)
    mean, M2 = torch.zeros(1, 2, dtype=F64, device=DEV), torch.zeros(1, 2, dtype=F64, device=DEV)
    table = torch.full((2,), -3.0, dtype=F64, device=DEV)
    with pytest.raises(ValueError, match="at least two draws"):
        pl.metric_from_moments(mean, M2, 1, "diag", table=table)  # C n = 1
    m3 = torch.zeros(3, 2, dtype=F64, device=DEV)
    with pytest.raises(ValueError, match="at least two draws"):
        pl.metric_from_moments(m3, m3.clone(), 1, "diag", pooled=False)  # per chain: n = 1 whatever C
    torch.cuda.synchronize()
    assert (table == -3.0).all()
    t, s = pl.metric_from_moments(m3, m3.clone(), 1, "diag")  # pooled: C n = 3
    assert int(s.sum()) == 0 and torch.isfinite(t).all()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing():
    from eeyore_amd import _lib as Lb
    from eeyore_amd.plan import _stream
    C, n = 3, 4
    nan = float("nan")

    def buffers(pl, dtype, kind):
        b = dict(th=torch.full((C, pl.P), 0.25, dtype=dtype, device=DEV), tv=torch.full((C,), -7.0, dtype=dtype, device=DEV),
                 gr=torch.full((C, pl.P), 0.5, dtype=dtype, device=DEV), acc=torch.full((C,), 9, dtype=torch.uint8, device=DEV),
                 sv=torch.full((C,), 0.125, dtype=dtype, device=DEV), da=torch.full((C, 3), 2.0, dtype=F64, device=DEV),
                 tab=torch.ones(n, 3, dtype=F64, device=DEV), mean=torch.full((C, pl.P), 4.0, dtype=F64, device=DEV),
                 M2=torch.full((C, pl.P) if kind == DIAG else (C, pl.P, pl.P), 5.0, dtype=F64, device=DEV))
        b["metric"] = (torch.ones(pl.P, dtype=dtype, device=DEV) if kind == DIAG
                       else torch.eye(pl.P, dtype=dtype, device=DEV).contiguous())
        return b

    def untouched(b):
        torch.cuda.synchronize()
        return all(bool((b[k] == v).all()) for k, v in (("th", 0.25), ("tv", -7.0), ("gr", 0.5), ("acc", 9), ("sv", 0.125),
                                                        ("da", 2.0), ("mean", 4.0), ("M2", 5.0)))

    def raw(pl, b, kind, n_iters=n, L=3, sv="sv", da="da", tab="tab", da_n=n, mean="mean", M2="M2", form=None, count=0):
        g = lambda k: None if k is None else Lb.ptr(b[k])  # noqa: E731
        return Lb.lib().ey_hmc_metric_warmup(
            pl.handle, g("th"), g("tv"), g("gr"), g("metric"), kind if form is None else form, 1, None, 0.1, g(sv), L, None,
            C, 0, 0, 0, 0, n_iters, None, None, None, None, g("acc"), g(da), g(tab), da_n, 0.8, nan, 0, g(mean), g(M2), count,
            None, None, _stream(pl.device))

    err = lambda: Lb.lib().ey_last_error()  # noqa: E731
    pl = _plan("mix2_2", F64)
    for kind in (DIAG, TRIL):
        b = buffers(pl, F64, kind)
        assert raw(pl, b, kind, n_iters=0) == -1 and b"n_iters" in err()
        assert raw(pl, b, kind, L=0) == -1 and b"num_steps" in err()
        assert raw(pl, b, kind, sv=None) == -1 and b"needs step_vec" in err()
        assert raw(pl, b, kind, mean=None) == -1 and b"exactly one" in err()
        assert raw(pl, b, kind, M2=None) == -1 and b"exactly one" in err()
        assert raw(pl, b, kind, tab=None) == -1 and b"needs its table" in err()
        assert raw(pl, b, kind, da_n=0) == -1 and raw(pl, b, kind, da_n=n + 1) == -1 and b"da_n" in err()
        assert raw(pl, b, kind, form=2) == -1 and b"EY_METRIC_DIAG or EY_METRIC_TRIL" in err()
        assert raw(pl, b, kind, count=-1) == -1 and b"count" in err()
        assert untouched(b)
        # the Plan method
        kw = dict(step_vec=b["sv"], da_state=b["da"], da_table=b["tab"], mean=b["mean"], M2=b["M2"],
                  out=dict(accepted=b["acc"]))
        name = "diag" if kind == DIAG else "dense"
        with pytest.raises(ValueError, match="n_iters"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], name, 0, **dict(kw, da_state=None))
        with pytest.raises(ValueError, match="num_steps"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 0, b["metric"], name, n, **kw)
        with pytest.raises(ValueError, match="needs step_vec"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.1, 3, b["metric"], name, n, **dict(kw, step_vec=None))
        with pytest.raises(ValueError, match="exactly one"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], name, n, **dict(kw, M2=None))
        with pytest.raises(ValueError, match="needs its table"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], name, n, **dict(kw, da_table=None))
        with pytest.raises(ValueError, match="'diag' or 'dense'"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], "full", n, **kw)
        with pytest.raises(ValueError, match="M2 must be"):
            pl.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], name, n, **dict(kw, M2=b["M2"].float()))
        assert untouched(b)
    # a dense form at P = 129: LR on 128 inputs with a bias
    dims, acts, lik = [128, 1], [1], 0
    x, y = _data(dims, lik, 64)
    big = _mlp_plan(dims, acts, lik, x, y, F32)
    assert big.P == 129
    b = buffers(big, F32, TRIL)
    assert raw(big, b, TRIL) == -2 and b"HMC with a dense metric" in err()
    with pytest.raises(RuntimeError, match="status -2"):
        big.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], "dense", n, step_vec=b["sv"], da_state=b["da"],
                              da_table=b["tab"], mean=b["mean"], M2=b["M2"], out=dict(accepted=b["acc"]))
    assert untouched(b)
    # a plan of a fused family with ey_plan_attach_da attached
    dims, acts, lik, N = CASES["mlp483"]
    x, y = _data(dims, lik, N)
    fused = _mlp_plan(dims, acts, lik, x, y, F32)
    assert fused.kernel == "fused16"
    b = buffers(fused, F32, DIAG)
    state, sv = torch.zeros(C, 3, dtype=F64, device=DEV), torch.full((C,), 0.05, dtype=F32, device=DEV)
    fused.attach_da(state, sv, torch.ones(n, 3, dtype=F64, device=DEV), n, 0.65)
    try:
        assert raw(fused, b, DIAG) == -1 and b"dual-averaging" in err()
        with pytest.raises(ValueError, match="dual-averaging"):
            fused.hmc_metric_warmup(b["th"], b["tv"], b["gr"], 0.0, 3, b["metric"], "diag", n, step_vec=b["sv"],
                                    out=dict(accepted=b["acc"]))
        assert untouched(b) and (state == 0).all() and (sv == 0.05).all()
    finally:
        fused.detach_da()
    t0, g0 = fused.log_target_grad(b["th"])
    out = fused.hmc_metric_warmup(b["th"].clone(), t0, g0, 0.01, 3, b["metric"], "diag", 2, seed=1)
    assert fused.kernel == "fused16" and out["accepted"].shape == (C,)


# ------------------------------------------------------------------------------------------------ 8. the sampler
BURN, SAMPLE, C_S, L_S, SEED_S = 100, 20, 16, 4, 6


def _sampler(fused_block, epochs=BURN + SAMPLE, **kw):
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.samplers import HMC
    m, _ = _mvn2()
    args = dict(theta0=_theta0(C_S), dataloader=_loader(), seed=SEED_S, metric='dense',
                tuner=WindowedAdaptation(num_steps=L_S), chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    args.update(kw)
    s = HMC(m, **args)
    s.fused_block = fused_block
    if epochs:
        s.run(num_epochs=epochs, num_burnin_epochs=min(BURN, epochs))
    return s


def test_the_sampler_is_its_own_hand_driven_calls():
    from eeyore_amd.samplers import HMC, DenseMetric
    a, b = _sampler(16), _sampler(256)
    # fused_block = 16 and 256 give the same bits
    for x, y in ((a._theta, b._theta), (a._target, b._target), (a._grad, b._grad), (a.step, b.step), (a._metric, b._metric),
                 (a.get_chain().get_samples(), b.get_chain().get_samples())):
        assert torch.equal(x, y)
    assert isinstance(a.metric, DenseMetric) and torch.equal(a.metric.scale_tril, a._metric)
    assert a.get_chain().get_samples().shape == (SAMPLE, C_S, 2) and tuple(a.step.shape) == (C_S,)
    # the metric changed at the window end, and nowhere else
    tuner = a.tuner
    assert tuner.windows(BURN) == [(15, 90)]
    assert tuner.history == [dict(draw=90, failed=0, updated=True)]
    assert not torch.equal(a._metric, torch.eye(2, dtype=F64, device=DEV))
    # the hand-driven loop: the Plan's calls along tuner.windows, every phase one launch
    h = _sampler(0, epochs=0, tuner=None, num_steps=L_S)
    plan = h.model._plan(*next(iter(h.dataloader)))
    th, tv, gr = h._theta, h._target, h._grad
    sched = WindowedAdaptation(num_steps=L_S)

    def search(k):
        return h.init_step_per_chain(th, momentum=plan.philox_normal(C_S, SEED_S, sched.SEARCH_ITER + k)).contiguous()

    step = search(0)
    state, t = sched.restart(step), 1
    mean, M2 = torch.zeros(C_S, 2, dtype=F64, device=DEV), torch.zeros(C_S, 2, 2, dtype=F64, device=DEV)
    (w0, w1), = sched.windows(BURN)
    metrics = []
    for s0, s1, adapts in ((0, w0, False), (w0, w1, True), (w1, BURN, False)):
        plan.hmc_metric_warmup(th, tv, gr, 0.0, L_S, h._metric, 'dense', s1 - s0, step_vec=step, seed=SEED_S, it=s0,
                               da_state=state, da_table=sched.table(t, s1 - s0, DEV), d=0.8, final_avg=s1 == BURN,
                               mean=mean if adapts else None, M2=M2 if adapts else None, count=0)
        t += s1 - s0
        metrics.append(h._metric.clone())
        if adapts:
            table, status = plan.metric_from_moments(mean, M2, s1 - s0, 'dense', pooled=True)
            assert int(status.sum()) == 0
            h._set_metric(DenseMetric(table))
            step = search(s1)
            state, t = sched.restart(step), 1
    assert torch.equal(metrics[0], metrics[1]) and torch.equal(metrics[0], torch.eye(2, dtype=F64, device=DEV))
    rec = torch.empty(SAMPLE, C_S, 2, dtype=F64, device=DEV)
    plan.hmc_metric_run(th, tv, gr, 0.0, L_S, h._metric, 'dense', SAMPLE, step_vec=step, seed=SEED_S, it=BURN, samples=rec)
    for x, y in ((a._theta, th), (a._target, tv), (a._grad, gr), (a.step, step), (a._metric, h._metric),
                 (a.get_chain().get_samples(), rec), (a.tuner.state, state)):
        assert torch.equal(x, y)
    # the sampling phase is a fresh sampler under the final metric and steps, from the warmed-up state at that iteration
    w = _sampler(256, epochs=BURN)
    assert torch.equal(w._metric, a._metric) and torch.equal(w.step, a.step)
    f = _sampler(256, epochs=0, tuner=None, num_steps=L_S, metric=w.metric, step=w.step, theta0=w._theta.clone())
    f._target.copy_(w._target)
    f._grad.copy_(w._grad)
    f._iter = BURN
    f.run(num_epochs=SAMPLE, num_burnin_epochs=0)
    assert torch.equal(f.get_chain().get_samples(), a.get_chain().get_samples())
    assert torch.equal(f.get_chain().get_accepted(), a.get_chain().get_accepted()) and torch.equal(f._theta, a._theta)
    assert float(a.get_chain().get_accepted().float().mean()) > 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_per_chain_estimates_with_a_temperature_vector(kind):
    """pooled=False: every chain ends with its own metric entry and step, under its own temperature."""
    from eeyore_amd.samplers import DenseMetric, DiagMetric
    temp = torch.linspace(0.4, 1.0, C_S, dtype=F64, device=DEV)
    runs = [_sampler(fb, metric=kind, tuner=WindowedAdaptation(num_steps=L_S, pooled=False), temperature=temp)
            for fb in (16, 256)]
    s = runs[0]
    assert torch.equal(s._metric, runs[1]._metric) and torch.equal(s._theta, runs[1]._theta)
    assert isinstance(s.metric, DiagMetric if kind == "diag" else DenseMetric) and s.metric.per_chain
    assert tuple(s._metric.shape) == ((C_S, 2) if kind == "diag" else (C_S, 2, 2)) and s._metric_index is None
    assert s.tuner.history == [dict(draw=90, failed=0, updated=True)]
    assert torch.isfinite(s._metric).all() and not torch.equal(s._metric[0], s._metric[1])
    assert torch.isfinite(s.step).all() and (s.step > 0).all() and tuple(s.step.shape) == (C_S,)
    assert float(s.get_chain().get_accepted().float().mean()) > 0.5


# ------------------------------------------------------------------------------------------------ 9. it adapts
@pytest.mark.parametrize("kind", KINDS)
def test_the_warm_up_whitens_an_ill_conditioned_gaussian(kind):
    """The scenario of tests/test_hmc_warmup_host.py on the device, for its seeds: the restatement ends below 5 there; the
    device runs other random streams, hence the factor of two."""
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.models import DistributionModel
    from eeyore_amd.models.targets import MultivariateNormal
    from eeyore_amd.samplers import HMC
    from tests.test_hmc_warmup_host import ADAPT, ADAPT_SEEDS, adapt_start
    for seed in ADAPT_SEEDS[CODE[kind]]:
        Sigma, _ = R.gaussian_case(CODE[kind], ADAPT["P"], ADAPT["cond"], seed)
        before = np.linalg.cond(Sigma)
        model = DistributionModel(MultivariateNormal(torch.zeros(ADAPT["P"], dtype=F64), torch.tensor(Sigma)), ADAPT["P"],
                                  dtype=F64, device=DEV)
        s = HMC(model, theta0=torch.tensor(adapt_start(seed), device=DEV), dataloader=_loader(), seed=seed, metric=kind,
                tuner=WindowedAdaptation(num_steps=ADAPT["num_steps"], d=ADAPT["d"]),
                chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
        s.run(num_epochs=ADAPT["n"] + 100, num_burnin_epochs=ADAPT["n"])
        after = R.whitened_condition(Sigma, CODE[kind], _np(s._metric))
        rate = float(s.get_chain().get_accepted().float().mean())
        steps = _np(s.step)
        print(f"{kind} seed {seed}: cond(Sigma) {before:.1f} -> {after:.3f}; steps {steps.min():.3f} .. {steps.max():.3f}; "
              f"acceptance of 100 draws after the warm-up {rate:.3f}; window ends {[h['draw'] for h in s.tuner.history]}")
        assert before > 100 and after < 10
        assert np.isfinite(steps).all() and (steps > 0).all() and steps.shape == (ADAPT["C"],)
        assert rate >= 0.6
        assert [h['draw'] for h in s.tuner.history] == [100, 150, 250] and all(h['updated'] for h in s.tuner.history)


# ------------------------------------------------------------------------------------------------ 10. the example
def test_example_runs():
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="300", EEYORE_EXAMPLE_CHAINS="256", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mvn_hmc_windowed_warmup.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rates = [float(v) for v in re.findall(r"acceptance rate \(mean over chains\): ([0-9.]+)", out.stdout)]
    assert "identity mass" in out.stdout and "windowed warm-up" in out.stdout and len(rates) == 2, out.stdout
    assert rates[0] > 0.5 and rates[1] > 0.5, out.stdout
    assert "nan" not in out.stdout
