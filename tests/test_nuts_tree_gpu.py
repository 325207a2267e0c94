"""NUTS with the tree in device memory (EY_NUTS_TREE_DEVICE, k_nuts_ws in eeyore_amd/csrc/ey_nuts_ws.hip)
against the numpy restatement beyond 128 parameters (tests/nuts_tree_cases.py, the margin rule and tolerances of
tests/test_nuts_gpu.py), against k_nuts bit for bit where both serve, and against itself: the run and its steps, what the
workspace held, the warm-up, the refusals, invariance of a known target, and the sampler."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import hmc_warmup_restatement as R
from tests import invariance as iv
from tests import nuts_cases as nc
from tests import nuts_tree_cases as tc
from tests import test_nuts_gpu as G
from tests import test_nuts_invariance_gpu as I
from tests.hmc_metric_restatement import DIAG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV, F64, F32 = G.DEV, G.F64, G.F32
FLAG = L.EY_NUTS_TREE_DEVICE
SEED, IT0, K_RUN = G.SEED, G.IT0, G.K_RUN
M141, IRIS = "mlp8-14-1/diag", "iris4-32-32-3/diag"
_t, _np = G._t, G._np


@functools.lru_cache(maxsize=None)
def _plan(name, dtype):
    from eeyore_amd.plan import Plan
    case = tc.CASES[name]
    pl = Plan(case["dims"], [1] * len(case["acts"]), case["acts"], case["lik"], dtype, DEV)
    X, Y = tc.data(name)
    pl.set_data(_t(X, dtype), _t(Y, dtype))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    assert pl.P == tc.num_params(name)
    return pl


def _device(name, dtype, chains=slice(None)):
    d = tc.inputs(name)
    return dict(th=_t(d["theta"][chains], dtype), steps=_t(d["steps"][chains], dtype), M=_t(d["metric"][1], dtype),
                kind="diag", temp=None)


def _bits_equal(xs, ys):
    for x, y in zip(xs, ys):
        assert x.dtype == y.dtype and torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 1. parity beyond 128
@pytest.mark.parametrize("name", list(tc.CASES))
def test_parity_with_given_randoms(name):
    """f64, explicit v0 / u, a step per chain, consecutive draws: exact outcomes, 1e-10 in the values, at most 5 % of the
    (chain, draw) pairs set aside by the margin rule."""
    case = tc.CASES[name]
    pl, dev, d = _plan(name, F64), _device(name, F64), tc.inputs(name)
    pl.attach_nuts_tree(case["C"], case["max_depth"])
    th, tv, gr = G._start(pl, dev)
    ref = tc.restate(name, start=(_np(th), _np(tv), _np(gr)))
    v0, u = _t(d["v0"], F64), _t(d["u"], F64)
    outs, states = [], []
    for k in range(case["draws"]):
        out = pl.nuts_step(th, tv, gr, 0.0, case["max_depth"], dev["M"], "diag", v0=v0[k], u=u[k], step_vec=dev["steps"],
                           flags=FLAG)
        outs.append({key: v.clone() for key, v in out.items()})
        states.append((_np(th), _np(tv), _np(gr)))
    n = G._compare(name, outs, states, ref)
    depths = np.stack([o["depth"].cpu().numpy() for o in outs])
    total = case["C"] * case["draws"]
    print(f"{name}: {n} of {total} draws compared, depths "
          f"{np.bincount(depths.ravel(), minlength=case['max_depth'] + 1).tolist()}, "
          f"divergent {int(sum(o['divergent'].sum() for o in outs))}")
    assert n >= (1 - tc.MAX_UNDER) * total
    assert int(sum(o["divergent"].sum() for o in outs)) >= 1 and (depths == case["max_depth"]).any() and (depths == 0).any()


# ------------------------------------------------------------------------------------------------ 2. k_nuts's bits
MVN64 = "mvn64/diag"   # P = 64 = Ppad in both kernels: no lane owns padding, the criterion runs exactly one full round


@functools.lru_cache(maxsize=None)
def _mvn64(dtype):
    """The plan and the device arguments (as G._device) of one normal target at P = 64, by the recipe of
    tests/nuts_cases.py: 4 chains whose steps are 0.02, 0.3, 0.9 and 100 times the stability limit under the metric."""
    from eeyore_amd.plan import Plan
    P, C = 64, 4
    rng = np.random.default_rng([P, 17])
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    cov = A @ A.T + 0.5 * np.eye(P)
    tgt = iv.Target([1.0], rng.standard_normal((1, P)), ((cov + cov.T) / 2)[None])
    s = 0.5 + rng.random(P)
    M = s[:, None] * tgt.prec[0] * s[None, :]
    limit = 2.0 / np.sqrt(np.linalg.eigvalsh((M + M.T) / 2).max())
    pl = Plan.mixture(tgt.c, tgt.mean, tgt.prec, dtype, DEV)
    assert pl.P == P
    return pl, dict(th=_t(iv.exact_draws(tgt, C, rng), dtype), steps=_t(limit * np.array([0.02, 0.3, 0.9, 100.0]), dtype),
                    M=_t(s, dtype), kind="diag", temp=None)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["mvn70/diag", "mvn128/diag", "xor/diag", MVN64])
def test_small_p_gives_the_bits_of_the_tree_in_lds(name, dtype):
    """K draws of nuts_run on the in-kernel streams with the flag and without: every output, record and the state.  K = 6
    draws of the 11 chains of a case of tests/nuts_cases.py at its max_depth 5; at P = 64, 3 draws of 4 chains at max_depth
    3, where the first chain's 7 leaves of a fiftieth of the stability limit never turn: every sub-block check runs."""
    if name == MVN64:
        (pl, dev), C, max_depth, K = _mvn64(dtype), 4, 3, 3
    else:
        pl, dev, C, max_depth, K = G._plan(name, dtype), G._device(name, dtype), nc.C, nc.MAX_DEPTH, K_RUN
    P = pl.P
    a = G._start(pl, dev)
    b = tuple(t.clone() for t in a)
    ra, rb = G._run_records(C, P, dtype, K), G._run_records(C, P, dtype, K)
    kw = dict(step_vec=dev["steps"], temp=dev["temp"], seed=SEED, it=IT0)
    oa = pl.nuts_run(*a, 0.0, max_depth, dev["M"], "diag", K, **kw, **ra)
    pl.attach_nuts_tree(C, max_depth)
    try:
        ob = pl.nuts_run(*b, 0.0, max_depth, dev["M"], "diag", K, flags=FLAG, **kw, **rb)
        torch.cuda.synchronize()
    finally:
        pl.detach_nuts_tree()
    _bits_equal(list(a) + [ra[k] for k in ra] + [oa[k] for k in oa], list(b) + [rb[k] for k in ra] + [ob[k] for k in oa])
    depths = np.bincount(ra["depth_rec"].cpu().numpy().ravel(), minlength=max_depth + 1)
    assert int(ra["accepted_rec"].sum()) > 0, depths
    if name == MVN64:
        assert depths[max_depth] >= K and depths[0] >= K, depths   # the first chain never turns, the last diverges at once
    else:
        assert (depths > 0).sum() >= 4, depths


# ------------------------------------------------------------------------------------------------ 3. run against step
def _run_vs_steps(name, dtype, chains, max_depth, n):
    pl = _plan(name, dtype)
    dev = _device(name, dtype, chains)
    C = dev["th"].shape[0]
    pl.attach_nuts_tree(C, max_depth)
    a = G._start(pl, dev)
    b = tuple(t.clone() for t in a)
    rec = G._run_records(C, pl.P, dtype, n)
    kw = dict(step_vec=dev["steps"], seed=SEED, flags=FLAG)
    oa = pl.nuts_run(*a, 0.0, max_depth, dev["M"], "diag", n, it=IT0, **kw, **rec)
    moved = 0
    for k in range(n):
        ob = pl.nuts_step(*b, 0.0, max_depth, dev["M"], "diag", it=IT0 + k, **kw)
        assert torch.equal(rec["samples"][k], b[0]) and torch.equal(rec["targets"][k], b[1]), k
        assert torch.equal(rec["accepted_rec"][k], ob["accepted"]) and torch.equal(rec["depth_rec"][k], ob["depth"]), k
        assert torch.equal(rec["divergent_rec"][k], ob["divergent"]), k
        moved += int(ob["accepted"].sum())
    _bits_equal(list(a) + [oa[key] for key in oa], list(b) + [ob[key] for key in oa])
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0)) and moved > 0
    assert torch.isfinite(rec["samples"]).all()


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_run_is_its_steps_bit_for_bit(dtype, C):
    _run_vs_steps(M141, dtype, slice(6, 7) if C == 1 else slice(None), 5, K_RUN)


def test_run_is_its_steps_bit_for_bit_at_1315_parameters():
    _run_vs_steps(IRIS, F32, slice(2, 5), 4, 2)


# ------------------------------------------------------------------------------------------------ 4. the workspace
def _four_draws(pl, dev, C):
    st = G._start(pl, dev)
    rec = G._run_records(C, pl.P, F64, 4)
    out = pl.nuts_run(*st, 0.0, 5, dev["M"], "diag", 4, step_vec=dev["steps"], seed=SEED, it=IT0, flags=FLAG, **rec)
    torch.cuda.synchronize()
    return list(st) + [rec[k] for k in rec] + [out[k] for k in sorted(out)]


def test_results_do_not_depend_on_what_the_workspace_holds_or_on_its_size():
    pl, dev = _plan(M141, F64), _device(M141, F64)
    C = 11
    pl.detach_nuts_tree()
    ws = pl.attach_nuts_tree(C, 5)
    assert ws.dtype == torch.uint8 and ws.numel() == pl.nuts_tree_bytes(C, 5) and pl._nuts_tree is ws
    ws.fill_(0xFF)   # every element a NaN
    assert torch.isnan(ws.view(F64)).all()
    nan_run = _four_draws(pl, dev, C)
    assert pl._nuts_tree is ws    # (the sampler's own attach neither moved nor shrank it)
    ws.zero_()
    zero_run = _four_draws(pl, dev, C)
    _bits_equal(nan_run, zero_run)
    # attached for 32 chains, used by 11: it grows, and the chains of a smaller call sit where they sat
    big = pl.attach_nuts_tree(32, 5)
    assert big is not ws and big.numel() == pl.nuts_tree_bytes(32, 5)
    assert pl.attach_nuts_tree(C, 5) is big and pl.attach_nuts_tree(C, 3) is big   # never shrinks
    big.fill_(0xFF)
    _bits_equal(nan_run, _four_draws(pl, dev, C))
    assert int(nan_run[3 + 2].sum()) > 0   # (accepted_rec: the chains moved)
    pl.detach_nuts_tree()
    assert pl._nuts_tree is None


def test_tree_bytes():
    """nvec Ppad esz C, monotone in C and max_depth."""
    for name, dtype, esz in ((M141, F64, 8), (M141, F32, 4), (IRIS, F32, 4)):
        pl = _plan(name, dtype)
        ppad = (pl.P + 63) // 64 * 64
        assert ppad >= pl.P and ppad % 64 == 0
        for C in (1, 7, 4096):
            for depth in (1, 4, 10):
                assert pl.nuts_tree_bytes(C, depth) == (12 + 2 * depth) * ppad * esz * C
            assert pl.nuts_tree_bytes(C, 5) < pl.nuts_tree_bytes(C, 6) and pl.nuts_tree_bytes(C, 5) < pl.nuts_tree_bytes(C + 1, 5)
    assert _plan(IRIS, F32).nuts_tree_bytes(4096, 6) == 24 * 1344 * 4 * 4096
    assert pl.nuts_tree_bytes(0, 5) == 0
    for bad in (0, 11):
        with pytest.raises(ValueError, match="max_depth"):
            pl.nuts_tree_bytes(4, bad)
    # beyond 2^31 bytes the count is still exact
    assert pl.nuts_tree_bytes(1 << 20, 10) == 32 * 1344 * 4 * (1 << 20)


# ------------------------------------------------------------------------------------------------ 5. the warm-up
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_warmup_with_nothing_attached_is_the_run(dtype):
    pl, dev = _plan(M141, dtype), _device(M141, dtype)
    pl.attach_nuts_tree(11, 5)
    a = G._start(pl, dev)
    b = tuple(t.clone() for t in a)
    ra, rb = G._run_records(11, pl.P, dtype, K_RUN), G._run_records(11, pl.P, dtype, K_RUN)
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0, flags=FLAG)
    oa = pl.nuts_run(*a, 0.0, 5, dev["M"], "diag", K_RUN, **kw, **ra)
    ob = pl.nuts_warmup(*b, 0.0, 5, dev["M"], "diag", K_RUN, **kw, **rb)
    _bits_equal(list(a) + [ra[k] for k in ra] + [oa[k] for k in oa], list(b) + [rb[k] for k in ra] + [ob[k] for k in oa])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_warmup_epilogues_against_the_host(dtype):
    """tests/test_nuts_gpu.py's test of the two epilogues, at P = 141 with the flag: the steps recorded are ey_da_update's
    recurrence replayed on the host from the recorded accept statistics (rtol 1e-6), the moments numpy's Welford of the
    recorded samples (1e-12 relative to the largest entry)."""
    from eeyore_amd.tuners import WindowedAdaptation
    pl, dev = _plan(M141, dtype), _device(M141, dtype)
    C, P, K_WARM, D_TARGET = 11, pl.P, G.K_WARM, G.D_TARGET
    pl.attach_nuts_tree(C, 5)
    dev["steps"] = dev["steps"][G.MID.start].expand(C).contiguous().clone()   # every chain from a step that moves
    state = G._start(pl, dev)
    rec = G._run_records(C, P, dtype, K_WARM)
    steps_rec, rate_rec = torch.empty(K_WARM, C, dtype=dtype, device=DEV), torch.empty(K_WARM, C, dtype=dtype, device=DEV)
    step_vec = dev["steps"].clone()
    tuner = WindowedAdaptation(num_steps=1)
    da_state = tuner.restart(step_vec)
    mean, M2 = torch.zeros(C, P, dtype=F64, device=DEV), torch.zeros(C, P, dtype=F64, device=DEV)
    out = pl.nuts_warmup(*state, 0.0, 5, dev["M"], "diag", K_WARM, step_vec=step_vec, seed=SEED, it=IT0, flags=FLAG,
                         da_state=da_state, da_table=tuner.table(1, K_WARM, DEV), d=D_TARGET, final_avg=True, mean=mean,
                         M2=M2, count=0, steps_rec=steps_rec, rate_rec=rate_rec, **rec)
    assert torch.equal(steps_rec[0], dev["steps"])
    bits = torch.int64 if dtype == F64 else torch.int32
    assert torch.equal(rate_rec[-1].contiguous().view(bits), out["accept_stat"].view(bits))
    rates, steps = _np(rate_rec), _np(steps_rec)
    for c in range(C):
        st = R.da_restart(float(dev["steps"][c]))
        for k in range(K_WARM):
            st, nxt = R.da_update(st, k + 1, rates[k, c], D_TARGET, averaged=k == K_WARM - 1)
            got = steps[k + 1, c] if k + 1 < K_WARM else float(step_vec[c])
            assert abs(got - nxt) <= 1e-6 * nxt, (c, k, got, nxt)
        np.testing.assert_allclose(_np(da_state[c, :2]), st[:2], rtol=1e-9, atol=1e-12)
    # (the accept statistic is 0 by definition for a draw whose first leaf diverges, and by rounding where every leaf's
    # energy error is below -104 in f32 -- exp underflows long before the divergence bound of -1000; the dual averaging's
    # first steps, from mu = log(10 step), reach such draws at this P: [0, 1] is the range, and zeros are rare)
    assert len(np.unique(steps[-1])) > 1 and (rates >= 0).all() and (rates <= 1).all()
    assert (rates > 0).mean() > 0.8
    want_mean, want_M2 = R.welford_chains(_np(rec["samples"]), DIAG)
    np.testing.assert_allclose(_np(M2), want_M2, rtol=1e-12, atol=1e-12 * np.abs(want_M2).max())
    np.testing.assert_allclose(_np(mean), want_mean, rtol=1e-12, atol=1e-12 * np.abs(want_mean).max())
    assert int(rec["accepted_rec"].sum()) > 0


# ------------------------------------------------------------------------------------------------ 6. refusals
def _raw_step(pl, th, tv, gr, M, form, max_depth, flags, acc):
    from eeyore_amd.plan import _stream
    C = th.shape[0]
    return L.lib().ey_nuts_step(pl.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(M), form, 1, None, None, None, 0, 0.05,
                                None, max_depth, None, C, SEED, 0, 0, flags, L.ptr(acc), None, None, None, None, None,
                                _stream(pl.device))


def test_refusals_leave_everything_untouched():
    from eeyore_amd.plan import Plan
    err = lambda: L.lib().ey_last_error()  # noqa: E731
    # P = 70: the dense form serves it, so the flag is what is refused
    pl, dev = G._plan("mvn70/diag", F64), G._device("mvn70/diag", F64, slice(0, 5))
    th, tv, gr = G._start(pl, dev)
    before = tuple(t.clone() for t in (th, tv, gr))
    acc = torch.full((5,), 7, dtype=torch.uint8, device=DEV)
    out = dict(accepted=acc, depth=torch.full((5,), -3, dtype=torch.int32, device=DEV))
    tril = torch.eye(70, dtype=F64, device=DEV)
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0, flags=FLAG)

    def untouched():
        torch.cuda.synchronize()
        return (all(torch.equal(x, y) for x, y in zip((th, tv, gr), before)) and bool((acc == 7).all())
                and bool((out["depth"] == -3).all()))

    pl.detach_nuts_tree()
    # the flag with nothing attached
    with pytest.raises(ValueError, match="ey_plan_attach_nuts_tree"):
        pl.nuts_step(th, tv, gr, 0.0, 3, dev["M"], "diag", out=out, **kw)
    assert _raw_step(pl, th[:4], tv[:4], gr[:4], dev["M"], L.EY_METRIC_DIAG, 3, FLAG, acc[:4]) == -1
    assert b"ey_plan_attach_nuts_tree" in err() and untouched()
    try:
        pl.attach_nuts_tree(4, 3)
        # the flag with a dense metric, workspace or not
        with pytest.raises(ValueError, match="diagonal metric only"):
            pl.nuts_step(th[:4], tv[:4], gr[:4], 0.05, 3, tril, "dense", seed=SEED, flags=FLAG,
                         out=dict(accepted=acc[:4], depth=out["depth"][:4]))
        assert _raw_step(pl, th[:4], tv[:4], gr[:4], tril, L.EY_METRIC_TRIL, 3, FLAG, acc[:4]) == -1 and untouched()
        # attached for (C = 4, depth 3): one chain more, one doubling more; the message names both counts
        have, need5, need4 = pl.nuts_tree_bytes(4, 3), pl.nuts_tree_bytes(5, 3), pl.nuts_tree_bytes(4, 4)
        with pytest.raises(ValueError, match=f"{have} bytes is smaller than the {need5} bytes"):
            pl.nuts_step(th, tv, gr, 0.0, 3, dev["M"], "diag", out=out, **kw)
        with pytest.raises(ValueError, match=f"{have} bytes is smaller than the {need4} bytes"):
            pl.nuts_run(th[:4], tv[:4], gr[:4], 0.0, 4, dev["M"], "diag", 2, step_vec=dev["steps"][:4], seed=SEED,
                        flags=FLAG, out=dict(accepted=acc[:4], depth=out["depth"][:4]))
        with pytest.raises(ValueError, match="is smaller than"):
            pl.nuts_warmup(th[:4], tv[:4], gr[:4], 0.0, 4, dev["M"], "diag", 2, step_vec=dev["steps"][:4], seed=SEED,
                           flags=FLAG, out=dict(accepted=acc[:4], depth=out["depth"][:4]))
        assert _raw_step(pl, th, tv, gr, dev["M"], L.EY_METRIC_DIAG, 3, FLAG, acc) == -1 and untouched()
        # ... and what it was attached for is served
        o = pl.nuts_step(th[:4].clone(), tv[:4].clone(), gr[:4].clone(), 0.0, 3, dev["M"], "diag", step_vec=dev["steps"][:4],
                         seed=SEED, it=IT0, flags=FLAG)
        assert int(o["depth"].max()) == 3
        # without the flag, the attached workspace changes nothing: k_nuts's bits at P = 70
        a, b = tuple(t.clone() for t in before), tuple(t.clone() for t in before)
        kw0 = dict(step_vec=dev["steps"], seed=SEED, it=IT0)
        ob = pl.nuts_step(*b, 0.0, 5, dev["M"], "diag", **kw0)
        pl.detach_nuts_tree()
        oa = pl.nuts_step(*a, 0.0, 5, dev["M"], "diag", **kw0)
        _bits_equal(list(a) + [oa[k] for k in oa], list(b) + [ob[k] for k in oa])
        assert untouched()
    finally:
        pl.detach_nuts_tree()
    # P = 129 without the flag, after a workspace was attached and detached: refused as before, by Plan and by the library
    big = Plan([128, 1], [1], [1], 0, F64, DEV)
    assert big.P == 129
    big.set_data(torch.zeros(4, 128, dtype=F64, device=DEV), torch.zeros(4, 1, dtype=F64, device=DEV))
    big.set_prior(torch.zeros(big.P), torch.ones(big.P))
    thb = torch.zeros(3, 129, dtype=F64, device=DEV)
    tb, gb = big.log_target_grad(thb)
    ones, accb = torch.ones(129, dtype=F64, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV)
    big.attach_nuts_tree(3, 5)
    assert _raw_step(big, thb, tb, gb, ones, L.EY_METRIC_DIAG, 5, 0, accb) == -2   # attached, but not asked for
    assert b"exceeds the limit of 128 parameters" in err()
    big.detach_nuts_tree()
    with pytest.raises(ValueError, match="128 parameters"):
        big.nuts_step(thb, tb, gb, 0.1, 5, ones, "diag", seed=SEED)
    assert _raw_step(big, thb, tb, gb, ones, L.EY_METRIC_DIAG, 5, 0, accb) == -2
    assert b"exceeds the limit of 128 parameters" in err()
    assert _raw_step(big, thb, tb, gb, ones, L.EY_METRIC_DIAG, 5, FLAG, accb) == -1 and b"ey_plan_attach_nuts_tree" in err()
    torch.cuda.synchronize()
    assert bool((thb == 0).all()) and bool((accb == 0).all())


# ------------------------------------------------------------------------------------------------ 7. invariance
INV_TARGET, INV_KIND, INV_DTYPE = "mix2_2", "diag", "f64"
INV_THRESHOLD = iv.threshold(iv.n_features(iv.target_of(INV_TARGET).P))   # for the z-scores THIS file asserts on


def test_the_tree_in_device_memory_leaves_its_target_invariant():
    """The diagonal f64 case of tests/test_nuts_invariance_gpu.py on the P = 2 mixture, its step, seed rule and assertions,
    with the flag: 16384 chains, 16 draws, max_depth 5, a workspace of 22 x 64 x 8 x 16384 bytes."""
    C, N = I.C, I.N
    assert (C, N, I.MAX_DEPTH) == (16384, 16, 5)
    seed = I.SEED0 + 100
    tgt, dt = iv.target_of(INV_TARGET), I.DT[INV_DTYPE]
    pl = I._plan(INV_TARGET, INV_DTYPE)
    rng = np.random.default_rng([seed, 1])
    th = I._t(iv.exact_draws(tgt, C, rng), dt)
    tv, gr = pl.log_target_grad(th)
    tv, gr = tv.contiguous(), gr.contiguous()
    count = torch.zeros(C, dtype=torch.int32, device=DEV)
    depth_rec = torch.empty(N, C, dtype=torch.int32, device=DEV)
    div_rec = torch.empty(N, C, dtype=torch.uint8, device=DEV)
    ws = pl.attach_nuts_tree(C, I.MAX_DEPTH)
    assert ws.numel() == 22 * 64 * 8 * C
    try:
        out = pl.nuts_run(th, tv, gr, I.STEPS[(INV_TARGET, INV_KIND)], I.MAX_DEPTH, I._t(I.table(INV_TARGET, INV_KIND), dt),
                          INV_KIND, N, seed=seed, accept_count=count, depth_rec=depth_rec, divergent_rec=div_rec, flags=FLAG)
        torch.cuda.synchronize()
    finally:
        pl.detach_nuts_tree()
    assert torch.isfinite(th).all() and torch.isfinite(tv).all()
    z = iv.z_scores(iv.features(I._np(th), I._np(tv)), iv.reference_moments(tgt, I.N_REF, rng))
    w, where = iv.worst(z[None], tgt.P)
    depths = np.bincount(depth_rec.cpu().numpy().ravel(), minlength=I.MAX_DEPTH + 1)
    moved, stat = float(count.double().mean()) / N, float(out["accept_stat"].double().mean())
    print(f"nuts, tree in device memory/{INV_TARGET}/{INV_KIND}/{INV_DTYPE}: largest |z| {w:.2f} ({where}), threshold "
          f"{INV_THRESHOLD:.2f}, moved {moved:.3f}, accept_stat of the last draw {stat:.3f}, depths {depths.tolist()}, "
          f"divergent {int(div_rec.sum())}")
    assert w < INV_THRESHOLD, (w, where)
    assert moved > 0.5 and 0.5 < stat < 0.995 and (depths[1:4] > 0).all() and int(div_rec.sum()) == 0
    t1, g1 = pl.log_target_grad(th.clone())
    np.testing.assert_allclose(I._np(tv), I._np(t1), rtol=1e-9, atol=1e-9)
    want = I._np(g1)
    np.testing.assert_allclose(I._np(gr), want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


# ------------------------------------------------------------------------------------------------ 8. the sampler
def test_the_sampler_warms_up_and_samples_the_iris_network():
    """NUTS(tree='device', tuner=WindowedAdaptation) on MLP(4-32-32-3) with the 12 Iris rows of the parity case: 64 chains,
    a warm-up of 30 draws with one metric window, 20 recorded draws."""
    from torch.distributions import Normal
    from torch.utils.data import DataLoader
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import NUTS, DiagMetric
    from eeyore_amd.tuners import WindowedAdaptation
    C, BURN, KEEP, DEPTH = 64, 30, 20, 5
    X, Y = tc.data(IRIS)
    data = XYDataset(_t(X, F32), _t(Y, F32))
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                                activations=[torch.sigmoid, torch.sigmoid, None]),
                    dtype=F32, device=DEV)
    P = model.num_params()
    assert P == 1315
    model.prior = Normal(torch.zeros(P, device=DEV), torch.ones(P, device=DEV))
    gen = torch.Generator().manual_seed(4)
    theta0 = (0.1 * torch.randn(C, P, generator=gen)).to(DEV)
    tuner = WindowedAdaptation(num_steps=1)
    s = NUTS(model, theta0=theta0, dataloader=DataLoader(data, batch_size=len(data), shuffle=False), tree='device',
             metric='diag', max_depth=DEPTH, tuner=tuner, seed=2,
             chain=ChainBuffer(keys=['sample', 'target_val', 'accepted', 'depth', 'divergent']))
    s.run(num_epochs=BURN + KEEP, num_burnin_epochs=BURN)
    torch.cuda.synchronize()
    chain = s.get_chain()
    assert len(chain) == KEEP and tuple(chain.get_samples().shape) == (KEEP, C, P)
    assert tuple(s.step.shape) == (C,) and bool(torch.isfinite(s.step).all()) and bool((s.step > 0).all())
    depth = chain.bufs['depth'][:KEEP]
    assert tuple(depth.shape) == (KEEP, C) and int(depth.min()) >= 0 and int(depth.max()) <= DEPTH and int(depth.max()) >= 2
    assert tuple(chain.bufs['divergent'][:KEEP].shape) == (KEEP, C)
    assert bool(torch.isfinite(chain.get_samples()).all()) and float(chain.acceptance_rate().mean()) > 0.5
    assert len(tuner.history) == len(tuner.windows(BURN)) >= 1
    assert isinstance(s.metric, DiagMetric) and not torch.equal(s._metric, torch.ones_like(s._metric))
    plan = model._plan(*next(iter(s.dataloader)))
    assert plan._nuts_tree is not None and plan._nuts_tree.numel() >= plan.nuts_tree_bytes(C, DEPTH)


def test_iris_nuts_example_runs():
    """examples/iris_nuts.py at reduced size, through the environment tests/test_examples.py uses."""
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="20", EEYORE_EXAMPLE_CHAINS="64", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "iris_nuts.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "cceptance rate" in out.stdout and "tree depths of the stored draws" in out.stdout
    assert "64 chains, 1315 parameters" in out.stdout and "steps " in out.stdout and "divergent draws" in out.stdout
