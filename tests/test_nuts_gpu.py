"""NUTS on the device (ey_nuts_step / ey_nuts_run / ey_nuts_warmup, k_nuts in eeyore_amd/csrc/ey_nuts.hip) against the
recursive numpy restatement (tests/nuts_restatement.py) on the cases of tests/nuts_cases.py, and against itself.

A NUTS draw is a chain of discontinuous decisions, so the comparison follows the restatement's margins: a draw whose
smallest decision margin is above 1e-9 must agree exactly in depth, n_leapfrog, divergent and accepted and to 1e-10 relative
(against the largest entry of the vector compared) in theta, target, grad, accept_stat and energy; a chain is followed
only up to its first draw under the margin, and at most 5 % of the (chain, draw) pairs may be lost that way
(tests/test_nuts_host.py holds the committed inputs to that with the restatement alone)."""
import functools

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from oracle import philox_oracle as po
from tests import hmc_warmup_restatement as R
from tests import nuts_cases as nc
from tests import nuts_restatement as nr
from tests.hmc_metric_restatement import DIAG, TRIL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
RTOL = 1e-10
SEED, IT0, K_RUN = 31, 5, 6


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _plan(name, dtype):
    from eeyore_amd.plan import Plan
    if nc.CASES[name].get("mlp"):
        pl = Plan(nc.XOR_DIMS, [1, 1], nc.XOR_ACTS, nc.XOR_LIK, dtype, DEV)
        pl.set_data(_t(nc.XOR_X, dtype), _t(nc.XOR_Y, dtype))
        pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    else:
        tgt = nc.target(name)
        pl = Plan.mixture(tgt.c, tgt.mean, tgt.prec, dtype, DEV)
    assert pl.P == nc.CASES[name]["P"]
    return pl


def _device(name, dtype, chains=slice(None)):
    """The case's device arguments for the chains selected: theta, steps, metric table, kind, temps."""
    d = nc.inputs(name)
    kind, table = d["metric"]
    return dict(th=_t(d["theta"][chains], dtype), steps=_t(d["steps"][chains], dtype), M=_t(table, dtype), kind=kind,
                temp=None if d["temps"] is None else _t(d["temps"][chains], dtype))


def _start(pl, dev):
    th = dev["th"].clone()
    tv, gr = pl.log_target_grad(th, temp=dev["temp"])
    return th, tv.contiguous(), gr.contiguous()


def _compare(name, outs_dev, states_dev, outs_ref):
    """The margin rule over the draws of a case.  Returns the number of (chain, draw) pairs compared."""
    C = len(outs_ref[0]["depth"])
    live = np.ones(C, bool)
    compared = 0
    for k, (od, sd, orf) in enumerate(zip(outs_dev, states_dev, outs_ref)):
        live &= orf["margin"] > nc.MARGIN
        compared += int(live.sum())
        if not live.any():
            break
        for key in nr.OUTCOME:
            got = od[key].cpu().numpy().astype(int)
            assert np.array_equal(got[live], orf[key][live]), (name, k, key, got, orf[key], orf["margin"])
        vals = dict(theta=sd[0], target=sd[1], grad=sd[2], accept_stat=_np(od["accept_stat"]), energy=_np(od["energy"]))
        for key in nr.VALUES:
            want, got = orf[key][live], vals[key][live]
            scale = np.abs(want).max(axis=-1, keepdims=True) if want.ndim == 2 else np.abs(want).max()
            err = np.abs(got - want)
            assert (err <= RTOL * scale).all(), (name, k, key, float((err / np.maximum(scale, 1e-300)).max()))
    return compared


def _draws_on_device(pl, dev, state, n, **kw):
    th, tv, gr = state
    outs, states = [], []
    for k in range(n):
        args = {key: (v[k] if key in ("v0", "u") else v) for key, v in kw.items()}
        if "it" in args:
            args["it"] = kw["it"] + k
        out = pl.nuts_step(th, tv, gr, 0.0, nc.MAX_DEPTH, dev["M"], dev["kind"], step_vec=dev["steps"], temp=dev["temp"],
                           **args)
        outs.append({key: v.clone() for key, v in out.items()})
        states.append((_np(th), _np(tv), _np(gr)))
    return outs, states


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(nc.CASES))
def test_parity_with_given_randoms(name):
    """f64, C = 11, max_depth = 5, explicit v0 / u, a step per chain: four consecutive draws."""
    pl = _plan(name, F64)
    dev = _device(name, F64)
    d = nc.inputs(name)
    state = _start(pl, dev)
    ref = nc.restate(name, start=tuple(_np(t) for t in state))
    v0, u = _t(d["v0"], F64), _t(d["u"], F64)
    outs, states = _draws_on_device(pl, dev, state, nc.DRAWS, v0=v0, u=u)
    n = _compare(name, outs, states, ref)
    depths = np.stack([o["depth"].cpu().numpy() for o in outs])
    print(f"{name}: {n} of {nc.C * nc.DRAWS} draws compared, depths {np.bincount(depths.ravel(), minlength=6).tolist()}, "
          f"divergent {int(sum(o['divergent'].sum() for o in outs))}")
    assert n >= (1 - nc.MAX_UNDER) * nc.C * nc.DRAWS
    assert int(sum(o["divergent"].sum() for o in outs)) >= 1 and (depths == nc.MAX_DEPTH).any() and (depths == 0).any()


@pytest.mark.parametrize("name", ["mvn5/dense", "mvn70/diag", "xor/diag"])
def test_parity_on_the_streams(name):
    """v0 = u = NULL in f64: the restatement on the Philox oracle's normals and uniform block words."""
    pl = _plan(name, F64)
    dev = _device(name, F64)
    P = pl.P
    state = _start(pl, dev)
    start = tuple(_np(t) for t in state)
    v0 = np.stack([po.normal(nc.C, P, SEED, IT0 + k, dtype=np.float64) for k in range(nc.DRAWS)])
    u = np.stack([po.uniform_blocks(np.arange(nc.C), nr.words(nc.MAX_DEPTH), SEED, IT0 + k, dtype=np.float64)
                  for k in range(nc.DRAWS)])
    ref = nc.restate(name, start=start, v0=v0, u=u)
    outs, states = _draws_on_device(pl, dev, state, nc.DRAWS, seed=SEED, it=IT0)
    n = _compare(name, outs, states, ref)
    print(f"{name} on the streams: {n} of {nc.C * nc.DRAWS} draws compared")
    assert n >= (1 - nc.MAX_UNDER) * nc.C * nc.DRAWS


# ------------------------------------------------------------------------------------------------ run against step
MID = slice(3, 10)   # the chains whose steps end by the U-turn criterion: a run of them moves


def _both_forms(kind, dtype, C):
    """(plan, dev) of the P = 5 normal under either metric form, C = 1 (chain 6) or 11."""
    name = "mvn5/dense"
    pl = _plan(name, dtype)
    dev = _device(name, dtype, slice(6, 7) if C == 1 else slice(None))
    if kind == "diag":
        dev["M"], dev["kind"] = _t(0.5 + np.random.default_rng(3).random(pl.P), dtype), "diag"
    return pl, dev


def _run_records(C, P, dtype, n):
    return dict(samples=torch.empty(n, C, P, dtype=dtype, device=DEV), targets=torch.empty(n, C, dtype=dtype, device=DEV),
                accepted_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV),
                accept_count=torch.zeros(C, dtype=torch.int32, device=DEV),
                depth_rec=torch.empty(n, C, dtype=torch.int32, device=DEV),
                divergent_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("kind", ["dense", "diag"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_run_is_its_steps_bit_for_bit(dtype, kind, C):
    pl, dev = _both_forms(kind, dtype, C)
    a = _start(pl, dev)
    b = tuple(t.clone() for t in a)
    rec = _run_records(C, pl.P, dtype, K_RUN)
    kw = dict(step_vec=dev["steps"], temp=dev["temp"], seed=SEED)
    oa = pl.nuts_run(*a, 0.0, nc.MAX_DEPTH, dev["M"], dev["kind"], K_RUN, it=IT0, **kw, **rec)
    moved = 0
    for k in range(K_RUN):
        ob = pl.nuts_step(*b, 0.0, nc.MAX_DEPTH, dev["M"], dev["kind"], it=IT0 + k, **kw)
        assert torch.equal(rec["samples"][k], b[0]) and torch.equal(rec["targets"][k], b[1]), k
        assert torch.equal(rec["accepted_rec"][k], ob["accepted"]) and torch.equal(rec["depth_rec"][k], ob["depth"]), k
        assert torch.equal(rec["divergent_rec"][k], ob["divergent"]), k
        moved += int(ob["accepted"].sum())
    for x, y in list(zip(a, b)) + [(oa[key], ob[key]) for key in oa]:
        assert torch.equal(x, y)
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0)) and moved > 0
    assert torch.isfinite(rec["samples"]).all()


def test_raising_max_depth_moves_no_variate():
    """max_depth 5 -> 7 on the streams: the draws that ended below depth 5 are the same bits."""
    pl, dev = _both_forms("dense", F64, 11)
    a, kw = _start(pl, dev), dict(step_vec=dev["steps"], temp=dev["temp"], seed=SEED, it=IT0)
    b = tuple(t.clone() for t in a)
    o5 = pl.nuts_step(*a, 0.0, 5, dev["M"], dev["kind"], **kw)
    o7 = pl.nuts_step(*b, 0.0, 7, dev["M"], dev["kind"], **kw)
    below = o5["depth"] < 5
    assert 3 <= int(below.sum()) < 11 and bool((o7["depth"][~below] >= 5).all())
    for x, y in list(zip(a, b)) + [(o5[key], o7[key]) for key in o5]:
        assert torch.equal(x[below], y[below])
    assert not torch.equal(a[0][~below], b[0][~below])   # (and the capped ones went on)


# ------------------------------------------------------------------------------------------------ the epilogues
D_TARGET, K_WARM = 0.8, 12


@pytest.mark.parametrize("kind", ["dense", "diag"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_warmup_with_nothing_attached_is_the_run(dtype, kind):
    pl, dev = _both_forms(kind, dtype, 11)
    a = _start(pl, dev)
    b = tuple(t.clone() for t in a)
    ra, rb = _run_records(11, pl.P, dtype, K_RUN), _run_records(11, pl.P, dtype, K_RUN)
    kw = dict(step_vec=dev["steps"], temp=dev["temp"], seed=SEED, it=IT0)
    oa = pl.nuts_run(*a, 0.0, nc.MAX_DEPTH, dev["M"], dev["kind"], K_RUN, **kw, **ra)
    ob = pl.nuts_warmup(*b, 0.0, nc.MAX_DEPTH, dev["M"], dev["kind"], K_RUN, **kw, **rb)
    for x, y in list(zip(a, b)) + [(ra[key], rb[key]) for key in ra] + [(oa[key], ob[key]) for key in oa]:
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["dense", "diag"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_warmup_epilogues_against_the_host(dtype, kind):
    """Dual averaging: the steps recorded are ey_da_update's recurrence replayed on the host from the recorded accept
    statistics (rtol 1e-6, tests/test_hmc_warmup_gpu.py's bound).  Moments: numpy Welford of the recorded samples (1e-12
    relative to the largest entry, that file's bound)."""
    from eeyore_amd.tuners import WindowedAdaptation
    pl, dev = _both_forms(kind, dtype, 11)
    C, P = 11, pl.P
    dev["steps"] = dev["steps"][MID.start].expand(C).contiguous().clone()   # every chain from a step that moves
    state = _start(pl, dev)
    rec = _run_records(C, P, dtype, K_WARM)
    steps_rec, rate_rec = torch.empty(K_WARM, C, dtype=dtype, device=DEV), torch.empty(K_WARM, C, dtype=dtype, device=DEV)
    step_vec = dev["steps"].clone()
    tuner = WindowedAdaptation(num_steps=1)
    da_state = tuner.restart(step_vec)
    mean = torch.zeros(C, P, dtype=F64, device=DEV)
    M2 = torch.zeros((C, P) if kind == "diag" else (C, P, P), dtype=F64, device=DEV)
    out = pl.nuts_warmup(*state, 0.0, nc.MAX_DEPTH, dev["M"], kind, K_WARM, step_vec=step_vec, temp=dev["temp"], seed=SEED,
                         it=IT0, da_state=da_state, da_table=tuner.table(1, K_WARM, DEV), d=D_TARGET, final_avg=True,
                         mean=mean, M2=M2, count=0, steps_rec=steps_rec, rate_rec=rate_rec, **rec)
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
    assert len(np.unique(steps[-1])) > 1 and (rates > 0).all() and (rates <= 1).all()
    want_mean, want_M2 = R.welford_chains(_np(rec["samples"]), DIAG if kind == "diag" else TRIL)
    got_M2 = _np(M2)
    if kind == "dense":
        got_M2, want_M2 = np.tril(got_M2), np.tril(want_M2)
    np.testing.assert_allclose(got_M2, want_M2, rtol=1e-12, atol=1e-12 * np.abs(want_M2).max())
    np.testing.assert_allclose(_np(mean), want_mean, rtol=1e-12, atol=1e-12 * np.abs(want_mean).max())
    assert int(rec["accepted_rec"].sum()) > 0


# ------------------------------------------------------------------------------------------------ refusals, non-finite
def test_refusals_leave_theta_untouched():
    from eeyore_amd.plan import Plan
    pl, dev = _both_forms("diag", F64, 11)
    th, tv, gr = _start(pl, dev)
    before = th.clone()
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0)
    for depth in (0, 11):
        with pytest.raises(ValueError, match="max_depth"):
            pl.nuts_step(th, tv, gr, 0.0, depth, dev["M"], "diag", **kw)
        with pytest.raises(ValueError, match="max_depth"):
            pl.nuts_run(th, tv, gr, 0.0, depth, dev["M"], "diag", 2, **kw)
    short = torch.rand(11, 20 + 2 ** 5, dtype=F64, device=DEV)
    with pytest.raises(ValueError, match="S >= 21"):
        pl.nuts_step(th, tv, gr, 0.0, 5, dev["M"], "diag", u=short, **kw)
    # a plan of a fused family with ey_plan_attach_da attached (tests/test_hmc_warmup_gpu.py's)
    from tests.test_ram_gpu import CASES, _data
    from tests.test_ram_gpu import _plan as _mlp_plan
    dims, acts, lik, n_rows = CASES["mlp483"]
    fused = _mlp_plan(dims, acts, lik, *_data(dims, lik, n_rows), F32)
    assert fused.kernel == "fused16"
    thf = torch.zeros(11, fused.P, dtype=F32, device=DEV)
    tf, gf = fused.log_target_grad(thf)
    ones = torch.ones(fused.P, dtype=F32, device=DEV)
    state, step_vec = torch.zeros(11, 3, dtype=F64, device=DEV), torch.full((11,), 0.05, dtype=F32, device=DEV)
    fused.attach_da(state, step_vec, torch.ones(4, 3, dtype=F64, device=DEV), 4, 0.65)
    try:
        for call in (lambda: fused.nuts_step(thf, tf, gf, 0.05, 5, ones, "diag", seed=SEED),
                     lambda: fused.nuts_warmup(thf, tf, gf, 0.05, 5, ones, "diag", 2, seed=SEED)):
            with pytest.raises(ValueError, match="ey_plan_attach_da"):
                call()
    finally:
        fused.detach_da()
    torch.cuda.synchronize()
    assert bool((thf == 0).all()) and bool((state == 0).all()) and bool((step_vec == 0.05).all())
    # (a distribution plan stops at 128 parameters itself: P = 129 is an MLP plan)
    big = Plan([128, 1], [1], [1], 0, F64, DEV)
    assert big.P == 129
    big.set_data(torch.zeros(4, 128, dtype=F64, device=DEV), torch.zeros(4, 1, dtype=F64, device=DEV))
    big.set_prior(torch.zeros(big.P), torch.ones(big.P))
    thb = torch.zeros(3, 129, dtype=F64, device=DEV)
    tb, gb = big.log_target_grad(thb)
    with pytest.raises(ValueError, match="128 parameters"):
        big.nuts_step(thb, tb, gb, 0.1, 5, torch.ones(129, dtype=F64, device=DEV), "diag", seed=SEED)
    # ... and the library's own refusal of that size, below the Python check: EY_ERR_UNSUPPORTED with nothing launched
    from eeyore_amd.plan import _stream
    ones, acc = torch.ones(129, dtype=F64, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV)
    rc = L.lib().ey_nuts_step(big.handle, L.ptr(thb), L.ptr(tb), L.ptr(gb), L.ptr(ones), L.EY_METRIC_DIAG, 1, None, None,
                              None, 0, 0.1, None, 5, None, 3, SEED, 0, 0, 0, L.ptr(acc), None, None, None, None, None,
                              _stream(big.device))
    assert rc == -2 and b"exceeds the limit of 128 parameters" in L.lib().ey_last_error()
    torch.cuda.synchronize()
    assert torch.equal(th, before) and bool((thb == 0).all())


def test_a_chain_that_starts_at_a_nan_target_stays_put():
    pl, dev = _both_forms("dense", F64, 11)
    a = _start(pl, dev)
    dev_b = dict(dev, th=dev["th"].clone())
    dev_b["th"][4] = float("nan")   # the target and gradient there are NaN: H0 is NaN, every leaf's energy error is
    b = _start(pl, dev_b)
    assert torch.isnan(b[1][4])
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0)
    oa = pl.nuts_step(*a, 0.0, 5, dev["M"], "dense", **kw)
    ob = pl.nuts_step(*b, 0.0, 5, dev["M"], "dense", **kw)
    assert int(ob["divergent"][4]) == 1 and int(ob["accepted"][4]) == 0 and int(ob["depth"][4]) == 0
    assert torch.isnan(b[0][4]).all() and torch.isnan(b[1][4])
    others = torch.arange(11, device=DEV) != 4
    for x, y in list(zip(a, b)) + [(oa[key], ob[key]) for key in oa]:
        assert torch.equal(x[others], y[others])
    assert int(oa["divergent"][4]) == 0
