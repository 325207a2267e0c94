"""NUTS on the matrix cores (EY_NUTS_FUSED, k_nuts_mfma in eeyore_amd/csrc/ey_nuts_mfma.hip) on the
MLP(4-32-32-dK) plans of tests/nuts_fused_cases.py: against the f64 restatement, against the parent's path on the same plan
(EY_NUTS_TREE_DEVICE alone: k_nuts_ws on the generic f32 evaluation), and against itself.

The plans are f32, so the comparison with the restatement cannot be to rounding of f64 as tests/test_nuts_tree_gpu.py's is.
The tolerances are MEASURED, not chosen: tests/tools/nuts_fused_margin_probe.py runs the parent's path on every case, each
draw from the restatement's f32 state, and prints per quantity the largest error against the restatement -- target, energy
and accept_stat absolutely, theta and the gradient relative to their largest entry.  TAU of a quantity is 8 times that
figure rounded up to one digit; the factor covers the other order of summation over the row tiles and the bf16x3 pieces, as
in tests/test_eslice_fused_gpu.py.  Every (draw, chain) pair of every case has a decision margin above MARGIN_FLOOR = 0.05 by
the restatement (tests/test_nuts_fused_host.py), and the TAUs of the quantities decisions are made on must not exceed it, so
every pair is compared: outcomes exactly, values within TAU.

Measured on the device (the probe), the parent's path, the largest over the six cases: target 5.81e-4 (the BCE
case, at a target near -3800), energy 6.80e-4, accept_stat 7.52e-5, theta 5.22e-7 and the gradient 7.86e-7 of the largest
entry; so TAU = 5e-3, 6e-3, 7e-4, 5e-6 and 7e-6.  The fused kernel's own largest errors on the same draws are 5.81e-4,
8.81e-4, 7.51e-5, 6.16e-7 and 8.24e-7, and neither path decides any of the 198 pairs otherwise than the restatement."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import nuts_fused_cases as nf
from tests import nuts_restatement as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
FUSED, DEVICE = L.EY_NUTS_FUSED, L.EY_NUTS_TREE_DEVICE
SEED, IT0, K_RUN = 31, 5, 6
# the probe's figures (the parent's path against the f64 restatement, the largest over the six cases) and 8 x each, rounded up
E_PARENT = dict(target=5.81e-4, energy=6.80e-4, accept_stat=7.52e-5, theta=5.22e-7, grad=7.86e-7)
TAU = dict(target=5e-3, energy=6e-3, accept_stat=7e-4, theta=5e-6, grad=7e-6)
OUTCOME, VALUES = nr.OUTCOME, nr.VALUES


def _t(a, dtype=F32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


def test_the_tolerances_are_eight_times_the_probes_figures_and_below_the_floor():
    import math
    for key, e in E_PARENT.items():
        digit = 10.0 ** math.floor(math.log10(8 * e))
        assert math.isclose(TAU[key], math.ceil(8 * e / digit - 1e-9) * digit, rel_tol=1e-9), key
    assert max(TAU["target"], TAU["energy"], TAU["accept_stat"]) <= nf.MARGIN_FLOOR


@functools.lru_cache(maxsize=None)
def plan_of(name):
    from eeyore_amd.plan import Plan
    d, model = nf.setup(name), nf.model_of(name)
    pl = Plan(model["dims"], [1, 1, 1], model["acts"], model["lik"], F32, DEV)
    pl.f32_products = d["products"]
    pl.set_data(_t(d["x"]), _t(d["y"]))
    pl.set_prior(torch.tensor(d["prior"][0]), torch.tensor(d["prior"][1]))
    assert pl.kernel == "mfma32" and pl.f32_products == d["products"] and pl.P == d["P"]
    return pl


def device_args(name, chains=slice(None)):
    d = nf.setup(name)
    if d["index"] is None:
        M, index = _t(d["tables"][0]), None
    else:
        M, index = _t(d["tables"]), torch.tensor(d["index"][chains], dtype=torch.int32, device=DEV)
    return dict(M=M, index=index, steps=_t(d["steps"][chains]), temp=None if d["temps"] is None else _t(d["temps"][chains]))


def _start(pl, dev, theta):
    th = _t(theta)
    tv, gr = pl.log_target_grad(th, temp=dev["temp"])
    return th, tv.contiguous(), gr.contiguous()


def draws_on_device(name, flags):
    """Each of the case's draws on the device from the restatement's f32 state, the target and the gradient from
    log_target_grad there.  Returns per draw a dict of numpy arrays: the outcome, the values and the state left."""
    pl, dev = plan_of(name), device_args(name)
    v0, u, ref = nf.restate(name)
    pl.attach_nuts_tree(nf.C, nf.MAX_DEPTH)
    got = []
    for k, o in enumerate(ref):
        th, tv, gr = _start(pl, dev, o["start_theta"])
        out = pl.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", index=dev["index"], v0=_t(v0[k]), u=_t(u[k]),
                           step_vec=dev["steps"], temp=dev["temp"], flags=flags)
        g = {key: out[key].cpu().numpy().astype(int) for key in OUTCOME}
        g.update(theta=_np(th), target=_np(tv), grad=_np(gr), accept_stat=_np(out["accept_stat"]), energy=_np(out["energy"]))
        got.append(g)
    return got


def errors(got, want):
    """Per quantity the largest error of one draw's values: absolute, or relative to the chain's largest entry."""
    errs = {}
    for key in VALUES:
        w, g = want[key], got[key]
        err = np.abs(g - w)
        if w.ndim == 2:
            err = err / np.abs(w).max(axis=1, keepdims=True)
        errs[key] = float(err.max())
    return errs


def _parity(name, flags):
    _, _, ref = nf.restate(name)
    got = draws_on_device(name, flags)
    worst = dict.fromkeys(VALUES, 0.0)
    for k, (o, g) in enumerate(zip(ref, got)):
        for key, e in errors(g, o).items():
            worst[key] = max(worst[key], e)
    print(f"{name} flags {flags}: largest errors " + ", ".join(f"{key} {worst[key]:.3g} (TAU {TAU[key]:.1g})" for key in VALUES))
    for k, (o, g) in enumerate(zip(ref, got)):
        for key in OUTCOME:
            assert np.array_equal(g[key], o[key].astype(int)), (name, flags, k, key, g[key], o[key], o["margin"])
        for key, e in errors(g, o).items():
            assert e <= TAU[key], (name, flags, k, key, e)
        stay = o["accepted"] == 0
        assert np.array_equal(g["theta"][stay], o["start_theta"][stay])   # a chain that does not move keeps its bits
    depth = np.stack([g["depth"] for g in got])
    assert set(depth.ravel().tolist()) == set(range(nf.MAX_DEPTH + 1))
    return got


# ------------------------------------------------------------------------------------------------ the kernel that serves
def test_nuts_kernel_names_the_fused_path():
    """Fails on the parent commit: there is no Plan.nuts_kernel."""
    from tests.test_nuts_gpu import _plan as generic_plan
    for name in nf.CASES:
        pl = plan_of(name)
        assert pl.nuts_kernel(FUSED) == "mfma32" and pl.nuts_kernel(FUSED | DEVICE) == "mfma32"
        assert pl.nuts_kernel() == "generic" and pl.nuts_kernel(DEVICE) == "generic"
        assert pl.nuts_kernel(FUSED | L.EY_FORCE_GENERIC) == "generic"
    xor = generic_plan("xor/diag", F32)
    assert xor.kernel == "generic" and xor.nuts_kernel(FUSED) == "generic" and xor.nuts_kernel() == "generic"
    th = torch.zeros(3, xor.P, dtype=F32, device=DEV)
    tv, gr = xor.log_target_grad(th)
    before = (th.clone(), tv.clone(), gr.clone())
    xor.attach_nuts_tree(3, 3)
    try:
        with pytest.raises(RuntimeError, match="status -2"):
            xor.nuts_step(th, tv, gr, 0.1, 3, torch.ones(xor.P, dtype=F32, device=DEV), "diag", seed=SEED, flags=FUSED)
        assert b"ey_plan_kernel" in L.lib().ey_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((th, tv, gr), before))
    finally:
        xor.detach_nuts_tree()


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(nf.CASES))
def test_parity_with_given_randoms(name):
    """The fused path against the restatement on every pair, the parent's path against the restatement the same way, and the
    two against each other."""
    fused = _parity(name, FUSED)
    parent = _parity(name, DEVICE)
    for k, (a, b) in enumerate(zip(fused, parent)):
        for key in OUTCOME:
            assert np.array_equal(a[key], b[key]), (name, k, key)
        for key, e in errors(a, b).items():
            assert e <= TAU[key], (name, k, key, e)


@pytest.mark.parametrize("name", ["n150", "n33/prior/temp", "n150/bce-tanh"])
def test_on_the_streams_both_paths_consume_the_same_variates(name):
    """v0 = u = NULL: the restatement on the Philox oracle's normals and block words.  The chains whose margin exceeds the
    floor must agree in outcome on both paths; at least a third of the 11 are decided (the unconditioned rate)."""
    from oracle import philox_oracle as po
    pl, dev, d = plan_of(name), device_args(name), nf.setup(name)
    pl.attach_nuts_tree(nf.C, nf.MAX_DEPTH)
    v0 = nf.f32(po.normal(nf.C, pl.P, SEED, IT0, dtype=np.float32))
    u = nf.f32(po.uniform_blocks(np.arange(nf.C), nf.S, SEED, IT0, dtype=np.float32))
    t, g = nf.evaluate(name, d["theta"])
    ref = nf.restate_draw(name, d["theta"], t, g, v0, u)
    live = ref["margin"] > nf.MARGIN_FLOOR
    for flags in (FUSED, DEVICE):
        th, tv, gr = _start(pl, dev, d["theta"])
        out = pl.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", index=dev["index"], step_vec=dev["steps"],
                           temp=dev["temp"], seed=SEED, it=IT0, flags=flags)
        for key in OUTCOME:
            got = out[key].cpu().numpy().astype(int)
            assert np.array_equal(got[live], ref[key][live].astype(int)), (name, flags, key, got, ref[key], ref["margin"])
        err = np.abs(_np(th) - ref["theta"]) / np.abs(ref["theta"]).max(axis=1, keepdims=True)
        assert (err[live] <= TAU["theta"]).all(), (name, flags, float(err[live].max()))
    print(f"{name} on the streams: {int(live.sum())} of {nf.C} chains decided")
    assert live.sum() >= (nf.C + 2) // 3


# ------------------------------------------------------------------------------------------------ run against steps
def _run_records(C, P, n):
    return dict(samples=torch.empty(n, C, P, dtype=F32, device=DEV), targets=torch.empty(n, C, dtype=F32, device=DEV),
                accepted_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV),
                accept_count=torch.zeros(C, dtype=torch.int32, device=DEV),
                depth_rec=torch.empty(n, C, dtype=torch.int32, device=DEV),
                divergent_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV))


def _bits_equal(xs, ys):
    for x, y in zip(xs, ys):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("name", ["n33/prior/temp", "n150/bce-tanh"])
def test_run_is_its_steps_bit_for_bit(name, C):
    chains = slice(1, 2) if C == 1 else slice(None)
    pl, dev = plan_of(name), device_args(name, chains)
    pl.attach_nuts_tree(C, nf.MAX_DEPTH)
    a = _start(pl, dev, nf.setup(name)["theta"][chains])
    b = tuple(t.clone() for t in a)
    rec = _run_records(C, pl.P, K_RUN)
    kw = dict(index=dev["index"], step_vec=dev["steps"], temp=dev["temp"], seed=SEED, flags=FUSED)
    oa = pl.nuts_run(*a, 0.0, nf.MAX_DEPTH, dev["M"], "diag", K_RUN, it=IT0, **kw, **rec)
    moved = 0
    for k in range(K_RUN):
        ob = pl.nuts_step(*b, 0.0, nf.MAX_DEPTH, dev["M"], "diag", it=IT0 + k, **kw)
        assert torch.equal(rec["samples"][k], b[0]) and torch.equal(rec["targets"][k], b[1]), k
        assert torch.equal(rec["accepted_rec"][k], ob["accepted"]) and torch.equal(rec["depth_rec"][k], ob["depth"]), k
        assert torch.equal(rec["divergent_rec"][k], ob["divergent"]), k
        moved += int(ob["accepted"].sum())
    _bits_equal(list(a) + [oa[key] for key in oa], list(b) + [ob[key] for key in oa])
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0)) and moved > 0
    assert torch.isfinite(rec["samples"]).all()


# ------------------------------------------------------------------------------------------------ the warm-up
def test_warmup_with_nothing_attached_is_the_run():
    name = "n33/index"
    pl, dev = plan_of(name), device_args(name)
    pl.attach_nuts_tree(nf.C, nf.MAX_DEPTH)
    a = _start(pl, dev, nf.setup(name)["theta"])
    b = tuple(t.clone() for t in a)
    ra, rb = _run_records(nf.C, pl.P, K_RUN), _run_records(nf.C, pl.P, K_RUN)
    kw = dict(index=dev["index"], step_vec=dev["steps"], seed=SEED, it=IT0, flags=FUSED)
    oa = pl.nuts_run(*a, 0.0, nf.MAX_DEPTH, dev["M"], "diag", K_RUN, **kw, **ra)
    ob = pl.nuts_warmup(*b, 0.0, nf.MAX_DEPTH, dev["M"], "diag", K_RUN, **kw, **rb)
    _bits_equal(list(a) + [ra[k] for k in ra] + [oa[k] for k in oa], list(b) + [rb[k] for k in ra] + [ob[k] for k in oa])
    assert int(ra["accepted_rec"].sum()) > 0


def test_warmup_epilogues_against_the_host():
    """tests/test_nuts_tree_gpu.py's test of the two epilogues and its bounds, on the fused path: the steps recorded are
    ey_da_update's recurrence replayed on the host from the recorded accept statistics (rtol 1e-6), the moments numpy's
    Welford of the recorded samples (1e-12 relative to the largest entry)."""
    from eeyore_amd.tuners import WindowedAdaptation
    from tests import hmc_warmup_restatement as R
    from tests import test_nuts_gpu as G
    from tests.hmc_metric_restatement import DIAG
    name = "n33"
    pl, dev = plan_of(name), device_args(name)
    C, P, K_WARM, D_TARGET = nf.C, pl.P, G.K_WARM, G.D_TARGET
    pl.attach_nuts_tree(C, nf.MAX_DEPTH)
    steps0 = dev["steps"][1].expand(C).contiguous().clone()   # every chain from a step that moves
    state = _start(pl, dev, nf.setup(name)["theta"])
    rec = _run_records(C, P, K_WARM)
    steps_rec, rate_rec = torch.empty(K_WARM, C, dtype=F32, device=DEV), torch.empty(K_WARM, C, dtype=F32, device=DEV)
    step_vec = steps0.clone()
    tuner = WindowedAdaptation(num_steps=1)
    da_state = tuner.restart(step_vec)
    mean, M2 = torch.zeros(C, P, dtype=F64, device=DEV), torch.zeros(C, P, dtype=F64, device=DEV)
    out = pl.nuts_warmup(*state, 0.0, nf.MAX_DEPTH, dev["M"], "diag", K_WARM, step_vec=step_vec, seed=SEED, it=IT0,
                         flags=FUSED, da_state=da_state, da_table=tuner.table(1, K_WARM, DEV), d=D_TARGET, final_avg=True,
                         mean=mean, M2=M2, count=0, steps_rec=steps_rec, rate_rec=rate_rec, **rec)
    assert torch.equal(steps_rec[0], steps0)
    assert torch.equal(rate_rec[-1].contiguous().view(torch.int32), out["accept_stat"].view(torch.int32))
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
    assert int(rec["accepted_rec"].sum()) > 0


# ------------------------------------------------------------------------------------------------ every wave slot and round
@pytest.mark.parametrize("name", ["n33/index", "n150/bce-tanh", "n33/exact"])
def test_every_wave_slot_and_chain_round(name):
    """The 11 chains tiled over C = 8 CUs + 11 with tiled v0 and u, as tests/test_persistent_slots.py does: every replica
    equals its original bit for bit, and replica 0 the same chains launched alone.  max_depth 3: a workspace near 200 MB."""
    from tests.test_persistent_slots import Replicas, slot
    pl, dev, d = plan_of(name), device_args(name), nf.setup(name)
    v0, u, _ = nf.restate(name)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    C = 8 * n_cu + nf.C
    assert slot(C - 1, n_cu, 8)[2] == 1   # a second round, ragged
    rep = Replicas(C, n_cu, 8)
    assert nf.C == 11 == int(rep.idx.max()) + 1
    pl.attach_nuts_tree(C, nf.MAX_DEPTH)

    def fn(th, v0, u, steps, temp, index):
        tv, gr = pl.log_target_grad(th, temp=temp)
        tv, gr = tv.contiguous(), gr.contiguous()
        out = pl.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", index=index, v0=v0, u=u, step_vec=steps, temp=temp,
                           flags=FUSED)
        return dict(theta=th, target=tv, grad=gr, **{k: out[k] for k in ("accepted", "depth", "n_leapfrog", "divergent",
                                                                          "accept_stat", "energy")})
    small = rep.both(f"nuts_step fused {name}", fn, _t(d["theta"]), _t(v0[0]), _t(u[0]), dev["steps"], dev["temp"], dev["index"])
    assert set(small["depth"].tolist()) >= {0, nf.MAX_DEPTH} and int(small["accepted"].sum()) > 0


# ------------------------------------------------------------------------------------------------ the workspace
def _four_draws(pl, dev, theta):
    st = _start(pl, dev, theta)
    rec = _run_records(nf.C, pl.P, 4)
    out = pl.nuts_run(*st, 0.0, nf.MAX_DEPTH, dev["M"], "diag", 4, index=dev["index"], step_vec=dev["steps"], temp=dev["temp"],
                      seed=SEED, it=IT0, flags=FUSED, **rec)
    torch.cuda.synchronize()
    return list(st) + [rec[k] for k in rec] + [out[k] for k in sorted(out)]


def test_results_do_not_depend_on_what_the_workspace_holds_or_on_its_size():
    name = "n33"
    pl, dev, theta = plan_of(name), device_args(name), nf.setup(name)["theta"]
    pl.detach_nuts_tree()
    ws = pl.attach_nuts_tree(nf.C, nf.MAX_DEPTH)
    assert ws.numel() == pl.nuts_tree_bytes(nf.C, nf.MAX_DEPTH) == nf.C * 18 * 1344 * 4
    ws.fill_(0xFF)   # every element a NaN
    assert torch.isnan(ws.view(F32)).all()
    nan_run = _four_draws(pl, dev, theta)
    ws.zero_()
    _bits_equal(nan_run, _four_draws(pl, dev, theta))
    big = pl.attach_nuts_tree(32, nf.MAX_DEPTH + 2)   # a larger workspace serves a smaller call
    assert big is not ws and big.numel() > ws.numel()
    big.fill_(0xFF)
    _bits_equal(nan_run, _four_draws(pl, dev, theta))
    assert int(nan_run[3 + 2].sum()) > 0   # (accepted_rec: the chains moved)
    pl.detach_nuts_tree()


# ------------------------------------------------------------------------------------------------ non-finite, refusals
def test_a_chain_that_starts_at_a_nan_state_stays_put():
    name = "n150"
    pl, dev, theta = plan_of(name), device_args(name), nf.setup(name)["theta"]
    pl.attach_nuts_tree(nf.C, nf.MAX_DEPTH)
    a = _start(pl, dev, theta)
    bad = theta.copy()
    bad[4] = np.nan
    b = _start(pl, dev, bad)
    assert torch.isnan(b[1][4])
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0, flags=FUSED)
    oa = pl.nuts_step(*a, 0.0, nf.MAX_DEPTH, dev["M"], "diag", **kw)
    ob = pl.nuts_step(*b, 0.0, nf.MAX_DEPTH, dev["M"], "diag", **kw)
    assert int(ob["depth"][4]) == 0 and int(ob["divergent"][4]) == 1 and int(ob["accepted"][4]) == 0
    assert int(ob["n_leapfrog"][4]) == 0 and torch.isnan(b[0][4]).all()
    others = torch.arange(nf.C, device=DEV) != 4
    for x, y in list(zip(a, b)) + [(oa[key], ob[key]) for key in oa]:
        assert torch.equal(x[others], y[others])
    assert int(oa["depth"][4]) > 0


def test_refusals_leave_everything_untouched():
    from eeyore_amd.plan import _stream
    lib = L.lib()
    name = "n33"
    pl, dev = plan_of(name), device_args(name)
    C = nf.C
    th, tv, gr = _start(pl, dev, nf.setup(name)["theta"])
    before = tuple(t.clone() for t in (th, tv, gr))
    acc = torch.full((C,), 7, dtype=torch.uint8, device=DEV)
    depth = torch.full((C,), -3, dtype=torch.int32, device=DEV)
    tril = torch.eye(4, dtype=F32, device=DEV)   # (refused before it is looked at)

    def raw_step(M, form, max_depth, flags, n=C):
        return lib.ey_nuts_step(pl.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(M), form, 1, None, None, None, 0, 0.05,
                                None, max_depth, None, n, SEED, 0, 0, flags, L.ptr(acc), L.ptr(depth), None, None, None, None,
                                _stream(pl.device))

    def untouched():
        torch.cuda.synchronize()
        return (all(torch.equal(x, y) for x, y in zip((th, tv, gr), before)) and bool((acc == 7).all())
                and bool((depth == -3).all()))

    out = dict(accepted=acc, depth=depth)
    kw = dict(step_vec=dev["steps"], seed=SEED, it=IT0, out=out)
    pl.detach_nuts_tree()
    # the bit with nothing attached: the existing check and message
    with pytest.raises(ValueError, match="ey_plan_attach_nuts_tree"):
        pl.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", flags=FUSED, **kw)
    assert raw_step(dev["M"], L.EY_METRIC_DIAG, nf.MAX_DEPTH, FUSED | DEVICE) == -1
    assert b"ey_plan_attach_nuts_tree" in lib.ey_last_error() and untouched()
    try:
        pl.attach_nuts_tree(C - 1, nf.MAX_DEPTH)
        have, need = pl.nuts_tree_bytes(C - 1, nf.MAX_DEPTH), pl.nuts_tree_bytes(C, nf.MAX_DEPTH)
        # an undersized workspace: one chain more, one doubling more
        with pytest.raises(ValueError, match=f"{have} bytes is smaller than the {need} bytes"):
            pl.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", flags=FUSED, **kw)
        assert raw_step(dev["M"], L.EY_METRIC_DIAG, nf.MAX_DEPTH + 1, FUSED, C - 1) == -1
        assert b"is smaller than" in lib.ey_last_error() and untouched()
        pl.detach_nuts_tree()
        pl.attach_nuts_tree(C, nf.MAX_DEPTH)
        # the bit with a dense metric, and with EY_FORCE_GENERIC
        assert raw_step(tril, L.EY_METRIC_TRIL, nf.MAX_DEPTH, FUSED) == -1
        assert b"diagonal metric only" in lib.ey_last_error() and untouched()
        with pytest.raises(ValueError, match="EY_FORCE_GENERIC"):
            pl.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", flags=FUSED | L.EY_FORCE_GENERIC, **kw)
        with pytest.raises(ValueError, match="EY_FORCE_GENERIC"):
            pl.nuts_run(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", 2, step_vec=dev["steps"], seed=SEED,
                        flags=FUSED | L.EY_FORCE_GENERIC, out=out)
        with pytest.raises(ValueError, match="EY_FORCE_GENERIC"):
            pl.nuts_warmup(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", 2, step_vec=dev["steps"], seed=SEED,
                           flags=FUSED | L.EY_FORCE_GENERIC, out=out)
        assert untouched()
        # a batch beyond the row limit of the family: the plan is no longer served, status -2 naming ey_plan_kernel
        from eeyore_amd.plan import Plan
        model = nf.model_of(name)
        wide = Plan(model["dims"], [1, 1, 1], model["acts"], model["lik"], F32, DEV)
        rows = 32 * 24 + 1
        wide.set_data(torch.zeros(rows, 4, dtype=F32, device=DEV), torch.eye(3, dtype=F32, device=DEV)[torch.zeros(rows, dtype=torch.long)])
        wide.set_prior(torch.zeros(wide.P), torch.ones(wide.P))
        assert wide.kernel != "mfma32" and wide.nuts_kernel(FUSED) == "generic"
        wide.attach_nuts_tree(C, nf.MAX_DEPTH)
        with pytest.raises(RuntimeError, match="status -2"):
            wide.nuts_step(th, tv, gr, 0.0, nf.MAX_DEPTH, dev["M"], "diag", flags=FUSED, **kw)
        assert b"ey_plan_kernel" in lib.ey_last_error() and untouched()
        # ... and what was attached is served
        o = pl.nuts_step(*(t.clone() for t in before), 0.0, nf.MAX_DEPTH, dev["M"], "diag", step_vec=dev["steps"], seed=SEED,
                         it=IT0, flags=FUSED)
        assert int(o["depth"].max()) == nf.MAX_DEPTH
    finally:
        pl.detach_nuts_tree()


# ------------------------------------------------------------------------------------------------ the sampler
def _iris_model():
    from torch.distributions import Normal
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                                activations=[torch.sigmoid, torch.sigmoid, None]),
                    dtype=F32, device=DEV)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEV), torch.ones(P, device=DEV))
    return model, P


def test_the_sampler_warms_up_and_samples_the_iris_network():
    """NUTS(tree='fused', tuner=WindowedAdaptation) on MLP(4-32-32-3) on Iris: 64 chains, a warm-up of 30 draws, 20 stored."""
    from torch.utils.data import DataLoader
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.samplers import NUTS, DiagMetric
    from eeyore_amd.tuners import WindowedAdaptation
    C, BURN, KEEP, DEPTH = 64, 30, 20, 5
    iris = XYDataset.from_eeyore('iris', yndmin=1, dtype=F32, yonehot=True, device=DEV)
    model, P = _iris_model()
    gen = torch.Generator().manual_seed(4)
    theta0 = (0.1 * torch.randn(C, P, generator=gen)).to(DEV)
    tuner = WindowedAdaptation(num_steps=1)
    s = NUTS(model, theta0=theta0, dataloader=DataLoader(iris, batch_size=len(iris), shuffle=False), tree='fused',
             metric='diag', max_depth=DEPTH, tuner=tuner, seed=2,
             chain=ChainBuffer(keys=['sample', 'target_val', 'accepted', 'depth', 'divergent']))
    s.run(num_epochs=BURN + KEEP, num_burnin_epochs=BURN)
    torch.cuda.synchronize()
    chain = s.get_chain()
    assert len(chain) == KEEP and tuple(chain.get_samples().shape) == (KEEP, C, P)
    assert tuple(s.step.shape) == (C,) and bool(torch.isfinite(s.step).all()) and bool((s.step > 0).all())
    depth = chain.bufs['depth'][:KEEP]
    assert tuple(depth.shape) == (KEEP, C) and int(depth.min()) >= 0 and int(depth.max()) <= DEPTH
    assert bool(torch.isfinite(chain.get_samples()).all()) and bool(torch.isfinite(chain.get_target_vals()).all())
    assert isinstance(s.metric, DiagMetric) and bool(torch.isfinite(s._metric).all())
    plan = model._plan(*next(iter(s.dataloader)))
    assert plan.kernel == "mfma32" and plan.nuts_kernel(s._flags(plan)) == "mfma32"
    assert plan._nuts_tree is not None and plan._nuts_tree.numel() >= plan.nuts_tree_bytes(C, DEPTH)


def test_sampler_on_the_streams_reproduces_nuts_run():
    """NUTS(tree='fused', rng='philox') on the headline model: 8 chains, 8 draws, 3 of them burn-in, against plan.nuts_run."""
    from torch.utils.data import DataLoader
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.samplers import NUTS
    n, burn, C, DEPTH, STEP = 8, 3, 8, 4, 0.02
    iris = XYDataset.from_eeyore('iris', yndmin=1, dtype=F32, yonehot=True, device=DEV)
    model, P = _iris_model()
    th0 = _t(0.3 * np.random.default_rng(2).standard_normal((C, P)))
    s = NUTS(model, theta0=th0, dataloader=DataLoader(iris, batch_size=len(iris), shuffle=False), tree='fused', step=STEP,
             max_depth=DEPTH, rng='philox', seed=SEED,
             chain=ChainBuffer(keys=['sample', 'target_val', 'accepted', 'depth', 'divergent']))
    assert s._can_fuse(False)
    s.run(num_epochs=n, num_burnin_epochs=burn)
    plan = s.model._plan(*next(iter(s.dataloader)))
    assert plan.nuts_kernel(FUSED) == "mfma32"
    th = th0.clone()
    tv, gr = plan.log_target_grad(th)
    rec = _run_records(C, P, n)
    out = plan.nuts_run(th, tv.contiguous(), gr.contiguous(), STEP, DEPTH, torch.ones(P, dtype=F32, device=DEV), "diag", n,
                        seed=SEED, it=0, flags=FUSED, **rec)
    ch = s.get_chain()
    assert len(ch) == n - burn
    assert torch.equal(ch.get_samples(), rec["samples"][burn:]) and torch.equal(ch.get_target_vals(), rec["targets"][burn:])
    assert torch.equal(ch.get_accepted(), rec["accepted_rec"][burn:])
    assert torch.equal(ch.bufs['depth'][:len(ch)], rec["depth_rec"][burn:])
    assert torch.equal(s._theta, th) and torch.equal(s.last['depth'], out['depth']) and int(rec["accepted_rec"].sum()) > 0


def test_iris_nuts_example_runs_fused():
    """examples/iris_nuts.py --tree fused at reduced size, through the environment tests/test_examples.py uses."""
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="20", EEYORE_EXAMPLE_CHAINS="64", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "iris_nuts.py"), "--tree", "fused"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "tree='fused': NUTS runs on the mfma32 kernel" in out.stdout
    assert "64 chains, 1315 parameters" in out.stdout and "tree depths of the stored draws" in out.stdout
