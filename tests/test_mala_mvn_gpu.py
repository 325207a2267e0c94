"""MALA with a MultivariateNormalKernel proposal on the device (ey_mala_tril_step / ey_mala_tril_run, k_mala_tril in
eeyore_amd/csrc/ey_generic.hip) against the numpy restatement (tests/mala_mvn_restatement.py), the reference's own traces
(g17_mala_mvn_traces.npz), ey_mala_step, and itself.  Plans, sizes and factor forms are those of tests/test_mh_mvn_gpu.py.

Tolerances are the generic family's: log-rate 1e-9 in f64, rtol 2e-4 / atol 2e-3 in f32; state and gradient 1e-12 / 1e-5;
decision margin F32_DECISION_TOL."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mlp_oracle as orc
from tests import dist_restatement as dr
from tests import test_mh_mvn_gpu as MH
from tests.mala_mvn_restatement import group_value_grad, mala_mvn_draw
from tests.test_dist_gpu import _loader, _mixture, _model
from tests.test_mala_mvn_host import _groups
from tests.test_mh_mvn_gpu import CS, FORMS, MIX, PLANS, _factor_of, _num_params, _plan, _round32
from tests.test_ram_gpu import CASES, F32_DECISION_TOL, _data, _t
from tests.test_ram_gpu import _plan as _mlp_plan

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
STEP_VEC_PLAN, TEMP_PLAN = "mix63_2", "mlp433"  # the case with per-chain steps; the one with a temperature vector (MH's)
# (plan, C) -> seed of _inputs for which the restatement alone (f64, and on the inputs rounded to f32) leaves no chain
# inside ten times the decision margin in any of the three factor forms (searched on the CPU with _undecided below; seeds
# not listed are 0)
SEEDS = {('mix2_2', 3): 1, ('mix63_2', 11): 1, ('mix64_1', 1): 1, ('mix64_1', 11): 2, ('mix65_2', 11): 2, ('mlp433', 11): 1}


def _step(name):
    """The scalar step of a plan's cases: small where the factors are small (P > 60, MH's scale 0.05) and smaller for the
    MLP plans' steeper targets, so that the drift step/2 grad stays of the order of the noise L z and the cases mix accepts
    and rejects."""
    return (0.02 if name in MIX else 0.002) if _num_params(name) > 60 else (0.5 if name in MIX else 0.05)


def _inputs(name, C, form, seed):
    """MH's inputs of the case (start, z, u, temperatures, factors [G, P, P], index) and the steps (numpy f64)."""
    d = MH._inputs(name, C, form, seed)
    d["step"] = _step(name)
    d["step_vec"] = None
    if name == STEP_VEC_PLAN:
        d["step_vec"] = d["step"] * (0.5 + np.random.default_rng(1000 * seed + C + 77).random(C))
    return d


def _cpu_value_grad(name, f32, temp):
    """(log-target, gradient) of a plan in numpy f64, on the tables rounded to f32 for an f32 plan."""
    if name in MIX:
        (c, mean, prec), _ = _mixture(*MIX[name])
        tab = tuple(_round32(a) for a in (c, mean, prec)) if f32 else (c, mean, prec)
        return dr.mix_value_grad_fn(*tab, temperature=temp)
    dims, acts, lik, N = CASES[name]
    x, y = _data(dims, lik, N)
    spec = orc.Spec(dims, acts, lik, temperature=temp)

    def fn(th):
        t, g = orc.upto_grad_log_target(spec, np.asarray(th, np.float64), x, y)
        return float(t), g
    return fn


def _chain_step(d, ch):
    return float(d["step"] if d["step_vec"] is None else d["step_vec"][ch])


def _undecided(name, C, seed, f32, slack=1.0):
    """How many chains of a case the restatement alone leaves inside ``slack`` times the decision margin, at worst over
    the three factor forms (CPU only)."""
    worst = 0
    for form in FORMS:
        d = _inputs(name, C, form, seed)
        if f32:
            d = {k: (v if k in ("idx", "step") else _round32(v)) for k, v in d.items()}
        n = 0
        for ch in range(C):
            vg = _cpu_value_grad(name, f32, None if d["temp"] is None else float(d["temp"][ch]))
            t0, g0 = vg(d["th"][ch])
            lr = mala_mvn_draw(vg, d["th"][ch], t0, g0, _factor_of(d, form, ch), d["z"][ch], d["u"][ch],
                               _chain_step(d, ch))[4]
            tol = F32_DECISION_TOL * max(1.0, abs(lr)) if f32 else 1e-9
            n += not abs(np.log(d["u"][ch]) - lr) > slack * tol
        worst = max(worst, n)
    return worst


def _device_inputs(name, C, form, dtype, seed=None):
    d = _inputs(name, C, form, SEEDS.get((name, C), 0) if seed is None else seed)
    dev = {k: None if v is None else _t(v, dtype) for k, v in d.items() if k not in ("idx", "step")}
    dev["idx"] = None if d["idx"] is None else torch.tensor(d["idx"], dtype=torch.int32, device=DEV)
    dev["step"] = d["step"]
    if form == "shared":
        dev["L"] = dev["L"][0].contiguous()
    return d, dev


def _start(pl, dev):
    th = dev["th"].clone()
    tv, gr = pl.log_target_grad(th, temp=dev["temp"])
    return th, tv.contiguous(), gr.contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", PLANS)
def test_one_step_against_the_restatement(name, dtype, C, form):
    """The f32 P = 128 cases sum two quadratic forms of size about P that nearly cancel; they keep the generic f32 log-rate
    bound all the same: measured on an MI355X, the largest f32 log-rate error of any case is 6.9e-5 (mix128_16), 3 % of
    the bound, and the largest gradient error 1.0e-5 beside an entry of 40 (mlp483)."""
    pl = _plan(name, dtype)
    f64 = dtype == F64
    d, dev = _device_inputs(name, C, form, dtype)
    # the restatement starts from the values the device holds (f32: rounded)
    th0, z, u, Ls = (_np(dev[k]) for k in ("th", "z", "u", "L"))
    Ls = Ls[None] if form == "shared" else Ls
    temps = None if dev["temp"] is None else _np(dev["temp"])
    steps = None if dev["step_vec"] is None else _np(dev["step_vec"])
    th, tv, gr = _start(pl, dev)
    tv0, gr0 = _np(tv), _np(gr)
    out = pl.mala_tril_step(th, tv, gr, dev["step"], dev["L"], index=dev["idx"], z=dev["z"], u=dev["u"],
                            step_vec=dev["step_vec"], temp=dev["temp"])
    acc = out["accepted"].cpu().numpy()
    lr_dev = _np(out["log_rate"])
    th1, tv1, gr1 = _np(th), _np(tv), _np(gr)
    decided = 0
    for c in range(C):
        vg = _cpu_value_grad(name, not f64, None if temps is None else float(temps[c]))
        Lc = Ls[0 if form == "shared" else c if form == "per_chain" else d["idx"][c]]
        # the restatement from the device's own starting target and gradient (f32: their rounding is not what is tested)
        w_th, w_tv, w_gr, w_acc, lr_ref = mala_mvn_draw(vg, th0[c], float(tv0[c]), gr0[c], Lc, z[c], u[c],
                                                        d["step"] if steps is None else float(steps[c]))
        margin = abs(np.log(u[c]) - lr_ref)
        tol = 1e-9 if f64 else F32_DECISION_TOL * max(1.0, abs(lr_ref))
        print(f"{name} {form} C={C} chain {c}: log_rate {lr_dev[c]!r} restatement {lr_ref!r} margin {margin:.3e} "
              f"accepted {acc[c]}")
        np.testing.assert_allclose(lr_dev[c], lr_ref, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
        if margin > tol:
            decided += 1
            assert bool(acc[c]) == w_acc, (c, lr_ref, np.log(u[c]))
        st = dict(rtol=1e-12 if f64 else 1e-5, atol=1e-12 if f64 else 1e-5)
        if acc[c]:
            print(f"  state error {np.abs(th1[c] - w_th).max():.3e} gradient error {np.abs(gr1[c] - w_gr).max():.3e} "
                  f"(largest gradient entry {np.abs(w_gr).max():.3e})")
            np.testing.assert_allclose(th1[c], w_th, **st)
            np.testing.assert_allclose(gr1[c], w_gr, **st)
        else:
            assert np.array_equal(th1[c], th0[c]) and np.array_equal(gr1[c], gr0[c]) and tv1[c] == tv0[c]
    assert decided >= max(1, C - 3)


# ------------------------------------------------------------------------------------------------ the upper triangle
@pytest.mark.parametrize("name,dtype", [("mix65_2", F64), ("mlp433", F32), ("mix128_16", F32)])
def test_the_upper_triangle_is_never_read(name, dtype):
    pl = _plan(name, dtype)
    C, P = 3, _num_params(name)
    _, dev = _device_inputs(name, C, "per_chain", dtype)
    dirty = dev["L"].clone()
    dirty[torch.triu(torch.ones(P, P, dtype=torch.bool, device=DEV), 1).expand(C, P, P)] = float("nan")
    res = []
    for L_ in (dev["L"], dirty):
        th, tv, gr = _start(pl, dev)
        out = pl.mala_tril_step(th, tv, gr, dev["step"], L_, z=dev["z"], u=dev["u"], temp=dev["temp"])
        res.append((th, tv, gr, out["accepted"], out["log_rate"]))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t).all() for t in (res[1][0], res[1][2], res[1][4]))


# ------------------------------------------------------------------------------------------------ L = sqrt(step) I
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["mix65_2", "mlp483"])
def test_scaled_identity_factor_against_mala_step(name, dtype):
    """L = sqrt(step) I proposes what ey_mala_step proposes, bit for bit (the same Philox normals, one multiply-add per
    row onto the same mean), so accepted states are identical; the log-rates differ by the order of the sums only."""
    from eeyore_amd import _lib as L
    pl = _plan(name, dtype)
    pl.row_waves = "off"
    f64 = dtype == F64
    C, P, step = 11, _num_params(name), 0.4 if name in MIX else 0.02  # steps at which about half the proposals are accepted
    _, dev = _device_inputs(name, C, "shared", dtype)
    sc = torch.tensor(np.sqrt(step), dtype=dtype)  # np.sqrt on the python float, then cast: as ey_mala_step (mala.py:39)
    tril = (torch.eye(P, dtype=dtype) * sc).to(DEV).contiguous()
    accepts = compared = 0
    for it in range(4):
        th_a, tv_a, gr_a = _start(pl, dict(dev, temp=None))
        th_b, tv_b, gr_b = th_a.clone(), tv_a.clone(), gr_a.clone()
        a = pl.mala_tril_step(th_a, tv_a, gr_a, step, tril, seed=7, it=it)
        b = pl.mala_step(th_b, tv_b, gr_b, step, seed=7, it=it, flags=L.EY_FORCE_GENERIC)
        lr_a, lr_b = _np(a["log_rate"]), _np(b["log_rate"])
        np.testing.assert_allclose(lr_a, lr_b, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
        # u is the kernels' own (the same Philox stream): two decisions can differ only if log u lies between the two
        # log-rates, and the chain is then inside the margin exactly if those are within tol of each other
        acc_a, acc_b = a["accepted"].cpu().numpy().astype(bool), b["accepted"].cpu().numpy().astype(bool)
        for c in range(C):
            tol = 1e-9 if f64 else F32_DECISION_TOL * max(1.0, abs(lr_b[c]))
            if acc_a[c] != acc_b[c]:
                assert abs(lr_a[c] - lr_b[c]) <= tol, (it, c, lr_a[c], lr_b[c])
                continue
            compared += 1
            if acc_a[c]:  # identical proposals
                accepts += 1
                assert torch.equal(th_a[c], th_b[c]), (it, c)
                assert torch.equal(tv_a[c], tv_b[c]) and torch.equal(gr_a[c], gr_b[c]), (it, c)
            else:
                assert torch.equal(th_a[c], dev["th"][c])
    print(f"{name}: {accepts} of {compared} compared proposals accepted")
    assert compared >= 4 * C - 3 and accepts > 0


# ------------------------------------------------------------------------------------------------ run = steps
@pytest.mark.parametrize("form", ["shared", "indexed"])
@pytest.mark.parametrize("name,dtype", [("mix2_2", F64), ("mix128_16", F32)])
def test_run_equals_steps_bit_for_bit(name, dtype, form):
    pl = _plan(name, dtype)
    C, K, P = 11, 7, _num_params(name)
    _, dev = _device_inputs(name, C, form, dtype)
    th_a, tv_a, gr_a = _start(pl, dev)
    th_b, tv_b, gr_b = th_a.clone(), tv_a.clone(), gr_a.clone()
    rs = torch.empty(K, C, P, dtype=dtype, device=DEV)
    rt = torch.empty(K, C, dtype=dtype, device=DEV)
    ra = torch.empty(K, C, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(C, dtype=torch.int32, device=DEV)
    out = pl.mala_tril_run(th_a, tv_a, gr_a, dev["step"], dev["L"], K, index=dev["idx"], seed=9, it=11, samples=rs,
                           targets=rt, accepted_rec=ra, accept_count=cnt)
    for k in range(K):
        step = pl.mala_tril_step(th_b, tv_b, gr_b, dev["step"], dev["L"], index=dev["idx"], seed=9, it=11 + k)
        assert torch.equal(rs[k], th_b) and torch.equal(rt[k], tv_b) and torch.equal(ra[k], step["accepted"]), k
    assert torch.equal(th_a, th_b) and torch.equal(tv_a, tv_b) and torch.equal(gr_a, gr_b)
    assert torch.equal(out["accepted"], step["accepted"])
    assert torch.equal(cnt, ra.int().sum(0))
    assert 0 < int(cnt.sum()) < C * K


# ------------------------------------------------------------------------------------------------ chain independence
@pytest.mark.parametrize("name,dtype", [("mix65_2", F32), ("mlp433", F64)])
def test_a_chains_bits_do_not_depend_on_its_neighbours(name, dtype):
    pl = _plan(name, dtype)
    C = 11
    _, dev = _device_inputs(name, C, "per_chain", dtype)
    th, tv, gr = _start(pl, dev)
    tv0, gr0 = tv.clone(), gr.clone()
    pl.mala_tril_run(th, tv, gr, dev["step"], dev["L"], 5, temp=dev["temp"], seed=5)
    for c in range(C):
        th1, tv1, gr1 = dev["th"][c:c + 1].clone(), tv0[c:c + 1].clone(), gr0[c:c + 1].clone()
        tp = None if dev["temp"] is None else dev["temp"][c:c + 1].contiguous()
        pl.mala_tril_run(th1, tv1, gr1, dev["step"], dev["L"][c:c + 1].contiguous(), 5, temp=tp, seed=5, chain_offset=c)
        assert torch.equal(th1[0], th[c]) and torch.equal(tv1[0], tv[c]) and torch.equal(gr1[0], gr[c]), c
    assert not torch.equal(th, dev["th"])


# ------------------------------------------------------------------------------------------------ the reference's traces
@pytest.mark.parametrize("name", list("abcd"))
def test_fixture_replay(name):
    from eeyore_amd.plan import Plan
    rec = _groups()[name]
    if "weights" in rec:
        pl = Plan.mixture(*dr.tables(rec["weights"], rec["means"], rec["covs"], bool(rec["normalized"])), F64, DEV)
    else:
        pl = _mlp_plan(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], F64)
    th = _t(rec["theta0"], F64)[None].clone()
    tv = _t([rec["init_target"]], F64)
    gr = _t(rec["init_grad"], F64)[None].clone()
    L_ = _t(rec["L"], F64)
    in_margin = 0
    for it in range(rec["z"].shape[0]):
        out = pl.mala_tril_step(th, tv, gr, float(rec["step"]), L_, z=_t(rec["z"][it], F64)[None],
                                u=_t([rec["u"][it]], F64))
        if abs(np.log(float(rec["u"][it])) - out["log_rate"].item()) <= 1e-9:
            in_margin += 1
        assert int(out["accepted"].item()) == int(rec["accepted"][it]), it
        np.testing.assert_allclose(th[0].cpu().numpy(), rec["sample"][it], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(tv.item(), rec["target_val"][it], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(gr[0].cpu().numpy(), rec["grad_val"][it], rtol=1e-9, atol=1e-9)
    assert in_margin == 0
    assert group_value_grad(rec) is not None


# ------------------------------------------------------------------------------------------------ refusals
def _raw_step(pl, th, tv, gr, tril, G, idx, acc, C, step=0.1):
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import _stream
    return L.lib().ey_mala_tril_step(pl.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(tril), G, L.ptr(idx), None, None,
                                     step, None, None, C, 0, 0, 0, 0, L.ptr(acc), None, _stream(pl.device))


def _raw_run(pl, th, tv, gr, tril, G, idx, acc, C, n_iters, step=0.1):
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import _stream
    return L.lib().ey_mala_tril_run(pl.handle, L.ptr(th), L.ptr(tv), L.ptr(gr), L.ptr(tril), G, L.ptr(idx), step, None,
                                    None, C, 0, 0, 0, 0, n_iters, None, None, None, None, L.ptr(acc), _stream(pl.device))


def test_refusals_write_nothing():
    from eeyore_amd import _lib as L
    C = 3

    def state(pl, dtype, G=1):
        th = torch.full((C, pl.P), 0.25, dtype=dtype, device=DEV)
        tv = torch.full((C,), -7.0, dtype=dtype, device=DEV)
        gr = torch.full((C, pl.P), 0.5, dtype=dtype, device=DEV)
        acc = torch.full((C,), 9, dtype=torch.uint8, device=DEV)
        tril = torch.eye(pl.P, dtype=dtype, device=DEV).expand(G, pl.P, pl.P).contiguous()
        return th, tv, gr, acc, tril

    def untouched(th, tv, gr, acc):
        torch.cuda.synchronize()
        return bool((th == 0.25).all() and (tv == -7.0).all() and (gr == 0.5).all() and (acc == 9).all())

    # P > 128: MLP(4-32-32-3), and the plan whose evaluation image leaves the factor no room (as MH's test: LR on 127
    # inputs in f64, P = 128)
    for dims, acts, lik, dtype in (([4, 32, 32, 3], [1, 1, 0], 1, F32), ([127, 1], [1], 0, F64)):
        x, y = _data(dims, lik, 64)
        pl = _mlp_plan(dims, acts, lik, x, y, dtype)
        th, tv, gr, acc, tril = state(pl, dtype)
        assert _raw_step(pl, th, tv, gr, tril, 1, None, acc, C) == -2, dims
        assert b"MALA with a factor" in L.lib().ey_last_error()
        assert _raw_run(pl, th, tv, gr, tril, 1, None, acc, C, 4) == -2, dims
        assert untouched(th, tv, gr, acc), dims
        with pytest.raises(RuntimeError, match="status -2"):
            pl.mala_tril_step(th, tv, gr, 0.1, tril, out=dict(accepted=acc, log_rate=None))
        assert untouched(th, tv, gr, acc), dims
    pl = _plan("mix2_2", F64)
    th, tv, gr, acc, tril = state(pl, F64, G=2)
    assert _raw_step(pl, th, tv, gr, tril, 2, None, acc, C) == -1  # G = 2 without an index at C = 3
    assert b"tril_index" in L.lib().ey_last_error()
    assert _raw_run(pl, th, tv, gr, tril, 2, None, acc, C, 4) == -1
    assert _raw_step(pl, th, tv, gr, tril, 0, None, acc, C) == -1  # G < 1
    assert _raw_run(pl, th, tv, gr, tril, 1, None, acc, C, 0) == -1  # n_iters = 0
    assert b"n_iters" in L.lib().ey_last_error()
    assert _raw_step(pl, th, tv, gr, None, 1, None, acc, C) == -1  # a null tril
    assert b"null argument" in L.lib().ey_last_error()
    assert _raw_run(pl, th, tv, gr, None, 1, None, acc, C, 4) == -1
    assert _raw_step(pl, th, tv, None, tril, 1, None, acc, C) == -1  # a null grad
    assert b"null argument" in L.lib().ey_last_error()
    assert _raw_run(pl, th, tv, None, tril, 1, None, acc, C, 4) == -1
    assert _raw_step(pl, th, tv, gr, tril, 1, None, acc, C, step=0.0) == -1  # no step
    assert b"step must be positive" in L.lib().ey_last_error()
    assert untouched(th, tv, gr, acc)
    # the Python layer: the number of factors, the index's dtype and its range
    with pytest.raises(ValueError, match="without index"):
        pl.mala_tril_step(th, tv, gr, 0.1, tril)
    with pytest.raises(ValueError, match="int32"):
        pl.mala_tril_step(th, tv, gr, 0.1, tril, index=torch.zeros(C, dtype=torch.int64, device=DEV))
    for bad in ([0, 1, 2], [0, -1, 1]):
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            pl.mala_tril_step(th, tv, gr, 0.1, tril, index=torch.tensor(bad, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="tril must be"):
        pl.mala_tril_step(th, tv, gr, 0.1, tril.float())
    with pytest.raises(ValueError, match="n_iters"):
        pl.mala_tril_run(th, tv, gr, 0.1, tril[0].contiguous(), 0)
    assert untouched(th, tv, gr, acc)
    # C = 0 is nothing to do
    e = torch.empty(0, pl.P, dtype=F64, device=DEV)
    assert _raw_step(pl, e, e, e, tril, 2, None, acc, 0) == 0


# ------------------------------------------------------------------------------------------------ attached moments
def test_attached_moments_equal_the_moments_of_the_records():
    pl = _plan("mix2_2", F64)
    C, K, P = 11, 6, 2
    _, dev = _device_inputs("mix2_2", C, "indexed", F64)
    th, tv, gr = _start(pl, dev)
    s1, s2 = (torch.zeros(C, P, dtype=F64, device=DEV) for _ in range(2))
    acc = torch.zeros(C, dtype=F64, device=DEV)
    rs = torch.empty(K, C, P, dtype=F64, device=DEV)
    ra = torch.empty(K, C, dtype=torch.uint8, device=DEV)
    pl.attach_moments(s1, s2, acc)
    try:
        pl.mala_tril_run(th, tv, gr, dev["step"], dev["L"], K, index=dev["idx"], seed=2, samples=rs, accepted_rec=ra)
        # attached moments over several iterations need the records: refused before the launch, the chains left alone
        before = th.clone()
        with pytest.raises(RuntimeError, match="status -2"):
            pl.mala_tril_run(th, tv, gr, dev["step"], dev["L"], K, index=dev["idx"], seed=2, it=K)
        assert torch.equal(th, before)
    finally:
        pl.detach_moments()
    w1, w2 = torch.zeros_like(s1), torch.zeros_like(s2)
    for k in range(K):
        w1 += rs[k]
        w2 += rs[k] * rs[k]
    assert torch.equal(acc, ra.double().sum(0))
    # K terms per sum, in whatever order: the bounds of tests/test_mh_mvn_gpu.py's test of the same name
    bound = float(rs.abs().sum(0).max())
    np.testing.assert_allclose(s1.cpu().numpy(), w1.cpu().numpy(), rtol=0, atol=K * 2.0 ** -53 * bound)
    np.testing.assert_allclose(s2.cpu().numpy(), w2.cpu().numpy(), rtol=2 * K * 2.0 ** -52, atol=0)
    assert 0 < ra.sum() < K * C


# ------------------------------------------------------------------------------------------------ the sampler surface
def _tril3(seed, scale=0.8):
    return MH._tril3(seed, scale)


def _mala(per_chain, fused_block, epochs=40, C=8):
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.kernels import MultivariateNormalKernel
    from eeyore_amd.samplers import MALA
    m, tgt = _model("b", F64)
    th0 = (torch.tensor(tgt["means"][1], dtype=F64)[None].repeat(C, 1) + 0.1).to(DEV)
    L_ = torch.stack([_tril3(c) for c in range(C)]) if per_chain else _tril3(0)
    s = MALA(m, theta0=th0, dataloader=_loader(), step=0.4, seed=6, chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']),
             kernel=MultivariateNormalKernel(torch.zeros(3, dtype=F64), L_))
    s.fused_block = fused_block
    s.run(num_epochs=epochs, num_burnin_epochs=10)
    return s


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "per_chain"])
def test_sampler_run_in_blocks_equals_draws(per_chain):
    from eeyore_amd.kernels import MultivariateNormalKernel
    from eeyore_amd.samplers import MALA
    a, b, c = _mala(per_chain, 256), _mala(per_chain, 0), _mala(per_chain, 16)
    assert a._can_fuse(False) and not b._can_fuse(False)
    ca = a.get_chain()
    for other in (b, c):
        co = other.get_chain()
        assert torch.equal(ca.get_samples(), co.get_samples()) and torch.equal(ca.get_target_vals(), co.get_target_vals())
        assert torch.equal(ca.get_accepted(), co.get_accepted()) and torch.equal(a._theta, other._theta)
        assert torch.equal(a._grad, other._grad)
    smp, acc = ca.get_samples(), ca.get_accepted().bool()
    assert smp.shape == (30, 8, 3) and torch.isfinite(smp).all()
    moved = (smp[1:] != smp[:-1]).any(-1)
    assert torch.equal(moved, acc[1:]) and 0 < int(acc.sum()) < acc.numel()
    # MALA.kernel: the MultivariateNormalKernel centred at kernel_mean(current)
    k = a.kernel
    assert isinstance(k, MultivariateNormalKernel)
    assert tuple(k.scale_tril.shape) == ((8, 3, 3) if per_chain else (3, 3))
    assert torch.equal(k.density.loc, a._theta + 0.5 * 0.4 * a._grad)
    if per_chain:  # the chains really propose with different factors
        shared = _mala(False, 256).get_chain().get_samples()
        assert torch.equal(shared[:, 0], smp[:, 0]) and not torch.equal(shared[:, 1], smp[:, 1])
    m, _ = _model("b", F64)
    with pytest.raises(ValueError, match="one per chain"):
        MALA(m, theta0=torch.zeros(8, 3, dtype=F64, device=DEV), dataloader=_loader(),
             kernel=MultivariateNormalKernel(torch.zeros(3, dtype=F64), torch.stack([_tril3(0), _tril3(1)])))


K_PT, R_PT = 3, 2


def _pps(between, between_step, epochs, kernels=None, start=1):
    from eeyore_amd.kernels import MultivariateNormalKernel
    from eeyore_amd.samplers import PowerPosteriorSampler
    m, tgt = _model("b", F64)
    th0 = (torch.tensor(tgt["means"][1], dtype=F64)[None].repeat(R_PT, 1) + 0.1).to(DEV)
    if kernels is None:
        kernels = [MultivariateNormalKernel(torch.zeros(3, dtype=F64), _tril3(10 + k, 0.5 + 0.4 * k)) for k in range(K_PT)]
    s = PowerPosteriorSampler(m, _loader(), [['MALA', dict(step=0.4) if k is None else dict(step=0.4, kernel=k)]
                                             for k in kernels],
                              theta0=th0, between_step=between_step, rng='philox', seed=3, between=between,
                              keys=['sample', 'target_val', 'accepted'])
    # draw 0 is a between-draw whatever between_step is (0 % between_step == 0): a run without a move starts at draw 1
    s.counter.idx = start
    s.run(num_epochs=epochs, num_burnin_epochs=0)
    return s, th0


@pytest.mark.parametrize("between", ["host", "device"])
def test_power_posterior_proposes_with_one_factor_per_temperature(between):
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.kernels import MultivariateNormalKernel
    from eeyore_amd.samplers import MALA
    torch.manual_seed(0)
    s, th0 = _pps(between, 1000, 25)
    n = len(s.get_chain(0))
    assert n >= 24 and tuple(s.sampler._tril.shape) == (K_PT, 3, 3)  # K factors on the device, not K x R
    assert s.sampler._tril_index.tolist() == [0, 0, 1, 1, 2, 2]
    assert tuple(s.sampler.kernel.scale_tril.shape) == (K_PT * R_PT, 3, 3)
    m, _ = _model("b", F64)
    tvec = torch.tensor(s.temperature, dtype=F64, device=DEV).repeat_interleave(R_PT)
    trils = torch.stack([_tril3(10 + k, 0.5 + 0.4 * k) for k in range(K_PT)]).repeat_interleave(R_PT, 0)
    ref = MALA(m, theta0=th0.repeat(K_PT, 1).contiguous(), dataloader=_loader(), temperature=tvec, seed=3, step=0.4,
               chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']),
               kernel=MultivariateNormalKernel(torch.zeros(3, dtype=F64), trils))
    ref.run(num_epochs=n, num_burnin_epochs=0)
    assert torch.equal(s.sampler._theta, ref._theta) and torch.equal(s.sampler._target, ref._target)
    rc = ref.get_chain()
    for k in range(K_PT):
        ch = s.get_chain(k)
        sl = slice(k * R_PT, (k + 1) * R_PT)
        assert torch.equal(ch.get_samples(), rc.get_samples()[:, sl]), k
        assert torch.equal(ch.get_target_vals(), rc.get_target_vals()[:, sl]), k
        assert torch.equal(ch.get_accepted(), rc.get_accepted()[:, sl]), k
    acc = rc.get_accepted()
    assert 0 < int(acc.sum()) < acc.numel()


def test_power_posterior_with_between_moves_on_the_device():
    from eeyore_amd.kernels import MultivariateNormalKernel
    s, _ = _pps("device", 2, 30, start=0)
    for k in range(K_PT):
        ch = s.get_chain(k)
        assert ch.get_samples().shape == (30, R_PT, 3)
        assert torch.isfinite(ch.get_samples()).all() and torch.isfinite(ch.get_target_vals()).all()
    # a temperature without a kernel proposes with the identity
    mvn = MultivariateNormalKernel(torch.zeros(3, dtype=F64), _tril3(1))
    s, _ = _pps("device", 2, 6, kernels=[mvn, None, mvn], start=0)
    assert torch.equal(s.sampler._tril[1], torch.eye(3, dtype=F64, device=DEV))


def test_power_posterior_refuses_mixed_kernel_kinds():
    from eeyore_amd.kernels import MultivariateNormalKernel, NormalKernel
    mvn = MultivariateNormalKernel(torch.zeros(3, dtype=F64), _tril3(1))
    nk = NormalKernel(torch.zeros(3, dtype=F64), torch.ones(3, dtype=F64))
    with pytest.raises(ValueError, match="all NormalKernels or all MultivariateNormalKernels"):
        _pps("host", 5, 4, kernels=[mvn, nk, mvn])
    per_chain = MultivariateNormalKernel(torch.zeros(3, dtype=F64), torch.stack([_tril3(1), _tril3(2)]))
    with pytest.raises(ValueError, match=r"\[3, 3\] scale_tril"):
        _pps("host", 5, 4, kernels=[mvn, per_chain, mvn])


# ------------------------------------------------------------------------------------------------ the example
def test_example_runs():
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="33", EEYORE_EXAMPLE_CHAINS="96", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bivariate_normal_mixture_mala_mvn.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "cceptance rate" in out.stdout and "MMD" in out.stdout
