"""Elliptical slice sampling on the device (ey_eslice_ell / ey_eslice_step / ey_eslice_run, k_eslice in
eeyore_amd/csrc/ey_eslice.hip) against the numpy restatement (tests/eslice_restatement.py) on the cases of
tests/eslice_cases.py, and against itself.

A draw is a chain of discontinuous decisions, so the comparison follows the restatement's margins, as
tests/test_nuts_gpu.py's does and for the same reason: a draw whose smallest margin is above 1e-9 must agree exactly in
accepted and n_evals and to 1e-10 relative (against the largest entry of the vector compared) in theta, target and ell; a
chain is followed only up to its first draw under the margin, and at most 5 % of the (chain, draw) pairs may be lost that
way (tests/test_eslice_host.py holds the committed inputs to that with the restatement alone)."""
import functools

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from oracle import philox_oracle as po
from tests import eslice_cases as ec
from tests import eslice_restatement as er
from tests import invariance as iv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
RTOL = 1e-10
SEED, IT0, K_RUN = 37, 5, 6


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _plan(name, dtype):
    from eeyore_amd.plan import Plan
    from tests.test_invariance_gpu import _plan as iv_plan
    case, d = ec.CASES[name], ec.inputs(name)
    key = "f64" if dtype == F64 else "f32"
    if case["kind"] == "lin":
        return iv_plan(ec.LIN, key)
    if case["kind"] == "mix":
        return iv_plan(case["target"], key)
    if case["kind"] == "mvn":
        tgt = ec.mvn(case["P"])
        return Plan.mixture(tgt.c, tgt.mean, tgt.prec, dtype, DEV)
    nl = len(case["acts"])
    pl = Plan(case["dims"], [1] * nl, case["acts"], ec.XOR_LIK, dtype, DEV)
    x, y = ec.mlp_data(name)
    pl.set_data(_t(x, dtype), _t(y, dtype))
    loc, scale = d["prior"]
    if case.get("laplace"):
        pl.set_prior_family(L.EY_PRIOR_LAPLACE, torch.tensor(loc), torch.tensor(scale))
    else:
        pl.set_prior(torch.tensor(loc), torch.tensor(scale))
    assert pl.P == d["theta"].shape[1]
    return pl


def _device(name, dtype, chains=slice(None)):
    """The case's device arguments for the chains selected: theta, the base, temps, max_shrinks."""
    d = ec.inputs(name)
    base = dict(base_loc=None, base_scale=None)
    if d["base"] is not None:
        base = dict(base_loc=_t(d["base"][0], dtype), base_scale=_t(d["base"][1], dtype))
    return dict(th=_t(d["theta"][chains], dtype), base=base, max_shrinks=d["max_shrinks"],
                temp=None if d["temps"] is None else _t(d["temps"][chains], dtype))


def _start(pl, dev):
    th = dev["th"].clone()
    ell, tv = pl.eslice_ell(th, temp=dev["temp"], **dev["base"])
    return th, tv.contiguous(), ell.contiguous()


def _compare(name, outs_dev, states_dev, outs_ref):
    """The margin rule over the draws of a case.  Returns the number of (chain, draw) pairs compared."""
    live = np.ones(len(outs_ref[0]["n_evals"]), bool)
    compared = 0
    for k, (od, sd, orf) in enumerate(zip(outs_dev, states_dev, outs_ref)):
        live &= orf["margin"] > ec.MARGIN
        compared += int(live.sum())
        if not live.any():
            break
        for key in ("accepted", "n_evals"):
            got = od[key].cpu().numpy().astype(int)
            assert np.array_equal(got[live], orf[key][live].astype(int)), (name, k, key, got, orf[key], orf["margin"])
        for key, got in zip(("theta", "target", "ell"), sd):
            want, g = orf[key][live], got[live]
            scale = np.abs(want).max(axis=-1, keepdims=True) if want.ndim == 2 else np.abs(want).max()
            err = np.abs(g - want)
            assert (err <= RTOL * scale).all(), (name, k, key, float((err / np.maximum(scale, 1e-300)).max()))
    return compared


def _draws_on_device(pl, dev, state, n, **kw):
    th, tv, ell = state
    outs, states = [], []
    for k in range(n):
        args = {key: (v[k] if key in ("z", "u") else v) for key, v in kw.items()}
        if "it" in args:
            args["it"] = kw["it"] + k
        out = pl.eslice_step(th, tv, ell, max_shrinks=dev["max_shrinks"], temp=dev["temp"], **dev["base"], **args)
        outs.append({key: v.clone() for key, v in out.items()})
        states.append((_np(th), _np(tv), _np(ell)))
    return outs, states


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(ec.CASES))
def test_parity_with_given_randoms(name):
    """f64, C = 11, explicit z / u: four consecutive draws from the state eslice_ell gives."""
    pl = _plan(name, F64)
    dev = _device(name, F64)
    d = ec.inputs(name)
    state = _start(pl, dev)
    th, tv, ell = (_np(t) for t in state)
    # the start itself: ell and the target at the first states, by the restatement
    _, ell0, tv0 = ec.start(name)
    np.testing.assert_allclose(ell, ell0, rtol=RTOL, atol=RTOL * np.abs(ell0).max())
    np.testing.assert_allclose(tv, tv0, rtol=RTOL, atol=RTOL * np.abs(tv0).max())
    ref = ec.restate(name, state=(th, ell, tv))
    outs, states = _draws_on_device(pl, dev, state, ec.DRAWS, z=_t(d["z"], F64), u=_t(d["u"], F64))
    n = _compare(name, outs, states, ref)
    evals = np.stack([o["n_evals"].cpu().numpy() for o in outs])
    moved = int(sum(o["accepted"].sum() for o in outs))
    print(f"{name}: {n} of {ec.C * ec.DRAWS} draws compared, n_evals {np.bincount(evals.ravel()).tolist()}, moved {moved}")
    assert n >= (1 - ec.MAX_UNDER) * ec.C * ec.DRAWS
    if d["max_shrinks"] == 2:
        assert 0 < moved < ec.C * ec.DRAWS and evals.max() == 3
    else:
        assert moved == ec.C * ec.DRAWS


@pytest.mark.parametrize("name", ["xor", "lin12/temp", "mvn70/base"])
def test_parity_on_the_streams(name):
    """z = u = NULL in f64: the restatement on the Philox oracle's normals and uniform block words."""
    pl = _plan(name, F64)
    dev = _device(name, F64)
    state = _start(pl, dev)
    th, tv, ell = (_np(t) for t in state)
    z = np.stack([po.normal(ec.C, pl.P, SEED, IT0 + k, dtype=np.float64) for k in range(ec.DRAWS)])
    u = np.stack([po.uniform_blocks(np.arange(ec.C), er.words(), SEED, IT0 + k, dtype=np.float64) for k in range(ec.DRAWS)])
    ref = ec.restate(name, state=(th, ell, tv), z=z, u=u)
    outs, states = _draws_on_device(pl, dev, state, ec.DRAWS, seed=SEED, it=IT0)
    n = _compare(name, outs, states, ref)
    print(f"{name} on the streams: {n} of {ec.C * ec.DRAWS} draws compared")
    assert n >= (1 - ec.MAX_UNDER) * ec.C * ec.DRAWS


# ------------------------------------------------------------------------------------------------ run against step
def _run_records(C, P, dtype, n):
    return dict(samples=torch.empty(n, C, P, dtype=dtype, device=DEV), targets=torch.empty(n, C, dtype=dtype, device=DEV),
                accepted_rec=torch.empty(n, C, dtype=torch.uint8, device=DEV),
                accept_count=torch.zeros(C, dtype=torch.int32, device=DEV),
                n_evals_rec=torch.empty(n, C, dtype=torch.int32, device=DEV))


def _carried_is_fresh(pl, dev, th, tv, ell, f64):
    """tests.test_invariance_gpu._carried_state_is_fresh's tolerances, on the target and on ell."""
    lik, prior = pl.log_target(th.clone(), temp=dev["temp"])
    e1, t1 = pl.eslice_ell(th.clone(), temp=dev["temp"], **dev["base"])
    rtol, atol = (1e-9, 1e-9) if f64 else (2e-4, 2e-3)
    np.testing.assert_allclose(_np(tv), _np(lik + prior), rtol=rtol, atol=atol)
    np.testing.assert_allclose(_np(tv), _np(t1), rtol=rtol, atol=atol)
    np.testing.assert_allclose(_np(ell), _np(e1), rtol=rtol, atol=atol)


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("name", ["lin12/temp", "mvn70/base", "mix2/base/shrinks2"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_run_is_its_steps_bit_for_bit(dtype, name, C):
    """With and without a base, with a temperature, and where some chains stay: all records, and the carried state."""
    pl = _plan(name, dtype)
    dev = _device(name, dtype, slice(6, 7) if C == 1 else slice(None))
    a = _start(pl, dev)
    b = tuple(t.clone() for t in a)
    rec = _run_records(C, pl.P, dtype, K_RUN)
    kw = dict(max_shrinks=dev["max_shrinks"], temp=dev["temp"], seed=SEED, **dev["base"])
    oa = pl.eslice_run(*a, K_RUN, it=IT0, **kw, **rec)
    for k in range(K_RUN):
        ob = pl.eslice_step(*b, it=IT0 + k, **kw)
        assert torch.equal(rec["samples"][k], b[0]) and torch.equal(rec["targets"][k], b[1]), k
        assert torch.equal(rec["accepted_rec"][k], ob["accepted"]) and torch.equal(rec["n_evals_rec"][k], ob["n_evals"]), k
    for x, y in list(zip(a, b)) + [(oa[key], ob[key]) for key in oa]:
        assert torch.equal(x, y)
    assert torch.equal(rec["accept_count"], rec["accepted_rec"].int().sum(0)) and int(rec["accept_count"].sum()) > 0
    assert torch.isfinite(rec["samples"]).all() and int(rec["n_evals_rec"].min()) >= 1
    if dev["max_shrinks"] == 2 and C > 1:
        assert int(rec["accepted_rec"].sum()) < K_RUN * C
    _carried_is_fresh(pl, dev, *a, dtype == F64)


def test_raising_max_shrinks_moves_no_variate():
    """max_shrinks 2 -> 8 on the case's first z / u (tests/test_eslice_host.py: between 3 and 10 of its chains end within
    two shrinks): the draws that ended within two shrinks are the same bits."""
    name = "xor/laplace/base"
    pl, dev, d = _plan(name, F64), _device(name, F64), ec.inputs(name)
    a = _start(pl, dev)
    b = tuple(t.clone() for t in a)
    kw = dict(temp=dev["temp"], z=_t(d["z"][0], F64), u=_t(d["u"][0], F64), **dev["base"])
    o2 = pl.eslice_step(*a, max_shrinks=2, **kw)
    o8 = pl.eslice_step(*b, max_shrinks=8, **kw)
    within = o2["accepted"].bool()
    assert 3 <= int(within.sum()) < ec.C and bool((o8["n_evals"][~within] > 3).all()) and bool((o2["n_evals"] <= 3).all())
    for x, y in list(zip(a, b)) + [(o2[key], o8[key]) for key in o2]:
        assert torch.equal(x[within], y[within])
    assert torch.equal(a[0][~within], dev["th"][~within]) and not torch.equal(a[0][~within], b[0][~within])


def test_attached_moments_equal_the_moments_of_the_records():
    """As the other run kernels of the generic family (tests/test_mh_mvn_gpu.py's test and bounds): the moments are
    replayed from the records, and a run of several draws without them is refused before the launch."""
    name = "mix2/base/shrinks2"     # (some chains stay: their accept flags are 0)
    pl, dev = _plan(name, F64), _device(name, F64)
    th, tv, ell = _start(pl, dev)
    C, K, P = ec.C, K_RUN, pl.P
    s1, s2 = (torch.zeros(C, P, dtype=F64, device=DEV) for _ in range(2))
    acc = torch.zeros(C, dtype=F64, device=DEV)
    rs = torch.empty(K, C, P, dtype=F64, device=DEV)
    ra = torch.empty(K, C, dtype=torch.uint8, device=DEV)
    kw = dict(max_shrinks=2, seed=SEED, **dev["base"])
    pl.attach_moments(s1, s2, acc)
    try:
        pl.eslice_run(th, tv, ell, K, samples=rs, accepted_rec=ra, **kw)
        before = th.clone()
        with pytest.raises(RuntimeError, match="status -2"):
            pl.eslice_run(th, tv, ell, K, it=K, **kw)
        assert torch.equal(th, before)
    finally:
        pl.detach_moments()
    w1, w2 = torch.zeros_like(s1), torch.zeros_like(s2)
    for k in range(K):
        w1 += rs[k]
        w2 += rs[k] * rs[k]
    assert torch.equal(acc, ra.double().sum(0))
    bound = float(rs.abs().sum(0).max())
    np.testing.assert_allclose(s1.cpu().numpy(), w1.cpu().numpy(), rtol=0, atol=K * 2.0 ** -53 * bound)
    np.testing.assert_allclose(s2.cpu().numpy(), w2.cpu().numpy(), rtol=2 * K * 2.0 ** -52, atol=0)
    assert 0 < int(ra.sum()) < K * C


# ------------------------------------------------------------------------------------------------ non-finite, refusals
@pytest.mark.parametrize("name", ["lin12", "mvn70/base"])
def test_a_chain_that_starts_at_a_nan_state_stays_put(name):
    pl, dev = _plan(name, F64), _device(name, F64)
    a = _start(pl, dev)
    dev_b = dict(dev, th=dev["th"].clone())
    dev_b["th"][4] = float("nan")
    b = _start(pl, dev_b)
    assert torch.isnan(b[2][4])
    kw = dict(max_shrinks=dev["max_shrinks"], seed=SEED, it=IT0, **dev["base"])
    oa, ob = pl.eslice_step(*a, **kw), pl.eslice_step(*b, **kw)
    assert int(ob["n_evals"][4]) == 0 and int(ob["accepted"][4]) == 0
    assert torch.isnan(b[0][4]).all() and torch.isnan(b[2][4])
    others = torch.arange(ec.C, device=DEV) != 4
    for x, y in list(zip(a, b)) + [(oa[key], ob[key]) for key in oa]:
        assert torch.equal(x[others], y[others])
    assert int(oa["n_evals"][4]) >= 1 and int(oa["accepted"][4]) == 1


def test_refusals_leave_theta_untouched():
    from eeyore_amd.plan import _stream
    from tests.test_invariance_gpu import _plan as iv_plan
    lib = L.lib()
    pl, dev = _plan("lin12", F64), _device("lin12", F64)
    th, tv, ell = _start(pl, dev)
    before = th.clone()
    P, C = pl.P, ec.C
    acc, ne = torch.zeros(C, dtype=torch.uint8, device=DEV), torch.zeros(C, dtype=torch.int32, device=DEV)
    ones = torch.ones(P, dtype=F64, device=DEV)

    def raw_step(plan, t, tg, el, loc, scale, u=None, S=0, max_shrinks=8):
        return lib.ey_eslice_step(plan.handle, L.ptr(t), L.ptr(tg), L.ptr(el), L.ptr(loc), L.ptr(scale), None, L.ptr(u), S,
                                  max_shrinks, None, t.shape[0], SEED, 0, 0, 0, L.ptr(acc), L.ptr(ne), _stream(plan.device))
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_shrinks"):
            pl.eslice_step(th, tv, ell, max_shrinks=bad, seed=SEED)
        with pytest.raises(ValueError, match="max_shrinks"):
            pl.eslice_run(th, tv, ell, 2, max_shrinks=bad, seed=SEED)
    with pytest.raises(ValueError, match="S >= 2 \\+ max_shrinks"):
        pl.eslice_step(th, tv, ell, u=torch.rand(C, 9, dtype=F64, device=DEV), max_shrinks=8, seed=SEED)
    # one base table without the other: refused in Python, and by the library below it
    with pytest.raises(ValueError, match="go together"):
        pl.eslice_step(th, tv, ell, base_loc=ones, seed=SEED)
    with pytest.raises(ValueError, match="go together"):
        pl.eslice_ell(th, base_scale=ones)
    assert raw_step(pl, th, tv, ell, ones, None) == -1 and b"exactly one of them is null" in lib.ey_last_error()
    assert raw_step(pl, th, tv, ell, None, ones) == -1 and b"exactly one of them is null" in lib.ey_last_error()
    # a scale that is not positive and finite: Python's refusal, where the tables are on hand
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="positive and finite"):
            pl.eslice_step(th, tv, ell, base_loc=0 * ones, base_scale=bad * ones, seed=SEED)
    # no base on a plan whose prior is not Normal, or on a distribution plan
    lap, mix = _plan("xor/laplace/base", F64), _plan("mvn70/base", F64)
    for other, name in ((lap, "xor/laplace/base"), (mix, "mvn70/base")):
        d2 = _device(name, F64)
        s2 = _start(other, d2)
        keep = s2[0].clone()
        with pytest.raises(ValueError, match="give the Gaussian base"):
            other.eslice_step(*s2, seed=SEED)
        with pytest.raises(ValueError, match="give the Gaussian base"):
            other.eslice_run(*s2, 2, seed=SEED)
        with pytest.raises(ValueError, match="give the Gaussian base"):
            other.eslice_ell(s2[0])
        torch.cuda.synchronize()
        assert torch.equal(s2[0], keep)
    # a plan with ey_plan_attach_da attached (tests/test_nuts_gpu.py's)
    from tests.test_ram_gpu import CASES, _data
    from tests.test_ram_gpu import _plan as _mlp_plan
    dims, acts, lik, n_rows = CASES["mlp483"]
    fused = _mlp_plan(dims, acts, lik, *_data(dims, lik, n_rows), F32)
    thf = torch.zeros(C, fused.P, dtype=F32, device=DEV)
    ef, tf = fused.eslice_ell(thf)
    state, step_vec = torch.zeros(C, 3, dtype=F64, device=DEV), torch.full((C,), 0.05, dtype=F32, device=DEV)
    fused.attach_da(state, step_vec, torch.ones(4, 3, dtype=F64, device=DEV), 4, 0.65)
    try:
        for call in (lambda: fused.eslice_step(thf, tf, ef, seed=SEED), lambda: fused.eslice_run(thf, tf, ef, 2, seed=SEED)):
            with pytest.raises(ValueError, match="ey_plan_attach_da"):
                call()
    finally:
        fused.detach_da()
    torch.cuda.synchronize()
    assert bool((thf == 0).all()) and bool((state == 0).all())
    # an LDS image beyond 160 KiB (dims [400, 1] in f64: 401 activation rows of 65 doubles), EY_ERR_UNSUPPORTED with the
    # byte count; the plan of dims [200, 1], which HMC runs on the layerwise kernels, is served
    from eeyore_amd.plan import Plan
    big = Plan([400, 1], [1], [1], 0, F64, DEV)
    big.set_data(torch.zeros(4, 400, dtype=F64, device=DEV), torch.zeros(4, 1, dtype=F64, device=DEV))
    big.set_prior(torch.zeros(big.P), torch.ones(big.P))
    mid = iv_plan("lin200", "f64")
    assert mid.kernel == "bgemm" and torch.isfinite(mid.eslice_ell(torch.zeros(3, mid.P, dtype=F64, device=DEV))[0]).all()
    thb = torch.zeros(3, big.P, dtype=F64, device=DEV)
    tb = torch.zeros(3, dtype=F64, device=DEV)
    acc, ne = acc[:3].clone(), ne[:3].clone()
    assert raw_step(big, thb, tb, tb.clone(), None, None) == -2
    msg = lib.ey_last_error()
    assert b"bytes) do not fit the 160 KiB LDS" in msg and int(msg.split(b"(")[1].split(b" ")[0]) > 160 * 1024
    with pytest.raises(RuntimeError, match="160 KiB"):
        big.eslice_ell(thb)
    torch.cuda.synchronize()
    assert torch.equal(th, before) and bool((thb == 0).all())


# ------------------------------------------------------------------------------------------------ the sampler
def _xor_sampler(rng, fused_block=256, C=8, keys=('sample', 'target_val', 'accepted', 'n_evals'), base=None):
    from torch.distributions import Normal
    from torch.utils.data import DataLoader
    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import EllipticalSlice
    xor = XYDataset.from_eeyore('xor', dtype=F64, device=DEV)
    hp = mlp.Hyperparameters(dims=[2, 2, 1], bias=[True, True], activations=[torch.sigmoid, torch.sigmoid])
    model = mlp.MLP(loss=loss_functions['binary_classification'], hparams=hp, dtype=F64, device=DEV)
    model.prior = Normal(torch.zeros(9, dtype=F64, device=DEV), 3 * torch.ones(9, dtype=F64, device=DEV))
    th0 = _t(0.3 * np.random.default_rng(2).standard_normal((C, 9)), F64)
    s = EllipticalSlice(model, theta0=th0, dataloader=DataLoader(xor, batch_size=len(xor), shuffle=False), rng=rng, seed=SEED,
                        chain=ChainBuffer(keys=list(keys)), base=base)
    s.fused_block = fused_block
    return s, model, th0


def test_sampler_on_the_streams_reproduces_eslice_run():
    n, burn = 12, 4
    s, model, th0 = _xor_sampler('philox')
    assert s._can_fuse(False)
    s.run(num_epochs=n, num_burnin_epochs=burn)
    plan = s.model._plan(*next(iter(s.dataloader)))
    th = th0.clone()
    ell, tv = plan.eslice_ell(th)
    rec = _run_records(8, 9, F64, n)
    out = plan.eslice_run(th, tv, ell, n, seed=SEED, it=0, **rec)
    ch = s.get_chain()
    assert len(ch) == n - burn
    assert torch.equal(ch.get_samples(), rec["samples"][burn:]) and torch.equal(ch.get_target_vals(), rec["targets"][burn:])
    assert torch.equal(ch.get_accepted(), rec["accepted_rec"][burn:]) and torch.equal(ch.bufs['n_evals'][:len(ch)], rec["n_evals_rec"][burn:])
    assert torch.equal(s._theta, th) and torch.equal(s.last['n_evals'], out['n_evals'])
    assert torch.equal(s.current['n_evals'], out['n_evals']) and bool(ch.get_accepted().all())
    # ... and draw by draw (no blocks) it is the same chain
    s1, _, _ = _xor_sampler('philox', fused_block=0)
    s1.run(num_epochs=n, num_burnin_epochs=burn)
    assert torch.equal(s1.get_chain().get_samples(), ch.get_samples())
    assert torch.equal(s1.get_chain().bufs['n_evals'][:len(ch)], ch.bufs['n_evals'][:len(ch)])


def test_sampler_on_the_torch_generator_runs_and_records_n_evals():
    from torch.distributions import Normal
    torch.manual_seed(5)
    base = Normal(torch.zeros(9, dtype=F64), 2.0 * torch.ones(9, dtype=F64))
    for b in (None, base):
        s, _, _ = _xor_sampler('torch', base=b)
        assert not s._can_fuse(False)
        s.run(num_epochs=10, num_burnin_epochs=2)
        ch = s.get_chain()
        ne = ch.bufs['n_evals'][:len(ch)]
        assert len(ch) == 8 and tuple(ne.shape) == (8, 8) and ne.dtype == torch.int32
        assert int(ne.min()) >= 1 and int(ne.max()) <= 65 and bool(ch.get_accepted().all())
        assert torch.isfinite(ch.get_samples()).all() and torch.equal(s.last['n_evals'], ne[-1])
        moved = (ch.get_samples()[1:] != ch.get_samples()[:-1]).any(-1)
        assert bool(moved.all())
