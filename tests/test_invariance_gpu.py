"""Every non-adaptive sampler on the device leaves a known target invariant ("Invariance from exact draws";
the harness is tests/invariance.py, calibrated on the CPU by tests/test_invariance_host.py).

Each case: C = 16384 chains start from exact draws of the target (rounded to the plan's dtype), ``target`` / ``grad`` from
``log_target_grad``, n = 16 iterations through the ``*_run`` entry point -- in-kernel Philox, one launch, a seed of its own
-- and the final states held against 65536 exact draws made on the host in f64.  A case asserts that (1) the largest |z|
over its features is below ``threshold(K_TOTAL)``, the Bonferroni quantile that gives this whole file a false-alarm
probability of 1e-3 under exact invariance (derived, not measured); (2) the mean acceptance lies in [0.3, 0.97]; (3) the
carried target and gradient equal a fresh ``log_target_grad`` at the final states at the tolerances of the generic family's
parity tests (tests/test_dist_gpu.py: rtol 1e-9 in f64; rtol 2e-4 with atol 2e-3 on values in f32); and prints one line.
The ladder cases are driven by hand as tests/test_pt_between_gpu.py drives the move: one within-chain iteration under the
[K R] temperature vector, then ``pt_between``, 16 times; K = 4 temperatures of R = 4096 replicas, each temperature's rows
against its own law.  Four controls run ordinary calls that do not leave the target invariant and must be flagged with
more than twice the threshold.

Left out on purpose: RAM, AM, AM-softabs, in-kernel dual averaging and the windowed warm-up adapt, so they are not
invariant at any finite n; the fused families (mfma32, fused16, mid32) serve only models that have no exact sampler.
The layerwise family is in: a linear-Gaussian plan of dims [200, 1] in f64 reports "bgemm", and ``hmc_run`` on it is one
more case.  Gibbs runs on the linear-Gaussian plans only (dims [3, 1] in f64 where the minimum list names the mixture
of P = 5, M = 3): the library refuses Gibbs on a mixture plan by design, which tests/test_dist_gpu.py
holds it to."""
import functools

import numpy as np
import pytest
import torch

from tests import invariance as iv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f64": torch.float64, "f32": torch.float32}
C, N, N_REF = iv.C_GPU, iv.N_ITERS, iv.N_REF
THRESHOLD = iv.threshold(iv.K_TOTAL)
NAMES = [c["name"] for c in iv.CASES]
SEED0 = 4100   # case k runs on seed SEED0 + k, the controls behind them


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _plan(target, dtype):
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import Plan
    tgt = iv.target_of(target)
    if target in iv.LINEAR:
        D, n_rows = iv.LINEAR[target]
        x, y, _ = iv.linear_gaussian(D, n_rows)
        pl = Plan([D, 1], [1], [0], L.EY_LIK_GAUSS_SUM, DT[dtype], DEV)
        pl.set_data(_t(x, DT[dtype]), _t(y, DT[dtype]))
        pl.set_prior(torch.zeros(pl.P), torch.full((pl.P,), iv.PRIOR_SIGMA))
        pl.set_lik_scale(iv.LIK_SCALE)
    else:
        from tests.test_dist_gpu import _mixture
        from tests.test_dist_gpu import _plan as mix_plan
        (c, mean, prec), covs = _mixture(tgt.P, tgt.M)
        assert np.array_equal(c, tgt.c) and np.array_equal(mean, tgt.mean) and np.array_equal(prec, tgt.prec)
        assert np.array_equal(covs, tgt.covs)
        pl = mix_plan(tgt.P, tgt.M, DT[dtype])[0]
    assert pl.P == tgt.P
    return pl


def _case_plan(case):
    pl = _plan(case["target"], case["dtype"])
    assert pl.kernel == case.get("kernel", pl.kernel)   # the family a case is there for
    return pl


def _within(pl, case, s, th, tv, gr, n, seed, it, count, mode="intended", gibbs_table=None):
    """n iterations of the case's sampler from iteration ``it`` in one launch of its run entry point."""
    name = case["sampler"]
    kw = dict(temp=s["temps"], seed=seed, it=it, accept_count=count)
    if name == "hmc":
        pl.hmc_run(th, tv, gr, case["step"], case["L"], n, step_vec=s["step_vec"], **kw)
    elif name == "mala":
        pl.mala_run(th, tv, gr, case["step"], n, step_vec=s["step_vec"], **kw)
    elif name == "mh":
        pl.mh_run(th, tv, case["scale"], n, **kw)
    elif name == "mh_tril":
        pl.mh_tril_run(th, tv, s["table"], n, index=s["index"], **kw)
    elif name == "mala_tril":
        pl.mala_tril_run(th, tv, gr, case["step"], s["table"], n, index=s["index"], step_vec=s["step_vec"], **kw)
    elif name == "hmc_metric":
        pl.hmc_metric_run(th, tv, gr, case["step"], case["L"], s["table"], case["kind"], n, index=s["index"],
                          step_vec=s["step_vec"], **kw)
    elif name == "gibbs":
        pl.gibbs_run(th, tv, gibbs_table, n, mode=mode, **kw)
    else:
        raise ValueError(name)


def _start(case, seed, chains=C):
    """(plan, the case's device arguments, theta, target, grad, the host generator behind the start)."""
    dtype = DT[case["dtype"]]
    pl = _case_plan(case)
    s = iv.setup(case, chains)
    rng = np.random.default_rng([seed, 1])
    th = _t(iv.start(case, chains, rng), dtype)
    dev = dict(temps=None if s["temps"] is None else _t(s["temps"], dtype),
               step_vec=None if s["step_vec"] is None else _t(s["step_vec"], dtype),
               table=None if s["table"] is None else _t(s["table"], dtype),
               index=None if s["index"] is None else torch.tensor(s["index"], dtype=torch.int32, device=DEV))
    tv, gr = pl.log_target_grad(th, temp=dev["temps"])
    return pl, s, dev, th, tv.contiguous(), gr.contiguous(), rng


def _carried_state_is_fresh(pl, case, dev, th, tv, gr):
    """(3): the target (and gradient, for the samplers that carry one) the kernel left is the one of its final state."""
    f64 = case["dtype"] == "f64"
    t1, g1 = pl.log_target_grad(th.clone(), temp=dev["temps"])
    rtol = 1e-9 if f64 else 2e-4
    np.testing.assert_allclose(_np(tv), _np(t1), rtol=rtol, atol=1e-9 if f64 else 2e-3)
    if case["sampler"] in ("hmc", "mala", "mala_tril", "hmc_metric"):
        want = _np(g1)
        np.testing.assert_allclose(_np(gr), want, rtol=rtol, atol=rtol * np.abs(want).max())


def _run(name, seed, chains=C, mode="intended"):
    """A case on the device: its plan, arguments and final device state, the final theta and logp = target / temperature
    on the host, the mean acceptance and exchange rate, and the host generator.  ``chains``: a failing case is run again
    once, alone, at 65536 chains and another seed -- a real bias doubles z, chance does not come back."""
    case = iv.CASE[name]
    pl, s, dev, th, tv, gr, rng = _start(case, seed, chains)
    S = len(case["blocks"]) if case["sampler"] == "gibbs" else 0
    count = torch.zeros((chains, S) if S else (chains,), dtype=torch.int32, device=DEV)
    table = pl.gibbs_table(case["blocks"], case["scales"]) if S else None
    swaps = torch.zeros((), dtype=torch.float64, device=DEV)
    if case.get("ladder"):
        ladder = pl.pt_ladder(iv.LADDER_T, iv.ladder_q())
        for it in range(N):
            _within(pl, case, dev, th, tv, gr, 1, seed, it, count)
            out = pl.pt_between(ladder, th, tv, None if case["sampler"] == "mh" else gr, seed=seed, it=it)
            swaps += out["swap"].double().mean()
    else:
        _within(pl, case, dev, th, tv, gr, N, seed, 0, count, mode, table)
    torch.cuda.synchronize()
    assert torch.isfinite(th).all() and torch.isfinite(tv).all()
    logp = _np(tv) if s["temps"] is None else _np(tv) / s["temps"]
    return dict(case=case, pl=pl, dev=dev, th=th, tv=tv, gr=gr, rng=rng, theta=_np(th), logp=logp,
                accept=float(count.double().mean()) / N, swap=float(swaps) / N)


def _report(name, r, z, what=""):
    w, where = iv.worst(z, r["pl"].P)
    k = int(np.argmax(np.abs(z)))
    print(f"{name}{what}: kernel {r['pl'].kernel}, largest |z| {w:.2f} at feature {k % z.shape[-1]} ({where}), acceptance "
          f"{r['accept']:.3f}" + (f", exchanges {r['swap']:.3f}" if r["case"].get("ladder") else "") +
          f", threshold {THRESHOLD:.2f}")
    return w, where


@pytest.mark.parametrize("name", NAMES)
def test_sampler_leaves_its_target_invariant(name):
    """Measured on an MI355X: see the table of DESIGN.md 2 ("Invariance from exact draws")."""
    r = _run(name, SEED0 + NAMES.index(name))
    z = iv.case_z(r["case"], r["theta"], r["logp"], r["rng"], N_REF)
    assert z.size == iv.n_statistics(r["case"])
    w, where = _report(name, r, z)
    assert w < THRESHOLD, (w, where)
    assert iv.ACCEPT_BAND[0] <= r["accept"] <= iv.ACCEPT_BAND[1], r["accept"]
    if r["case"].get("ladder"):
        assert 0.0 < r["swap"] < 1.0
    _carried_state_is_fresh(r["pl"], r["case"], r["dev"], r["th"], r["tv"], r["gr"])


# ------------------------------------------------------------------------------------------------ positive controls
def _flagged(name, r, z, what):
    w, where = _report(name, r, z, what)
    assert w > 2 * THRESHOLD, (w, where)


def test_control_mala_that_accepts_every_proposal_is_flagged():
    """``mala_step`` driven n times with z from ``philox_normal`` and a given u of zeros: log u = -inf accepts every
    proposal, which is the unadjusted Langevin chain and not pi-invariant."""
    name, seed = "mala/mix5_3/f64", SEED0 + len(NAMES)
    case = iv.CASE[name]
    pl, s, dev, th, tv, gr, rng = _start(case, seed)
    u = torch.zeros(C, dtype=DT[case["dtype"]], device=DEV)
    accepted = 0.0
    for it in range(N):
        out = pl.mala_step(th, tv, gr, case["step"], z=pl.philox_normal(C, seed, it), u=u)
        accepted += float(out["accepted"].double().mean())
    assert accepted == N
    r = dict(case=case, pl=pl, accept=accepted / N, swap=0.0)
    _flagged(name, r, iv.case_z(case, _np(th), _np(tv), rng, N_REF), " with u = 0")


def test_control_gibbs_in_the_reference_mode_is_flagged():
    """``mode='reference'`` carries a rejected block in the proposal for the rest of the draw: not a valid
    Metropolis within Gibbs."""
    name = "gibbs/lin3/f64"
    r = _run(name, SEED0 + len(NAMES) + 1, mode="reference")
    _flagged(name, r, iv.case_z(r["case"], r["theta"], r["logp"], r["rng"], N_REF), " in mode 'reference'")


def test_control_between_move_that_always_exchanges_is_flagged():
    """``pt_between`` with given valid partners and a given u of 1e-300: every step exchanges, whatever its rate."""
    name, seed = "ladder/mala/mix5_1/f64", SEED0 + len(NAMES) + 2
    case = iv.CASE[name]
    pl, s, dev, th, tv, gr, rng = _start(case, seed)
    K, R = len(iv.LADDER_T), C // len(iv.LADDER_T)
    count = torch.zeros(C, dtype=torch.int32, device=DEV)
    ladder = pl.pt_ladder(iv.LADDER_T, iv.ladder_q())
    _, _, cdf = iv.ladder_tables(iv.LADDER_T, iv.ladder_q())
    u = torch.full((K, R), 1e-300, dtype=DT[case["dtype"]], device=DEV)
    swaps = 0.0
    for it in range(N):
        _within(pl, case, dev, th, tv, gr, 1, seed, it, count)
        partners = torch.tensor(iv.draw_partners(cdf, rng.random((K, R))), dtype=torch.int32, device=DEV)
        swaps += float(pl.pt_between(ladder, th, tv, gr, partners=partners, u=u)["swap"].double().mean())
    assert swaps == N
    r = dict(case=case, pl=pl, accept=float(count.double().mean()) / N, swap=swaps / N)
    _flagged(name, r, iv.case_z(case, _np(th), _np(tv) / s["temps"], rng, N_REF), " with u = 1e-300")


def test_control_tempered_run_against_the_untempered_law_is_flagged():
    name = "hmc/lin12/f32/temp"
    r = _run(name, SEED0 + len(NAMES) + 3)
    z = iv.case_z(r["case"], r["theta"], r["logp"], r["rng"], N_REF, untempered=True)
    _flagged(name, r, z[1:], " against the law at t = 1")   # (the first half runs at t = 1)
