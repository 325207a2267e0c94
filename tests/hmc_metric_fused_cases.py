"""The parity cases of HMC under a diagonal metric on the matrix cores (k_hmc_metric_mfma):
tests/test_hmc_metric_fused_gpu.py runs them on the device, tests/test_hmc_metric_fused_host.py holds them to the coverage and
margin rules on the CPU.  TEST INFRASTRUCTURE ONLY, numpy only.

A case is an f32 MLP(4-32-32-dK) plan on standardised iris rows (tests/eslice_fused_cases.py's rows and models), C = 11
chains, three draws of ``num_steps`` leapfrog steps under a diagonal metric with scales in [0.5, 1.5], restated by
``hmc_metric_restatement.hmc_metric_draw`` on ``oracle.mlp_oracle`` in f64.  A step per chain: the prior's stability limit
2 / max(scale / sigma) times FACTORS, from 0.02 of it to a hundred times it; the last makes a non-finite or hugely uphill
trajectory that must reject.  Everything the device is given is rounded to f32 BEFORE the restatement sees it (theta, v0, u,
the rows, the steps, the temperatures, the prior and metric tables), and every draw starts from the restatement's state of
the draw before rounded to f32, with the target and the gradient evaluated afresh there: a device draw that decides otherwise
costs one (chain, draw) pair.

THE ACCEPT VARIATES ARE CONDITIONED.  The decision margin of a pair is |min(H_cur - H_prop, 0) - log u|, a NaN rate counting
as +inf (it rejects whatever u is).  For each (draw, chain) in order the generator redraws that pair's u from the seeded
generator until the margin exceeds MARGIN_FLOOR; the loop is bounded (MAX_TRIES) and v0 is never redrawn.  By the restatement
alone every pair of every case is then above MARGIN_FLOOR.

A pair is BLOWN when the restatement's H_prop is not below BLOWN in magnitude (the hundredfold step: 1e9 and beyond, infinite,
or NaN where the naive logs of the BCE head saturate).  An f32 kernel cannot be held to an absolute tolerance there -- it
overflows where f64 does not -- so of a blown pair the device comparison asks for the decision (reject), the untouched state,
a rate that is 0 or NaN and an H_prop that is itself not below BLOWN / 2.  Every other pair's H_prop is at most CALM in
magnitude (the host test holds the gap), the size of the targets themselves, and is compared absolutely."""
import functools

import numpy as np

from oracle import mlp_oracle as orc
from tests import eslice_fused_cases as fc
from tests import hmc_metric_restatement as hr

C, DRAWS = 11, 3
PAIRS = C * DRAWS
MARGIN_FLOOR = 0.05
MAX_TRIES = 60
BLOWN, CALM = 1e6, 5e3
HEADLINE, BCE_TANH = fc.HEADLINE, fc.BCE_TANH
SIGMA = 0.3            # the uniform prior's width (tests/nuts_fused_cases.py's)
FACTORS = np.array([0.02, 0.04, 0.06, 0.08, 0.1, 0.13, 0.16, 0.2, 0.25, 0.3, 100.0])
# (330 rows: the likelihood's curvature exceeds the prior's, and the same energy errors are reached at half the step)
FACTORS_N330 = np.array([0.02, 0.03, 0.04, 0.05, 0.06, 0.08, 0.1, 0.12, 0.14, 0.16, 100.0])
CASES = {
    "n33/L1": dict(N=33, L=1),                      # only the half-weight last kick
    "n33": dict(N=33, L=3),                         # two row tiles, a short last one
    "n150": dict(N=150, L=8, sigma=0.15),
    "n150/bce-tanh": dict(N=150, L=3, model=BCE_TANH, sigma=0.15),
    "n33/exact": dict(N=33, L=3, products="exact"),
    "n33/prior/temp": dict(N=33, L=3, prior="elementwise", temp=True),
    "n33/index": dict(N=33, L=3, G=3),
    "n330": dict(N=330, L=3, factors=FACTORS_N330),   # 11 row tiles > MF_TRD_TILES: the bf16x3 form without piece images
}
VALUES = ("target", "h_cur", "h_prop", "rate", "theta", "grad")
f32 = fc.f32


def model_of(name):
    return CASES[name].get("model", HEADLINE)


def rows_of(N):
    """(x [N, 4], labels [N]): the standardised iris rows; beyond 150 the rows repeated with a seeded jitter, labels kept."""
    xs, lab = fc.iris()
    reps = -(-N // len(xs))
    if reps == 1:
        return xs[:N], lab[:N]
    jitter = 0.05 * np.random.default_rng(330).standard_normal((reps * len(xs), xs.shape[1]))
    jitter[:len(xs)] = 0.0
    return (np.tile(xs, (reps, 1)) + jitter)[:N], np.tile(lab, reps)[:N]


@functools.lru_cache(maxsize=None)
def setup(name):
    """What a case fixes before any draw: dict(x, y, theta [C, P], steps [C], temps [C] or None, prior (mu, sigma), tables
    [G, P], index [C] int or None, products, factors, L), every float array f64 holding f32 values."""
    case, model = CASES[name], model_of(name)
    rng = np.random.default_rng([len(name), sum(name.encode()), 53])
    spec = orc.Spec(model["dims"], model["acts"], model["lik"])
    P, N = spec.P, case["N"]
    xs, lab = rows_of(N)
    x = f32(xs)
    y = np.eye(3)[lab] if model["lik"] == orc.LIK_CE else (lab > 0).astype(np.float64)[:, None]
    sigma = case.get("sigma", SIGMA)
    if case.get("prior") == "elementwise":
        prior = (f32(0.1 * rng.standard_normal(P)), f32(sigma * (0.9 + 0.2 * rng.random(P))))
    else:
        prior = (np.zeros(P), f32(np.full(P, sigma)))
    G = case.get("G", 1)
    tables = f32(0.5 + rng.random((G, P)))
    index = rng.integers(0, G, C) if G > 1 else None
    if index is not None:
        index[:G] = np.arange(G)   # every table is used
    temps = f32(0.4 + 0.6 * rng.random(C)) if case.get("temp") else None
    rows = tables[index] if index is not None else np.broadcast_to(tables[0], (C, P))
    limit = 2.0 / (rows / prior[1]).max(axis=1)
    theta = f32(prior[0] + prior[1] * 0.5 * rng.standard_normal((C, P)))
    factors = case.get("factors", FACTORS)
    return dict(x=x, y=y, theta=theta, steps=f32(limit * factors), temps=temps, prior=prior, tables=tables, index=index,
                products=case.get("products", "bf16x3"), factors=factors, P=P, L=case["L"])


def chain_functions(name):
    """One f(theta) -> (target, grad) per chain in f64 (the chain's temperature inside)."""
    d, model = setup(name), model_of(name)
    spec = orc.Spec(model["dims"], model["acts"], model["lik"], mu=d["prior"][0], sigma=d["prior"][1])

    def f(th, t):
        with np.errstate(all="ignore"):
            tv, g = orc.upto_grad_log_target(spec, np.asarray(th, np.float64), d["x"], d["y"], t)
        return float(tv), g
    return [functools.partial(f, t=None if d["temps"] is None else float(d["temps"][c])) for c in range(C)]


def scales(name, c):
    d = setup(name)
    return d["tables"][0 if d["index"] is None else d["index"][c]]


def evaluate(name, theta):
    """(target [C], grad [C, P]) of the f64 oracle at theta [C, P]."""
    fs = chain_functions(name)
    tg = [fs[c](theta[c]) for c in range(C)]
    return np.array([a for a, _ in tg]), np.stack([b for _, b in tg])


def margin_of(h_cur, h_prop, u):
    """|min(H_cur - H_prop, 0) - log u|; +inf where the rate is NaN (it rejects whatever u is)."""
    with np.errstate(all="ignore"):
        d = np.float64(h_cur) - np.float64(h_prop)
        if np.isnan(d):
            return np.inf
        m = abs(min(d, 0.0) - np.log(np.float64(u)))
    return float(m)   # (NaN where both are -inf: no margin, u is redrawn)


KEYS = ("theta", "target", "grad", "accepted", "h_cur", "h_prop", "rate")


def one_draw(name, fs, c, th, t, g, v, u, draw=hr.hmc_metric_draw, metric=None):
    d = setup(name)
    with np.errstate(all="ignore"):
        out = draw(fs[c], th, t, g, hr.DIAG, scales(name, c) if metric is None else metric, v, u, d["steps"][c], d["L"])
    o = dict(zip(KEYS, out[:7]))
    o["margin"] = margin_of(o["h_cur"], o["h_prop"], u)
    return o


def restate_draw(name, theta, t, g, v0, u):
    """One draw of the C chains by the restatement from (theta, t, g) with the tables v0 [C, P], u [C]."""
    fs = chain_functions(name)
    outs = [one_draw(name, fs, c, theta[c], t[c], g[c], v0[c], u[c]) for c in range(C)]
    return {k: np.array([o[k] for o in outs]) for k in outs[0]}


@functools.lru_cache(maxsize=None)
def restate(name):
    """The tables and the DRAWS draws of a case: (v0 [DRAWS, C, P], u [DRAWS, C] conditioned, outs), outs a list of dicts over
    the chains -- start_theta / start_target / start_grad (the f32 state a draw starts from and the oracle's values there),
    the ``hmc_metric_draw`` outputs, margin, and tries (the attempts each pair's u took)."""
    d, fs = setup(name), chain_functions(name)
    P = d["P"]
    rng = np.random.default_rng([len(name), sum(name.encode()), 59])
    v0, u = f32(rng.standard_normal((DRAWS, C, P))), np.empty((DRAWS, C))
    th = d["theta"].copy()
    outs = []
    for k in range(DRAWS):
        t, g = evaluate(name, th)
        rows, tries = [], np.zeros(C, int)
        for c in range(C):
            # the trajectory does not depend on u: one restatement, then u redrawn against its Hamiltonians
            o = one_draw(name, fs, c, th[c], t[c], g[c], v0[k, c], 0.5)
            for attempt in range(MAX_TRIES):
                u[k, c] = f32(rng.random())
                if margin_of(o["h_cur"], o["h_prop"], u[k, c]) > MARGIN_FLOOR:
                    break
            else:
                raise AssertionError(f"{name}: no u of chain {c}, draw {k} cleared the margin in {MAX_TRIES} attempts")
            tries[c] = attempt + 1
            rows.append(one_draw(name, fs, c, th[c], t[c], g[c], v0[k, c], u[k, c]))
        o = {key: np.array([r[key] for r in rows]) for key in rows[0]}
        o.update(start_theta=th.copy(), start_target=t, start_grad=g, tries=tries)
        outs.append(o)
        th = f32(o["theta"])   # the next draw starts from this state as the device holds it
    return v0, u, outs


@functools.lru_cache(maxsize=None)
def restate_identity(name):
    """The case's first draw under IDENTITY scales (the draw ey_hmc_step makes with p0 = v0): (u [C] conditioned as in
    ``restate``, outs), v0 being the case's own first table."""
    d, fs = setup(name), chain_functions(name)
    v0 = restate(name)[0][0]
    rng = np.random.default_rng([len(name), sum(name.encode()), 61])
    one = np.ones(d["P"])
    t, g = evaluate(name, d["theta"])
    u, rows = np.empty(C), []
    for c in range(C):
        o = one_draw(name, fs, c, d["theta"][c], t[c], g[c], v0[c], 0.5, metric=one)
        for _ in range(MAX_TRIES):
            u[c] = f32(rng.random())
            if margin_of(o["h_cur"], o["h_prop"], u[c]) > MARGIN_FLOOR:
                break
        else:
            raise AssertionError(f"{name}: no u of chain {c} cleared the margin under identity scales")
        rows.append(one_draw(name, fs, c, d["theta"][c], t[c], g[c], v0[c], u[c], metric=one))
    return u, {key: np.array([r[key] for r in rows]) for key in rows[0]}


def blown(o):
    """The pairs of one draw whose H_prop is not below BLOWN in magnitude (NaN and infinite included)."""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(o["h_prop"]) < BLOWN)


def coverage(name):
    """(accepted pairs, rejected pairs, blown pairs, non-finite H_prop, smallest margin, attempts per pair, largest calm
    |H_prop|) of a case."""
    _, _, outs = restate(name)
    acc = np.concatenate([o["accepted"] for o in outs])
    bl = np.concatenate([blown(o) for o in outs])
    hp = np.concatenate([o["h_prop"] for o in outs])
    margin = np.concatenate([o["margin"] for o in outs])
    tries = np.concatenate([o["tries"] for o in outs])
    return (int(acc.sum()), int((~acc.astype(bool)).sum()), int(bl.sum()), int((~np.isfinite(hp)).sum()), float(margin.min()),
            float(tries.mean()), float(np.abs(hp[~bl]).max()))
