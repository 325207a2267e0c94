"""The parity cases of NUTS on the matrix cores (k_nuts_mfma): tests/test_nuts_fused_gpu.py runs them on the
device, tests/test_nuts_fused_host.py holds them to the coverage and margin rules on the CPU.  TEST INFRASTRUCTURE ONLY, numpy
only.

A case is an f32 MLP(4-32-32-dK) plan on standardised iris rows (tests/eslice_fused_cases.py's rows and models), C = 11
chains, three draws at max_depth 3 under a diagonal metric with scales in [0.5, 1.5], restated by ``nuts_restatement.nuts_draw``
on ``oracle.mlp_oracle`` in f64.  A step per chain: the prior's stability limit 2 / max(scale / sigma) times the case's
factors, from a fraction of it (the draw stops at max_depth) to a hundred times it (a divergent draw of depth 0).  Everything
the device is given is rounded to f32 BEFORE the restatement sees it (theta, v0, u, the rows, the steps, the temperatures,
the prior and metric tables), and every draw starts from the restatement's state of the draw before rounded to f32, with the
target and the gradient evaluated afresh there: a device draw that decides otherwise costs one (chain, draw) pair.

THE TABLES ARE CONDITIONED.  With random v0 and u too few draws clear a margin of f32 size (of the 21 pairs of
tests/nuts_tree_cases.py's iris case 15 exceed 1e-2 and 12 exceed 2e-2), so for each (draw, chain) in order the generator
redraws that pair's v0 row and u row from the seeded generator until the restatement's smallest decision margin of the draw
exceeds MARGIN_FLOOR.  The loop is seeded and bounded (MAX_TRIES), and a later draw starts from the state the accepted
earlier one left.  By the restatement alone every pair of every case is then above MARGIN_FLOOR."""
import functools

import numpy as np

from oracle import mlp_oracle as orc
from tests import eslice_fused_cases as fc
from tests import nuts_restatement as nr

C, DRAWS, MAX_DEPTH = 11, 3, 3
PAIRS = C * DRAWS
MARGIN_FLOOR = 0.05
MAX_TRIES = 60
S = nr.words(MAX_DEPTH)
HEADLINE, BCE_TANH = fc.HEADLINE, fc.BCE_TANH
SIGMA = 0.3            # the uniform prior's width: narrow enough that the prior's curvature is felt beside the likelihood's
# A chain's role: its step as a multiple of the prior's stability limit, and whether it starts far out (BAND_AMPLITUDE prior
# widths, random signs) in the coordinates whose metric scale exceeds BAND_SCALE.  Under scales spread over [0.5, 1.5] the
# whitened frequencies of a plain start are spread threefold, and in 1315 dimensions no sub-block of seven leaves ever turns;
# a start whose energy sits in a narrow band of frequencies turns together, inside a new subtree ('subblock') or between
# the tree's edges ('tree').
FACTORS = np.array([0.02, 0.2, 0.9, 1.0, 0.3, 0.5, 0.5, 0.5, 0.5, 0.55, 100.0])
BANDED = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0], bool)
BAND_SCALE, BAND_AMPLITUDE = 1.4, 8.0
CASES = {
    "n33": dict(N=33),
    "n150": dict(N=150, sigma=0.15),
    "n150/bce-tanh": dict(N=150, model=BCE_TANH, sigma=0.15),
    "n33/exact": dict(N=33, products="exact"),
    "n33/prior/temp": dict(N=33, prior="elementwise", temp=True,   # (a temperature below 1 slows the chain: longer steps)
                           factors=np.array([0.02, 0.2, 1.0, 1.1, 0.45, 0.7, 0.7, 0.75, 0.8, 0.9, 100.0])),
    "n33/index": dict(N=33, G=3),
}
STOPS = ("divergent", "subblock", "tree", "max_depth")
f32 = fc.f32


def model_of(name):
    return CASES[name].get("model", HEADLINE)


@functools.lru_cache(maxsize=None)
def setup(name):
    """What a case fixes before any draw: dict(x, y, theta [C, P], steps [C], temps [C] or None, prior (mu, sigma), tables
    [G, P], index [C] int or None, products, factors), every float array f64 holding f32 values."""
    case, model = CASES[name], model_of(name)
    rng = np.random.default_rng([len(name), sum(name.encode()), 43])
    spec = orc.Spec(model["dims"], model["acts"], model["lik"])
    P, N = spec.P, case["N"]
    xs, lab = fc.iris()
    x = f32(xs[:N])
    y = np.eye(3)[lab[:N]] if model["lik"] == orc.LIK_CE else (lab[:N] > 0).astype(np.float64)[:, None]
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
    factors = case.get("factors", FACTORS)
    rows = tables[index] if index is not None else np.broadcast_to(tables[0], (C, P))
    limit = 2.0 / (rows / prior[1]).max(axis=1)
    banded = case.get("banded", BANDED)
    far = BAND_AMPLITUDE * (rows > BAND_SCALE) * banded[:, None] * np.sign(rng.standard_normal((C, P)))
    theta = f32(prior[0] + prior[1] * (0.5 * rng.standard_normal((C, P)) + far))
    return dict(x=x, y=y, theta=theta, steps=f32(limit * factors), temps=temps, prior=prior, tables=tables, index=index,
                products=case.get("products", "bf16x3"), factors=factors, P=P)


def chain_functions(name):
    """One f(theta) -> (target, grad) per chain in f64 (the chain's temperature inside)."""
    d, model = setup(name), model_of(name)
    spec = orc.Spec(model["dims"], model["acts"], model["lik"], mu=d["prior"][0], sigma=d["prior"][1])

    def f(th, t):
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


def restate_draw(name, theta, t, g, v0, u):
    """One draw of the C chains by the restatement from (theta, t, g) with the tables v0 [C, P], u [C, S]."""
    d, fs = setup(name), chain_functions(name)
    outs = []
    for c in range(C):
        mul, tmul = nr.metric_ops("diag", scales(name, c))
        outs.append(nr.nuts_draw(fs[c], theta[c], t[c], g[c], v0[c], u[c], d["steps"][c], MAX_DEPTH, mul, tmul))
    return {k: np.array([o[k] for o in outs]) for k in outs[0]}


@functools.lru_cache(maxsize=None)
def restate(name):
    """The conditioned tables and the DRAWS draws of a case: (v0 [DRAWS, C, P], u [DRAWS, C, S], outs), outs a list of dicts
    over the chains -- start_theta / start_target / start_grad (the f32 state a draw starts from and the oracle's values
    there), the ``nuts_draw`` outputs, and tries (the attempts each pair took)."""
    d, fs = setup(name), chain_functions(name)
    P = d["P"]
    rng = np.random.default_rng([len(name), sum(name.encode()), 47])
    v0, u = np.empty((DRAWS, C, P)), np.empty((DRAWS, C, S))
    th = d["theta"].copy()
    outs = []
    for k in range(DRAWS):
        t, g = evaluate(name, th)
        rows = []
        tries = np.zeros(C, int)
        for c in range(C):
            mul, tmul = nr.metric_ops("diag", scales(name, c))
            for attempt in range(MAX_TRIES):
                v0[k, c], u[k, c] = f32(rng.standard_normal(P)), f32(rng.random(S))
                o = nr.nuts_draw(fs[c], th[c], t[c], g[c], v0[k, c], u[k, c], d["steps"][c], MAX_DEPTH, mul, tmul)
                if o["margin"] > MARGIN_FLOOR:
                    break
            else:
                raise AssertionError(f"{name}: no draw of chain {c}, draw {k} cleared the margin in {MAX_TRIES} attempts")
            tries[c] = attempt + 1
            rows.append(o)
        o = {key: np.array([r[key] for r in rows]) for key in rows[0]}
        o.update(start_theta=th.copy(), start_target=t, start_grad=g, tries=tries)
        outs.append(o)
        th = f32(o["theta"])   # the next draw starts from this state as the device holds it
    return v0, u, outs


def coverage(name):
    """(depths seen, stops seen, moved pairs, unmoved pairs, smallest margin, attempts per pair) of a case."""
    _, _, outs = restate(name)
    depth = np.concatenate([o["depth"] for o in outs])
    stop = np.concatenate([o["stop"] for o in outs])
    acc = np.concatenate([o["accepted"] for o in outs])
    margin = np.concatenate([o["margin"] for o in outs])
    tries = np.concatenate([o["tries"] for o in outs])
    return (sorted(set(depth.tolist())), sorted(set(stop.tolist())), int(acc.sum()), int((acc == 0).sum()), float(margin.min()),
            float(tries.mean()))
