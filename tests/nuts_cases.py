"""The parity cases of NUTS (tests/test_nuts_gpu.py runs them on the device, tests/test_nuts_host.py holds their inputs to
the coverage and margin rules on the CPU).  TEST INFRASTRUCTURE ONLY, numpy only.

A case is a target (one multivariate normal as a tests.invariance.Target, or MLP(2-2-1) on XOR through the numpy oracle), a
metric form and C = 11 chains with a step each.  The steps are the case's stability limit 2 / sqrt(lambda_max(L^T Prec L))
(MLP: of the prior alone, 2) times FACTORS, which run from a fiftieth of it -- 31 leapfrog steps then never turn, the draw
stops at max_depth -- through the range in which trees of every depth end by the U-turn criterion, to a hundred times the
limit, where the first leaf's energy error is beyond 1000: a divergent draw of depth 0."""
import functools

import numpy as np

from tests import invariance as iv
from tests import nuts_restatement as nr

C, DRAWS, MAX_DEPTH = 11, 4, 5
MARGIN = 1e-9            # a draw with a decision closer than this is set aside
MAX_UNDER = 0.05         # ... and at most this share of (chain, draw) pairs may be
FACTORS = np.array([0.02, 0.04, 0.07, 0.12, 0.2, 0.3, 0.45, 0.65, 0.9, 1.2, 100.0])
CASES = {
    "mvn2/dense": dict(P=2, kind="dense"),
    "mvn5/dense": dict(P=5, kind="dense"),
    "mvn5/dense/temp": dict(P=5, kind="dense", temp=True),
    "mvn70/dense": dict(P=70, kind="dense"),
    "mvn70/diag": dict(P=70, kind="diag"),
    "mvn128/diag": dict(P=128, kind="diag"),
    "xor/diag": dict(P=9, kind="diag", mlp=True),
}
XOR_X = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
XOR_Y = np.array([[0.0], [1.0], [1.0], [0.0]])
XOR_DIMS, XOR_ACTS, XOR_LIK = [2, 2, 1], [1, 1], 0   # sigmoid, sigmoid, BCE sum; prior N(0, 1)


@functools.lru_cache(maxsize=None)
def target(name):
    """The Target of a normal case: mean and covariance from the case's own generator."""
    P = CASES[name]["P"]
    rng = np.random.default_rng([P, 17])
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    cov = A @ A.T + 0.5 * np.eye(P)
    return iv.Target([1.0], rng.standard_normal((1, P)), ((cov + cov.T) / 2)[None])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(theta [C, P], v0 [DRAWS, C, P], u [DRAWS, C, S], steps [C], metric (kind, table), temps [C] or None)."""
    case = CASES[name]
    P, kind = case["P"], case["kind"]
    rng = np.random.default_rng([P, len(name), 29])
    table = iv.factors(1, P, rng, 1.0)[0] if kind == "dense" else 0.5 + rng.random(P)
    temps = 0.5 + 0.5 * rng.random(C) if case.get("temp") else None
    if case.get("mlp"):
        theta, limit = 0.5 * rng.standard_normal((C, P)), 2.0 / table.max()
    else:
        tgt = target(name)
        theta = iv.exact_draws(tgt, C, rng)
        mul, tmul = nr.metric_ops(kind, table)
        M = np.stack([tmul(tgt.prec[0] @ mul(e)) for e in np.eye(P)])
        limit = 2.0 / np.sqrt(np.linalg.eigvalsh((M + M.T) / 2).max())
    return dict(theta=theta, v0=rng.standard_normal((DRAWS, C, P)), u=rng.random((DRAWS, C, nr.words(MAX_DEPTH))),
                steps=limit * FACTORS, metric=(kind, table), temps=temps)


def value_grads(name):
    """One point-wise (value, gradient) function per chain (the chain's temperature inside)."""
    temps = inputs(name)["temps"]
    if CASES[name].get("mlp"):
        from oracle import mlp_oracle as orc
        spec = orc.Spec(XOR_DIMS, XOR_ACTS, XOR_LIK)

        def f(th):
            t, g = orc.upto_grad_log_target(spec, np.asarray(th, np.float64), XOR_X, XOR_Y)
            return float(t), g
        return [f] * C
    tgt = target(name)
    return [nr.point_value_grad(tgt, None if temps is None else temps[c]) for c in range(C)]


def restate(name, start=None, v0=None, u=None, max_depth=MAX_DEPTH):
    """The DRAWS draws of a case by the restatement, each from the state the one before left: a list of ``run_chains``
    dicts.  ``start`` (theta, target, grad): the values the device starts from; ``v0`` / ``u``: other randoms."""
    d = inputs(name)
    fs = value_grads(name)
    if start is None:
        th = d["theta"].copy()
        tg = [fs[c](th[c]) for c in range(C)]
        t, g = np.array([a for a, _ in tg]), np.stack([b for _, b in tg])
    else:
        th, t, g = (np.array(a, np.float64) for a in start)
    v0 = d["v0"] if v0 is None else v0
    u = d["u"] if u is None else u
    outs = []
    for k in range(len(v0)):
        o = nr.run_chains(fs, th, t, g, v0[k], u[k], d["steps"], max_depth, d["metric"])
        th, t, g = o["theta"], o["target"], o["grad"]
        outs.append(o)
    return outs
