"""The parity cases of NUTS with its tree in device memory (tests/test_nuts_tree_gpu.py runs them on the device,
tests/test_nuts_tree_host.py holds their inputs to the coverage and margin rules on the CPU).  TEST INFRASTRUCTURE ONLY, numpy
only.

Two MLPs beyond the 128 parameters of the tree in LDS, under a diagonal metric and the N(0, 1) prior, through the numpy oracle,
built as tests/nuts_cases.inputs builds its XOR case: a step per chain, the prior's stability limit 2 / max(scale) times the
case's factors, from a fraction of it (the draw stops at max_depth) to a hundred times (a divergent draw of depth 0).
  "mlp8-14-1/diag": P = 141, three lane rounds with a last round of 13; six rows of normal inputs, Bernoulli labels.
  "iris4-32-32-3/diag": P = 1315, the model the project exists for, on every 13th row of Iris (4 of each class)."""
import functools
import os

import numpy as np

from tests import nuts_cases as nc
from tests import nuts_restatement as nr

MARGIN, MAX_UNDER = nc.MARGIN, nc.MAX_UNDER
CASES = {
    "mlp8-14-1/diag": dict(dims=[8, 14, 1], acts=[1, 1], lik=0, C=11, draws=4, max_depth=5, factors=nc.FACTORS),
    "iris4-32-32-3/diag": dict(dims=[4, 32, 32, 3], acts=[1, 1, 0], lik=1, C=7, draws=3, max_depth=4,
                               factors=np.array([0.02, 0.2, 0.25, 0.3, 0.35, 0.4, 100.0])),
}
IRIS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eeyore_amd", "data", "iris")


def num_params(name):
    dims = CASES[name]["dims"]
    return sum((a + 1) * b for a, b in zip(dims[:-1], dims[1:]))


@functools.lru_cache(maxsize=None)
def data(name):
    """(X [N, d0], Y [N, dK]) of a case, float64."""
    if name.startswith("iris"):
        X = np.loadtxt(os.path.join(IRIS, "x.csv"), delimiter=",", skiprows=1)[::13]
        y = np.loadtxt(os.path.join(IRIS, "y.csv"), delimiter=",", skiprows=1).astype(int)[::13]
        return X, np.eye(3)[y]
    rng = np.random.default_rng(5)
    X = rng.standard_normal((6, 8))
    return X, (rng.random((6, 1)) < 0.5).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(theta [C, P], v0 [DRAWS, C, P], u [DRAWS, C, S], steps [C], metric ('diag', table))."""
    case = CASES[name]
    P, C, draws = num_params(name), case["C"], case["draws"]
    rng = np.random.default_rng([P, len(name), 29])
    table = 0.5 + rng.random(P)
    theta = 0.5 * rng.standard_normal((C, P))
    v0 = rng.standard_normal((draws, C, P))
    u = rng.random((draws, C, nr.words(case["max_depth"])))
    return dict(theta=theta, v0=v0, u=u, steps=(2.0 / table.max()) * case["factors"], metric=("diag", table))


def value_grad(name):
    from oracle import mlp_oracle as orc
    case = CASES[name]
    spec = orc.Spec(case["dims"], case["acts"], case["lik"])
    X, Y = data(name)

    def f(th):
        t, g = orc.upto_grad_log_target(spec, np.asarray(th, np.float64), X, Y)
        return float(t), g
    return f


def restate(name, start=None):
    """The case's draws by the restatement, each from the state the one before left: a list of ``run_chains`` dicts.
    ``start`` (theta, target, grad): the values the device starts from."""
    case, d, f = CASES[name], inputs(name), value_grad(name)
    if start is None:
        th = d["theta"].copy()
        tg = [f(th[c]) for c in range(case["C"])]
        t, g = np.array([a for a, _ in tg]), np.stack([b for _, b in tg])
    else:
        th, t, g = (np.array(a, np.float64) for a in start)
    outs = []
    for k in range(case["draws"]):
        o = nr.run_chains(f, th, t, g, d["v0"][k], d["u"][k], d["steps"], case["max_depth"], d["metric"])
        th, t, g = o["theta"], o["target"], o["grad"]
        outs.append(o)
    return outs


@functools.lru_cache(maxsize=None)
def restated(name):
    """``restate(name)`` from the oracle's own start, computed once."""
    return restate(name)
