"""The parity cases of elliptical slice sampling (tests/test_eslice_gpu.py runs them on the device, tests/test_eslice_host.py
holds their inputs to the coverage and margin rules on the CPU).  TEST INFRASTRUCTURE ONLY, numpy only.

A case is a target, a Gaussian base (the plan's Normal prior, or tables of its own), C = 11 chains and four consecutive
draws with explicit z and u; nothing is tuned, there being nothing to tune.  The targets: MLP(2-2-1) on XOR (the
register-resident evaluation), the linear-Gaussian plan of dims [12, 1] on 70 rows of tests/invariance.py (the LDS tile
loop: one full row tile and a partial one), the same under a temperature per chain, the P = 2 mixture and a 70-parameter
normal with a base (two coordinates per lane, a partial second pass), XOR under a Laplace prior with a base, MLP dims
[128, 1] on four rows (P = 129), and the mixture again with max_shrinks = 2, where some chains exhaust the bracket and stay."""
import functools

import numpy as np

from tests import eslice_restatement as er
from tests import invariance as iv

C, DRAWS = 11, 4
MARGIN = 1e-9            # a draw with a decision closer than this is set aside
MAX_UNDER = 0.05         # ... and at most this share of (chain, draw) pairs may be
XOR_X = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
XOR_Y = np.array([[0.0], [1.0], [1.0], [0.0]])
XOR_DIMS, XOR_ACTS, XOR_LIK = [2, 2, 1], [1, 1], 0   # sigmoid, sigmoid, BCE sum
CASES = {
    "xor": dict(kind="mlp", dims=XOR_DIMS, acts=XOR_ACTS),
    "lin12": dict(kind="lin"),
    "lin12/temp": dict(kind="lin", temp=True),
    "mix2/base": dict(kind="mix", target="mix2_2", base=True),
    "mvn70/base": dict(kind="mvn", P=70, base=True),
    "xor/laplace/base": dict(kind="mlp", dims=XOR_DIMS, acts=XOR_ACTS, laplace=True, base=True),
    "mlp129": dict(kind="mlp", dims=[128, 1], acts=[1]),
    "mix2/base/shrinks2": dict(kind="mix", target="mix2_2", base=True, max_shrinks=2),
}
LIN = "lin12"


@functools.lru_cache(maxsize=None)
def mvn(P):
    rng = np.random.default_rng([P, 19])
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    cov = A @ A.T + 0.5 * np.eye(P)
    return iv.Target([1.0], rng.standard_normal((1, P)), ((cov + cov.T) / 2)[None])


@functools.lru_cache(maxsize=None)
def mlp_data(name):
    """(x, y) of an MLP case: XOR, or four rows of 128 features with 0 / 1 responses."""
    dims = CASES[name]["dims"]
    if dims == XOR_DIMS:
        return XOR_X, XOR_Y
    rng = np.random.default_rng([dims[0], 23])
    return rng.standard_normal((4, dims[0])) / np.sqrt(dims[0]), np.array([[0.0], [1.0], [1.0], [0.0]])


@functools.lru_cache(maxsize=None)
def lin_data(name=LIN):
    """(D, N, x, y) of a linear-Gaussian plan of tests/invariance.py: a name of its LINEAR table, or (D, N) itself."""
    D, N = iv.LINEAR[name] if isinstance(name, str) else name
    return (D, N) + iv.linear_gaussian(D, N)[:2]


def lin_parts(theta, temp=None, name=LIN):
    """(lik, prior) of a linear-Gaussian plan at theta [..., P], term by term as the plan adds them up, times temp."""
    D, N, x, y = lin_data(name)
    s, sg = iv.LIK_SCALE, iv.PRIOR_SIGMA
    out = theta[..., :D] @ x.T + theta[..., D:D + 1]
    lik = np.sum(-0.5 * ((y[:, 0] - out) / s) ** 2, -1) - N * np.log(s * np.sqrt(2 * np.pi))
    prior = np.sum(-0.5 * (theta / sg) ** 2, -1) - (D + 1) * np.log(sg * np.sqrt(2 * np.pi))
    t = 1.0 if temp is None else temp
    return lik * t, prior * t


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(theta [C, P], z [DRAWS, C, P], u [DRAWS, C, S], temps [C] or None, max_shrinks, prior (mu, sigma) or the Laplace
    tables (loc, b), base (m, s) or None)."""
    case = CASES[name]
    rng = np.random.default_rng([len(name), sum(name.encode()), 31])
    temps = 0.4 + 0.6 * rng.random(C) if case.get("temp") else None
    d = dict(temps=temps, max_shrinks=case.get("max_shrinks", er.MAX_SHRINKS), base=None, prior=None)
    if case["kind"] == "lin":
        tgt = iv.target_of(LIN)
        P = tgt.P
        theta = iv.exact_draws(tgt, C, rng)
        d["prior"] = (np.zeros(P), np.full(P, iv.PRIOR_SIGMA))
    elif case["kind"] == "mlp":
        from oracle import mlp_oracle as orc
        P = orc.Spec(case["dims"], case["acts"], XOR_LIK).P
        theta = 0.5 * rng.standard_normal((C, P))
        if case.get("laplace"):
            d["prior"] = (0.2 * rng.standard_normal(P), 0.5 + rng.random(P))
            d["base"] = (d["prior"][0] + 0.1, np.sqrt(2.0) * d["prior"][1])   # the prior's variance, a shifted centre
        else:
            d["prior"] = (np.zeros(P), np.ones(P))
    else:
        tgt = iv.target_of(case["target"]) if case["kind"] == "mix" else mvn(case["P"])
        P = tgt.P
        theta = iv.exact_draws(tgt, C, rng)
        mean = tgt.probs @ tgt.means
        var = np.einsum("k,kii->i", tgt.probs, tgt.covs) + tgt.probs @ (tgt.means - mean) ** 2
        d["base"] = (mean + 0.1, 1.5 * np.sqrt(var) * (0.8 + 0.4 * rng.random(P)))   # wider than the target, off centre
    d.update(theta=theta, z=rng.standard_normal((DRAWS, C, P)), u=rng.random((DRAWS, C, er.words())))
    return d


def chain_functions(name, mutant=None):
    """(fs, m, s): one point-wise f(theta) -> (ell, target) per chain (the chain's temperature inside), the base's location
    [P] and its scale [C, P]."""
    case, d = CASES[name], inputs(name)
    temps = d["temps"]
    if case["kind"] == "lin":
        parts = [functools.partial(lin_parts, temp=None if temps is None else temps[c]) for c in range(C)]
    elif case["kind"] == "mlp":
        from oracle import mlp_oracle as orc
        x, y = mlp_data(name)
        spec = orc.Spec(case["dims"], case["acts"], XOR_LIK)
        loc, scale = d["prior"]

        def mlp_parts(th):
            th = np.asarray(th, np.float64)
            lik = float(orc.log_lik(spec, th, x, y, None))
            if case.get("laplace"):
                return lik, float(np.sum(-np.abs(th - loc) / scale - np.log(2.0 * scale)))
            return lik, float(orc.log_prior(spec, th, None))
        parts = [mlp_parts] * C
    else:
        tgt = iv.target_of(case["target"]) if case["kind"] == "mix" else mvn(case["P"])
        parts = None
    if d["base"] is not None:
        m, s = d["base"]
        if parts is not None:
            fs = [er.given_base(lambda th, p=p: sum(p(th)), m, s)[0] for p in parts]
        else:
            fs = [er.given_base(lambda th: float(tgt.value(th[None])[0]), m, s)[0]] * C
        return fs, m, np.broadcast_to(s, (C, len(m)))
    mu, sigma = d["prior"]
    built = [er.prior_base(parts[c], mu, sigma, None if temps is None else temps[c], mutant) for c in range(C)]
    return [b[0] for b in built], mu, np.stack([b[2] for b in built])


def start(name):
    """(theta, ell, target) of the case's first states by the restatement."""
    fs, _, _ = chain_functions(name)
    th = inputs(name)["theta"].copy()
    et = [fs[c](th[c]) for c in range(C)]
    return th, np.array([a for a, _ in et], np.float64), np.array([b for _, b in et], np.float64)


def restate(name, state=None, z=None, u=None, max_shrinks=None):
    """The DRAWS draws of a case by the restatement, each from the state the one before left: a list of ``draw_chains``
    dicts.  ``state`` (theta, ell, target): the values the device starts from; ``z`` / ``u``: other randoms."""
    d = inputs(name)
    fs, m, s = chain_functions(name)
    th, ell, tv = start(name) if state is None else (np.array(a, np.float64) for a in state)
    z = d["z"] if z is None else z
    u = d["u"] if u is None else u
    outs = []
    for k in range(len(z)):
        o = er.draw_chains(fs, th, ell, tv, m, s, z[k], u[k], d["max_shrinks"] if max_shrinks is None else max_shrinks)
        th, ell, tv = o["theta"], o["ell"], o["target"]
        outs.append(o)
    return outs


# ------------------------------------------------------------------------------------------------ the invariance setups
# The base of a mixture target in the invariance tests: the mixture's own mean, and BASE_FACTOR times its standard deviation
# per coordinate.  The factors were picked on the CPU from the restatement alone (tests/test_eslice_host.py holds them to
# it) for a mean of 1.5 to 8 evaluations per draw: a base wider than the target makes the first angle miss more often.
BASE_FACTOR = {"mix2_2": 2.0, "mix5_3": 2.0}
EVALS_BAND = (1.5, 8.0)


def mix_base(target):
    """(m [P], s [P]) of the invariance tests' base for a mixture target of tests/invariance.py."""
    tgt = iv.target_of(target)
    mean = tgt.probs @ tgt.means
    var = np.einsum("k,kii->i", tgt.probs, tgt.covs) + tgt.probs @ (tgt.means - mean) ** 2
    return mean, BASE_FACTOR[target] * np.sqrt(var)


def batch_mix(target):
    """(f, m, s) of ``eslice_restatement.draw_batch`` for a mixture target under its base."""
    tgt = iv.target_of(target)
    m, s = mix_base(target)
    g = er.given_base(tgt.value, m, s)[0]
    return (lambda th, rows: g(th)), m, s


def batch_lin(name, temps=None, mutant=None):
    """(f, m, s) of ``draw_batch`` for a linear-Gaussian plan under its own prior: temps [C] or None; s [C, P] or [P]."""
    P = lin_data(name)[0] + 1
    mu, sigma = np.zeros(P), np.full(P, iv.PRIOR_SIGMA)
    assert mutant in (None,) + er.MUTANTS
    s = sigma if temps is None or mutant == "untempered_scale" else sigma[None] / np.sqrt(temps)[:, None]

    def f(th, rows):
        lik, prior = lin_parts(th, None if temps is None else temps[rows], name)
        return (lik + prior if mutant == "whole_target" else lik), lik + prior
    return f, mu, s


# The targets of tests/test_eslice_invariance_gpu.py: (target of tests/invariance.py, dtype, temperatures, with a base).
INVARIANCE = [("lin3", "f64", None, False), ("lin12", "f32", "halves", False), ("mix2_2", "f64", None, True),
              ("mix5_3", "f32", None, True)]
# Under the plan's own prior nothing can be picked: the mean evaluations per draw is a property of the posterior against
# its N(0, 2^2) prior, and the restatement gives it from exact starts (tests/test_eslice_host.py holds these figures to it
# at 4096 chains; the device test holds the kernel to them).  Both lie above EVALS_BAND, which binds where a base is chosen.
PRIOR_EVALS = {"lin3": 8.82, "lin12": 10.38}
EVALS_TOL = 0.25   # of a mean over >= 4096 x 8 draws whose standard deviation is about 5: more than 8 standard errors


def batch_setup(target, temps, mutant=None):
    """(f, m, s) of ``draw_batch`` for a target of INVARIANCE (or any (D, N) linear-Gaussian plan) with temps [C] or None."""
    if isinstance(target, str) and target.startswith("mix"):
        assert temps is None and mutant is None
        return batch_mix(target)
    return batch_lin(target, temps, mutant)
