"""The parity cases of elliptical slice sampling on the matrix cores (k_eslice_mfma):
tests/test_eslice_fused_gpu.py runs them on the device, tests/test_eslice_fused_host.py holds their inputs to the margin
rules on the CPU.  TEST INFRASTRUCTURE ONLY, numpy only.

A case is an MLP(4-32-32-dK) plan on standardised iris rows, C = 11 chains and four draws with explicit z and u, restated
by ``eslice_restatement.draw`` on ``oracle.mlp_oracle`` in f64.  Everything the device is given is rounded to f32 BEFORE the
restatement sees it (theta, z, u, the rows, the temperatures, the prior and base tables), and every draw starts from the
restatement's state of the draw before rounded to f32, with ell and the target evaluated afresh there: a device draw that
decides otherwise costs one (chain, draw) pair, not the rest of its chain.

Two margins per draw, kept apart because they live on different scales: the ell-margin, the smallest |ell' - log y| over
the draw's evaluations (ell is a sum over the rows: its f32 error grows with N), and the angle margin, the smallest |a|
where the sign of a is branched on (a is a few operations on uniforms)."""
import functools
import os

import numpy as np

from oracle import mlp_oracle as orc
from tests import eslice_restatement as er

C, DRAWS = 11, 4
PAIRS = C * DRAWS
ELL_MARGIN_MAX = 2e-2    # no tolerance on ell may exceed this ...
ANGLE_MARGIN = 1e-5      # ... a draw with an angle closer to 0 than this is set aside
MAX_UNDER = 0.10         # ... and at most this share of a case's pairs may be set aside at an ell-margin of ELL_MARGIN_MAX
HEADLINE = dict(dims=[4, 32, 32, 3], acts=[1, 1, 0], lik=orc.LIK_CE)
BCE_TANH = dict(dims=[4, 32, 32, 1], acts=[2, 2, 1], lik=orc.LIK_BCE)   # mfma32_kind == 2: the bf16x3 form only
# rows: 5 = one ragged 32-row tile, 33 = a second tile of one row, 150 = five tiles, the last of 22 rows
CASES = {
    "n5": dict(N=5, sigma=1.0),
    "n33": dict(N=33),
    "n150": dict(N=150),
    "n150/temp": dict(N=150, temp=True),
    "n33/prior": dict(N=33, prior="elementwise"),
    "n150/prior/temp": dict(N=150, prior="elementwise", temp=True),
    "n150/base": dict(N=150, base=True),
    "n33/base/temp": dict(N=33, base=True, temp=True),
    "n33/shrinks2": dict(N=33, max_shrinks=2),
    "n150/bce-tanh": dict(N=150, model=BCE_TANH, sigma=1.0),
    "n150/exact": dict(N=150, products="exact"),
}
N150 = [name for name, case in CASES.items() if case["N"] == 150]   # the cases tau is measured on


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def iris():
    """(x [150, 4] standardised, labels [150]) of eeyore_amd/data/iris, in a fixed shuffled order (the file is sorted by
    species: its first rows would all be of one class)."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eeyore_amd", "data", "iris")
    x = np.loadtxt(os.path.join(root, "x.csv"), delimiter=",", skiprows=1)
    lab = np.loadtxt(os.path.join(root, "y.csv"), delimiter=",", skiprows=1).astype(int)
    x = (x - x.mean(0)) / x.std(0)
    order = np.random.default_rng(150).permutation(len(x))
    return x[order], lab[order]


def model_of(name):
    return CASES[name].get("model", HEADLINE)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x [N, 4], y [N, dK], theta [C, P], z [DRAWS, C, P], u [DRAWS, C, S], temps [C] or None, max_shrinks,
    prior (mu [P], sigma [P]), base (m, s) or None, products), every array f64 holding f32 values."""
    case, model = CASES[name], model_of(name)
    rng = np.random.default_rng([len(name), sum(name.encode()), 41])
    spec = orc.Spec(model["dims"], model["acts"], model["lik"])
    P, N = spec.P, case["N"]
    xs, lab = iris()
    x = f32(xs[:N])
    y = np.eye(3)[lab[:N]] if model["lik"] == orc.LIK_CE else (lab[:N] > 0).astype(np.float64)[:, None]
    if case.get("prior") == "elementwise":
        prior = (f32(0.1 * rng.standard_normal(P)), f32(0.8 + 1.2 * rng.random(P)))
    else:
        prior = (np.zeros(P), f32(np.full(P, case.get("sigma", np.sqrt(3.0)))))
    base = (f32(prior[0] + 0.1), f32(1.25 * prior[1])) if case.get("base") else None   # off the prior's centre, wider
    temps = f32(0.4 + 0.6 * rng.random(C)) if case.get("temp") else None
    scale = 0.3 + 0.2 * rng.random((C, 1))
    return dict(x=x, y=y, theta=f32(prior[0] + scale * rng.standard_normal((C, P))), z=f32(rng.standard_normal((DRAWS, C, P))),
                u=f32(rng.random((DRAWS, C, er.words()))), temps=temps, max_shrinks=case.get("max_shrinks", er.MAX_SHRINKS),
                prior=prior, base=base, products=case.get("products", "bf16x3"))


def chain_functions(name):
    """(fs, m, s): one f(theta) -> (ell, target) per chain in f64 (the chain's temperature inside), the base's location [P]
    and its scale [C, P]."""
    d, model = inputs(name), model_of(name)
    mu, sigma = d["prior"]
    spec = orc.Spec(model["dims"], model["acts"], model["lik"], mu=mu, sigma=sigma)
    temps = d["temps"]

    def parts(th, t):
        th = np.asarray(th, np.float64)
        return float(orc.log_lik(spec, th, d["x"], d["y"], t)), float(orc.log_prior(spec, th, t))
    per_chain = [functools.partial(parts, t=None if temps is None else float(temps[c])) for c in range(C)]
    if d["base"] is not None:
        m, s = d["base"]
        return [er.given_base(lambda th, p=p: sum(p(th)), m, s)[0] for p in per_chain], m, np.broadcast_to(s, (C, len(m)))
    built = [er.prior_base(per_chain[c], mu, sigma, None if temps is None else float(temps[c])) for c in range(C)]
    return [b[0] for b in built], mu, np.stack([b[2] for b in built])


def angle_margin(u, n_evals, exhausted):
    """The smallest |a| over the shrinks a draw of n_evals evaluations made (every evaluation but the last is followed by
    one; so is the last of a draw that did not exhaust its bracket and did not move -- there is none such)."""
    a = u[1]
    lo, hi, margin = a - 1.0, a, np.inf
    for k in range(n_evals - 1):
        margin = min(margin, abs(a))
        if a < 0:
            lo = a
        else:
            hi = a
        a = lo + (hi - lo) * u[2 + k]
    return margin


@functools.lru_cache(maxsize=None)
def restate(name):
    """The DRAWS draws of a case: a list of dicts over the chains -- start (theta, ell, target: the f32 state a draw starts
    from and the restatement's values there), the ``draw`` outputs (theta, ell, target, accepted, n_evals), ell_margin,
    angle_margin, and points / point_ells (every point the draw evaluated, and ell there)."""
    d = inputs(name)
    fs, m, s = chain_functions(name)
    th = d["theta"].copy()
    outs = []
    for k in range(DRAWS):
        o = dict(start_theta=th.copy(), start_ell=np.empty(C), start_target=np.empty(C), theta=np.empty_like(th), ell=np.empty(C),
                 target=np.empty(C), accepted=np.zeros(C, bool), n_evals=np.zeros(C, int), ell_margin=np.empty(C),
                 angle_margin=np.empty(C), points=[], point_ells=[], point_chain=[])
        for c in range(C):
            ell, tv = fs[c](th[c])
            seen = []

            def f(p, c=c, seen=seen):
                e, t = fs[c](p)
                seen.append((np.array(p), e))
                return e, t
            r = er.draw(f, th[c], ell, tv, m, s[c], d["z"][k, c], d["u"][k, c], d["max_shrinks"])
            with np.errstate(divide="ignore"):
                logy = ell + np.log(d["u"][k, c, 0])
            o["start_ell"][c], o["start_target"][c] = ell, tv
            for key in ("theta", "ell", "target", "accepted", "n_evals"):
                o[key][c] = r[key]
            o["ell_margin"][c] = min(abs(e - logy) for _, e in seen)
            o["angle_margin"][c] = angle_margin(d["u"][k, c], r["n_evals"], r["exhausted"])
            assert min(o["ell_margin"][c], o["angle_margin"][c]) == r["margin"]
            o["points"] += [p for p, _ in seen]
            o["point_ells"] += [e for _, e in seen]
            o["point_chain"] += [c] * len(seen)
        outs.append(o)
        th = f32(o["theta"])   # the next draw starts from this state as the device holds it
    return outs


def decided(o, tau):
    """The chains of one draw whose decisions a device within tau of the restatement's ell must reproduce."""
    return (o["ell_margin"] > tau) & (o["angle_margin"] > ANGLE_MARGIN)


def summary(name, tau=ELL_MARGIN_MAX):
    """(pairs set aside at an ell-margin of tau, pairs that stayed, mean evaluations per draw) of a case."""
    outs = restate(name)
    under = sum(int((~decided(o, tau)).sum()) for o in outs)
    stayed = sum(int((~o["accepted"]).sum()) for o in outs)
    return under, stayed, float(np.mean([o["n_evals"].mean() for o in outs]))
