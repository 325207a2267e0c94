"""HMC under a metric, NUTS and elliptical slice sampling under every prior family, every likelihood and every evaluation
path of eval_target: the case builder of tests/test_cross_metric_gpu.py (the device) and tests/test_cross_metric_host.py
(the conditions on the table), beside tests/cross_restatement.py, whose shapes, families, losses, rows and targets it
uses.  TEST INFRASTRUCTURE ONLY, numpy only, needs no GPU.

A case is (sampler, family, loss, shape, dtype, tempered) with C = 11 chains and three consecutive draws from given
randoms.  What the tuple does not say is cycled over the cases and kept in EXTRA: the layout of the metric table (one for
all chains, one per chain, G = 3 entries named by an int32 index), whether elliptical slice sampling takes the plan's
Normal prior as its Gaussian or tables of its own, and the one case per shape with max_shrinks = 2.

The restatements are tests/nuts_restatement.py (``run_chains``), tests/hmc_metric_restatement.py (``hmc_metric_draw``)
and tests/eslice_restatement.py (``draw_chains`` under ``prior_base`` / ``given_base``), on per-chain point functions of
the case's targets with the chain's temperature inside.  ``advance`` is one draw of every chain from a given state,
``restate`` the loop over the draws, written once.  A BCE case of dtype 'f32' is restated with what f32 makes of the naive
BCE sum near a saturated sigmoid (``Saturation``).  ``set_aside`` is the rule by which a comparison leaves a draw out; the
host file states it and holds every case to its cap."""
import numpy as np

from tests import cross_restatement as cr
from tests import eslice_restatement as er
from tests import nuts_restatement as nr
from tests import prior_restatement as pr
from tests.hmc_metric_restatement import DIAG, TRIL, hmc_metric_draw

SAMPLERS = ("hmc_metric/diag", "hmc_metric/dense", "nuts/diag", "nuts/dense", "eslice")
GRADIENT_SAMPLERS = SAMPLERS[:4]
LAYOUTS = ("shared", "per_chain", "indexed")
C, DRAWS, G = 11, 3, 3
MAX_DEPTH = {"f64": 4, "f32": 3}
NUM_STEPS = 3
# the step of a chain is the shape's HMC step (cr.PAR, cr.TUNE) times its factor.  NUTS: from a quarter of it, where 15
# leapfrog steps do not turn, through the range in which trees end by the U-turn criterion, to 30 times it, where the
# first leaf's energy error is beyond 1000.  hmc_metric: around it, so that three steps both accept and reject.
NUTS_FACTORS = np.array([0.25, 0.6, 1.0, 1.5, 2.2, 3.2, 4.5, 6.5, 9.0, 13.0, 30.0])
HMC_FACTORS = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75, 3.0])
MARGIN = 1e-9              # f64: a (chain, draw) pair with a decision closer than this is set aside
F32_DECISION_TOL = 2e-3    # f32: the project's (tests/test_gpu_parity.py)
MAX_UNDER = {"f64": 0.05, "f32": 0.20}   # the share of pairs of a case that may be set aside (f64: tests/nuts_cases.py's)
OUTCOME = {"hmc_metric": ("accepted",), "nuts": nr.OUTCOME, "eslice": ("accepted", "n_evals")}


def _cases():
    """The table, built as tests/test_cross_gpu.py builds STEP_CASES: every sampler on every shape in both dtypes, three
    cases per cell (two on 'bce'), the family, the likelihood and the tempering cycled with periods that share no factor.
    Returns (cases, extra)."""
    out, extra = [], {}
    for si, s in enumerate(SAMPLERS):
        n = normals = 0
        for hi, (shape, sh) in enumerate(cr.SHAPES.items()):
            for dt in ("f64", "f32"):
                for j in range(2 if shape == "bce" else 3):
                    fam = cr.FAMILIES[(n + si) % 4]
                    loss = sh["losses"][(n + n // 4 + si) % len(sh["losses"])]
                    case = (s, fam, loss, shape, dt, bool((n + n // 4 + n // 20) % 2))
                    ex = dict(n=n, layout=LAYOUTS[(n + si) % 3])
                    if s == "eslice":
                        ex["own_base"] = fam != "normal" or bool(normals % 2)
                        normals += fam == "normal"
                        ex["max_shrinks"] = 2 if (j == 1 and dt == ("f64", "f32")[hi % 2]) else er.MAX_SHRINKS
                    out.append(case)
                    extra[case] = ex
                    n += 1
    return out, extra


CASES, EXTRA = _cases()


def case_id(case):
    s, fam, loss, shape, dt, temp = case
    return f"{s}-{fam}-{loss}-{shape}-{dt}-{'temp' if temp else 'plain'}"


# the seed of a case's inputs where 0 does not meet the conditions tests/test_cross_metric_host.py states (the set-aside
# caps and the variety of outcomes), found on the CPU from the restatement alone
SEEDS = {
    'hmc_metric/dense-cauchy-bce-bce-f32-plain': 2, 'nuts/diag-laplace-bce-bce-f32-temp': 1, 'nuts/diag-laplace-gauss-fix-f32-temp': 1,
    'nuts/diag-normal-laplace-dyn-f32-plain': 1, 'nuts/diag-cauchy-ce-lds1-f32-temp': 2,
    'nuts/diag-laplace-laplace-lds1-f32-temp': 2, 'nuts/diag-studentt-ce-lds3-f64-temp': 5,
    'nuts/diag-laplace-poisson-lds3-f32-plain': 1, 'nuts/diag-cauchy-laplace-lds3-f32-temp': 1,
    'nuts/dense-cauchy-poisson-fix-f64-plain': 1, 'nuts/dense-laplace-gauss-fix-f64-plain': 5,
    'nuts/dense-studentt-laplace-fix-f32-temp': 1, 'nuts/dense-cauchy-ce-fix-f32-temp': 2,
    'nuts/dense-normal-gauss-fix-f32-plain': 9, 'nuts/dense-studentt-ce-dyn-f32-temp': 1,
    'nuts/dense-normal-ce-dyn128-f32-temp': 1, 'nuts/dense-studentt-laplace-lds1-f64-temp': 5,
    'nuts/dense-cauchy-gauss-lds3-f64-temp': 1, 'nuts/dense-normal-laplace-lds3-f64-plain': 3,
    'nuts/dense-studentt-ce-lds3-f32-plain': 18, 'nuts/dense-cauchy-laplace-lds3-f32-plain': 17,
    'nuts/dense-normal-poisson-lds3-f32-temp': 9, 'eslice-studentt-ce-dyn-f32-plain': 2,
    'eslice-laplace-ce-dyn128-f64-plain': 1, 'eslice-studentt-poisson-lds1-f32-plain': 17,
    'eslice-laplace-poisson-lds3-f64-plain': 8, 'eslice-normal-poisson-lds3-f32-plain': 1,
}


def _rounded(a, round_to):
    return a if round_to is None or a is None else np.asarray(a).astype(round_to).astype(np.float64)


def _pick(factors, n):
    """n of the eleven factors, the first and the last among them (all of them at n = 11)."""
    return factors[np.round(np.linspace(0, len(factors) - 1, n)).astype(int)]


class Saturation:
    """What f32 makes of the naive BCE sum (log(o) y + log(1 - o) (1 - y), NaN once a sigmoid saturates: the reference's
    own form) where the f64 restatement still holds a number.  The f32 sigmoid 1 / (1 + exp(-g)) is exactly 1 once
    exp(-g) <= 2^-25, and the term is then NaN whatever y is; short of that, 1 - o carries a relative error of
    2^-24 / (1 - o), which is beyond the decision tolerance 2e-3 once 1 - o < 3e-5.  ``look`` says whether the target at a
    point is NaN in f32, and notes in ``band`` a point in the range between, where f32's value is a number but not one a
    decision can be held to: ``advance`` sets such a draw aside.  One per chain of a BCE case of dtype 'f32'."""
    NAN_BELOW, BAND_BELOW = 2.0 ** -25, 3e-5

    def __init__(self, tgt):
        self.tgt, self.band = tgt, False

    def look(self, th):
        import torch
        with torch.no_grad():
            o = self.tgt.forward(torch.as_tensor(np.asarray(th, np.float64), dtype=torch.float64)).numpy()
        gap = float((1.0 - o).min())
        if 0.5 * self.NAN_BELOW < gap < self.BAND_BELOW or not gap == gap:
            self.band = True
        return gap <= self.NAN_BELOW or float(o.min()) < 1e-37


def _lik_prior(tgt, guard=None):
    """parts(theta) -> (lik, prior) of a Target, both tempered, without the gradient."""
    import torch

    def parts(th):
        with torch.no_grad():
            t = torch.as_tensor(np.asarray(th, np.float64), dtype=torch.float64)
            lik = float("nan") if guard is not None and guard.look(th) else float(tgt.log_lik_t(t))
            return lik, float(tgt.log_prior_t(t))
    return parts


def _log_target(tgt, guard=None):
    def f(th):
        return float("nan") if guard is not None and guard.look(th) else tgt.log_target(th)
    return f


def _value_grad(tgt, guard=None):
    """value_and_grad of a Target; NaN where a trajectory has left the finite numbers (torch.distributions refuses such
    a point, the device evaluates it to NaN: an energy error that is not a number ends the tree as divergent)."""
    def f(th):
        if not np.isfinite(th).all() or (guard is not None and guard.look(th)):
            return float("nan"), np.full(len(th), np.nan)
        return tgt.value_and_grad(th)
    return f


def _start_points(kind, rng, C, P, loc, scale):
    """The gradient samplers start where tests/cross_restatement.py's cases do, at 0.3 N(0, 1).  Elliptical slice sampling
    starts at draws of N(loc, scale^2), the prior's tables: from there the first angle is often accepted and the later draws
    of the chain shrink the bracket, so a case holds draws of one evaluation and of many, and the likelihood differs between
    the points of an ellipse by the order of its own size, which keeps most f32 decisions clear of their margin."""
    e = rng.standard_normal((C, P))
    return loc + scale * e if kind == "eslice" else 0.3 * e


def build(case, seed=None, C=C, draws=DRAWS, extra=None):
    """The inputs of ``draws`` draws of C chains of a case, without the restatement's results: the rows, the prior's
    tables, the targets (one per chain where tempered), the start, the randoms, and per sampler the metric table with its
    layout and index, the steps, or the base and max_shrinks.  A case of dtype 'f32' has everything the device will hold
    rounded to f32.  ``extra`` stands in for EXTRA[case] (a case outside the table)."""
    s, fam, loss, shape, dt, temp = case
    kind, _, form = s.partition("/")
    ex = dict(EXTRA[case] if extra is None else extra)
    seed = SEEDS.get(case_id(case), 0) if seed is None else seed
    round_to = np.float32 if dt == "f32" else None
    sh = cr.SHAPES[shape]
    dims, acts, N = sh["dims"], sh["acts"], sh["N"]
    P = cr.num_params(dims)
    x, y = (_rounded(a, round_to) for a in cr.rows_for(dims, loss, N, seed=20 + seed))
    loc, scale, df = (_rounded(a, round_to) for a in pr.distinct_tables(P, 100 + seed))
    prior = pr.make_prior(fam, loc, scale, df)
    rng = np.random.default_rng([12000, seed, SAMPLERS.index(s), ex["n"]])
    d = dict(case=case, sampler=s, kind=kind, form=form, family=fam, loss=loss, shape=shape, dtype=dt, dims=dims, acts=acts,
             x=x, y=y, loc=loc, scale=scale, df=df if fam == "studentt" else None, P=P, C=C, draws=draws,
             th0=_rounded(_start_points(kind, rng, C, P, loc, scale), round_to),
             z=_rounded(rng.standard_normal((draws, C, P)), round_to))
    d["temps"] = _rounded(0.3 + 0.7 * rng.random(C), round_to) if temp else None
    d["targets"] = [cr.make_target(dims, acts, loss, x, y, prior, temperature=None if not temp else float(d["temps"][c]))
                    for c in range(C if temp else 1)] * (1 if temp else C)
    d["guards"] = [Saturation(t) for t in d["targets"]] if loss == "bce" and dt == "f32" else [None] * C
    d["fs"] = [_value_grad(t, g) for t, g in zip(d["targets"], d["guards"])]
    base = cr.par_of("hmc", shape, loss)["step"]
    if kind == "eslice":
        d["max_shrinks"] = ex["max_shrinks"]
        d["u"] = _rounded(rng.random((draws, C, er.words())), round_to)
        d["base"] = None
        if ex["own_base"]:
            d["base"] = (loc, _rounded(scale * (0.7 + 0.7 * rng.random(P)), round_to))
        return d
    d["layout"] = ex["layout"]
    entries = {"shared": 1, "per_chain": C, "indexed": G}[d["layout"]]
    if form == "diag":
        table = 0.5 + rng.random((entries, P))
    else:
        table = np.stack([np.tril(pr.dense_lower(P, 1.0, 1000 * seed + 10 * ex["n"] + g)) for g in range(entries)])
    d["table"] = _rounded(table, round_to)          # [entries, P] or [entries, P, P]; the device takes [0] where shared
    d["index"] = rng.integers(0, G, C).astype(np.int32) if d["layout"] == "indexed" else None
    if kind == "nuts":
        d["max_depth"] = MAX_DEPTH[dt]
        d["steps"] = _rounded(base * _pick(NUTS_FACTORS, C), round_to)
        d["u"] = _rounded(rng.random((draws, C, nr.words(d["max_depth"]))), round_to)
    else:
        d["num_steps"] = NUM_STEPS
        d["steps"] = _rounded(base * _pick(HMC_FACTORS, C), round_to)
        d["u"] = _rounded(rng.random((draws, C)), round_to)
    return d


def entry_of(d, c):
    """The metric table entry of chain c."""
    return d["table"][0 if d["layout"] == "shared" else c if d["layout"] == "per_chain" else d["index"][c]]


def eslice_functions(d):
    """(fs, m, s): per chain f(theta) -> (ell, target), the base's location [P] and its scale [C, P]."""
    C = d["C"]
    temps = d["temps"]
    if d["base"] is not None:
        m, s = d["base"]
        fs = [er.given_base(_log_target(t, g), m, s)[0] for t, g in zip(d["targets"], d["guards"])]
        return fs, m, np.broadcast_to(s, (C, len(m)))
    built = [er.prior_base(_lik_prior(d["targets"][c], d["guards"][c]), d["loc"], d["scale"],
                           None if temps is None else temps[c])
             for c in range(C)]
    return [b[0] for b in built], d["loc"], np.stack([b[2] for b in built])


def start(d):
    """The state the chains start from by the restatement: dict(theta, target, grad) or, for eslice, dict(theta, target,
    ell)."""
    th = d["th0"].copy()
    if d["kind"] == "eslice":
        fs, _, _ = eslice_functions(d)
        et = [fs[c](th[c]) for c in range(d["C"])]
        return dict(theta=th, ell=np.array([a for a, _ in et]), target=np.array([b for _, b in et]))
    tg = [d["fs"][c](th[c]) for c in range(d["C"])]
    return dict(theta=th, target=np.array([a for a, _ in tg]), grad=np.stack([b for _, b in tg]))


def advance(d, st, z, u):
    """One draw of every chain from the state ``st`` (not changed) with the randoms z [C, P] and u.  Returns a dict of
    arrays over the chains: the state the chains are left in (theta, target, grad or ell), the outcomes OUTCOME[kind], the
    other values the device reports, the draw's ``margin`` and ``scale`` -- what the f32 margin is relative to:
    max(1, |log rate|) for hmc_metric, max(1, |log y|) for eslice, 1 for NUTS."""
    for g in d["guards"]:
        if g is not None:
            g.band = False
    with np.errstate(over="ignore", invalid="ignore"):   # (a trajectory at 30 times the step leaves the finite numbers)
        o = _advance(d, st, z, u)
    band = np.array([g is not None and g.band for g in d["guards"]])
    for key in ("margin", "margin_ell"):   # a draw that met f32's BCE where it is no number to hold a decision to
        if key in o:
            o[key] = np.where(band, 0.0, o[key])
    return o


def _advance(d, st, z, u):
    C, kind = d["C"], d["kind"]
    if kind == "nuts":
        table = np.stack([entry_of(d, c) for c in range(C)])
        o = nr.run_chains(d["fs"], st["theta"], st["target"], st["grad"], z, u, d["steps"], d["max_depth"],
                          (d["form"], table))
        o["scale"] = np.ones(C)
        return o
    if kind == "hmc_metric":
        code = DIAG if d["form"] == "diag" else TRIL
        rows = [hmc_metric_draw(d["fs"][c], st["theta"][c], st["target"][c], st["grad"][c], code, entry_of(d, c), z[c], u[c],
                                d["steps"][c], d["num_steps"]) for c in range(C)]
        o = dict(theta=np.stack([r[0] for r in rows]), target=np.array([r[1] for r in rows], np.float64),
                 grad=np.stack([r[2] for r in rows]), accepted=np.array([int(r[3]) for r in rows]),
                 h_cur=np.array([r[4] for r in rows]), h_prop=np.array([r[5] for r in rows]),
                 rate=np.array([r[6] for r in rows]))
        with np.errstate(invalid="ignore", divide="ignore"):
            o["dh"] = o["h_cur"] - o["h_prop"]   # the log rate; the decision is u < min(exp(log rate), 1)
            fin = np.isfinite(o["dh"])           # (a log rate of -inf or NaN is a clear rejection)
            o["margin"] = np.where(fin, np.abs(np.log(u) - np.minimum(o["dh"], 0.0)), np.inf)
            o["scale"] = np.where(fin, np.maximum(1.0, np.abs(o["dh"])), 1.0)
        return o
    fs, m, s = eslice_functions(d)
    o = er.draw_chains(fs, st["theta"], st["ell"], st["target"], m, s, z, u, d["max_shrinks"])
    o["accepted"], o["exhausted"] = o["accepted"].astype(int), o["exhausted"].astype(int)
    with np.errstate(divide="ignore"):
        logy = st["ell"] + np.log(u[:, 0])
    o["scale"] = np.where(np.isfinite(logy), np.maximum(1.0, np.abs(logy)), 1.0)
    return o


def state_of(d, o):
    keys = ("theta", "target", "ell") if d["kind"] == "eslice" else ("theta", "target", "grad")
    return {k: np.array(o[k], np.float64) for k in keys}


def restate(d, st=None, z=None, u=None):
    """The draws of a case by the restatement, each from the state the one before left: a list of ``advance`` dicts.
    ``st``: the state the device starts from; ``z`` / ``u``: other randoms [draws, ...]."""
    st = start(d) if st is None else st
    z = d["z"] if z is None else z
    u = d["u"] if u is None else u
    outs = []
    for k in range(len(z)):
        o = advance(d, st, z[k], u[k])
        st = state_of(d, o)
        outs.append(o)
    return outs


def set_aside(d, o):
    """The chains of a draw that a comparison sets aside: the margin is at most 1e-9 in f64, at most F32_DECISION_TOL times
    the draw's scale in f32."""
    if d["dtype"] == "f64":
        return o["margin"] <= MARGIN
    if d["kind"] == "eslice":
        return (o["margin_ell"] <= F32_DECISION_TOL * o["scale"]) | (o["margin_angle"] <= F32_DECISION_TOL)
    return o["margin"] <= F32_DECISION_TOL * o["scale"]


def cap(d):
    """The number of (chain, draw) pairs of a case that may be set aside."""
    return int(MAX_UNDER[d["dtype"]] * d["C"] * d["draws"])
