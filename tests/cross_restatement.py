"""Every sampler of the generic kernels under every prior family and every likelihood, restated in f64 on the CPU: one case
builder, ``cross_case``, over tests/regression_restatement.py's Target (any ``torch.distributions`` prior, any likelihood)
and the draws the other restatements already hold (prior_restatement's hmc / mala / mh, ram / am / gibbs / mh_mvn /
mala_mvn _restatement).  ``rr.sampler_case`` and ``pr.other_case`` are calls of this module's ``run_case``: the loop over
steps and chains is written once, here.

Activation codes 0 none, 1 sigmoid, 2 tanh, 3 relu; likelihood codes 0 BCE-sum, 1 CE-sum, 2 Gaussian, 3 Laplace,
4 Poisson.  Needs no GPU."""
import numpy as np

from tests import prior_restatement as pr
from tests import regression_restatement as rr
from tests.am_restatement import am_draw
from tests.gibbs_restatement import gibbs_draw
from tests.mala_mvn_restatement import mala_mvn_draw
from tests.mh_mvn_restatement import mh_mvn_draw
from tests.ram_restatement import ram_draw

SAMPLERS = ("hmc", "mala", "mh", "ram", "am", "gibbs", "mh_tril", "mala_tril")
GRADIENT_SAMPLERS = ("hmc", "mala", "mala_tril")
FAMILIES = ("normal", "laplace", "studentt", "cauchy")
LOSSES = ("bce", "ce", "gauss", "laplace", "poisson")
LIK_CODE = dict(bce=0, ce=1, gauss=2, laplace=3, poisson=4)
LIK_SCALE = dict(bce=1.0, ce=1.0, gauss=0.5, laplace=0.8, poisson=1.0)
REGRESSION = ("gauss", "laplace", "poisson")

# name: the model, its rows, how the plan is set up (a variant of Plan.set_variant, the row-wave option), the evaluation
# path that set-up reaches (tiny_kind of ey_generic.hip: 0 the LDS tile loop, 1 TinyDyn, 4 TinyFix<2, 4, 3, 3>,
# 2 TinyFix<2, 2, 2, 1>) and the likelihoods its output admits: CE needs two outputs or more, BCE probabilities.
# "bce" is the one shape with a sigmoid output: without it no sampler would meet BCE-sum under these families.
SHAPES = {
    "fix": dict(dims=[4, 3, 3], acts=[1, 0], N=40, variant=0, waves="off", tiny=4, losses=("ce",) + REGRESSION),
    "dyn": dict(dims=[3, 4, 2], acts=[1, 2], N=40, variant=512, waves="off", tiny=1, losses=("ce",) + REGRESSION),
    "dyn128": dict(dims=[3, 4, 2], acts=[1, 2], N=150, variant=0, waves="off", tiny=1, losses=("ce",) + REGRESSION),
    "lds1": dict(dims=[3, 4, 2], acts=[1, 2], N=40, variant=0, waves="off", tiny=0, losses=("ce",) + REGRESSION),
    "lds3": dict(dims=[4, 8, 3], acts=[3, 0], N=150, variant=0, waves="off", tiny=0, losses=("ce",) + REGRESSION),
    "waves": dict(dims=[2, 3, 1], acts=[2, 0], N=150, variant=0, waves="on", tiny=1, losses=REGRESSION),
    "bce": dict(dims=[2, 2, 1], acts=[1, 1], N=40, variant=0, waves="off", tiny=2, losses=("bce",)),
}
FUSED = {("lds3", "ce")}  # with a Normal prior the fused 16x16x4 kernels serve this cell's hmc / mala / mh and values
WAVE_SAMPLERS = ("hmc", "mala", "mh")  # the kernels with a row-wave form; the others are one wave by construction

TINY_D0, TINY_DH = 8, 4
TINY_FIX = {(2, 2, 1): 2, (2, 3, 2, 1): 3, (4, 3, 3): 4, (4, 3, 2, 3): 5, (1, 2, 1): 6, (2, 3, 3, 2): 7, (4, 1): 8}


def tiny_kind(dims, N, variant=0):
    """The documented rule of the register-resident evaluation (the comment above tiny_kind in ey_generic.hip): never with
    variant bit 8 or beyond 3 layers / 8 inputs / 4 nodes; the compile-time shapes for any batch; otherwise from two
    64-row tiles up, or with variant bit 9."""
    if len(dims) - 1 > 3 or dims[0] > TINY_D0 or max(dims[1:]) > TINY_DH or variant & 256:
        return 0
    if tuple(dims) in TINY_FIX:
        return TINY_FIX[tuple(dims)]
    return 1 if (variant & 512 or N >= 128) else 0


def num_params(dims):
    return sum((dims[k] + 1) * dims[k + 1] for k in range(len(dims) - 1))


def node_blocks(dims):
    """The nodes of an MLP as Gibbs blocks: per layer and node its row of the weight matrix and its bias."""
    blocks, off = [], 0
    for k in range(len(dims) - 1):
        din, dout = dims[k], dims[k + 1]
        blocks += [[off + din * n + i for i in range(din)] + [off + din * dout + n] for n in range(dout)]
        off += (din + 1) * dout
    return blocks


def rows_for(dims, loss, N, seed=0):
    """N rows for a model under a likelihood: rr.synthetic for the regression forms, standard normal x with one-hot (CE) or
    Bernoulli (BCE) responses otherwise."""
    if loss in REGRESSION:
        return rr.synthetic(dims, loss, N, seed=seed)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, dims[0]))
    if loss == "bce":
        return x, (rng.random((N, dims[-1])) < 0.5).astype(np.float64)
    return x, np.eye(dims[-1])[rng.integers(0, dims[-1], N)]


def make_target(dims, acts, loss, x, y, prior, temperature=None):
    """rr.Target for a regression loss, pr.Target for BCE / CE."""
    if loss in REGRESSION:
        return rr.Target(dims, acts, loss, x, y, scale=LIK_SCALE[loss], prior=prior, temperature=temperature)
    return pr.Target(dims, acts, LIK_CODE[loss], x, y, prior, temperature=temperature)


# ------------------------------------------------------------------------------------------------ the fixture
def load_g21():
    """The groups of g21_cross_traces.npz, {'values/<family>/<loss>' or 'trace/<sampler>': rec}, every rec completed with
    the model, its rows under the rec's loss, the loss's scale and the prior's tables."""
    import json

    from tests.helpers import load
    npz = load("g21_cross_traces.npz")
    meta = json.loads(str(npz["meta"]))
    grouped = {}
    for k in npz.files:
        if k.startswith(("values/", "trace/")):
            g, f = k.rsplit("/", 1)
            grouped.setdefault(g, {})[f] = npz[k]
    for key, rec in grouped.items():
        tr = meta["traces"][key.split("/")[1]] if key.startswith("trace/") else None
        family, loss = (tr["family"], tr["loss"]) if tr else key.split("/")[1:]
        rec.update(dims=meta["model"]["dims"], acts=meta["model"]["acts"], x=npz["data/x"],
                   y=npz["data/counts" if loss == "poisson" else "data/y"], family=family, loss=loss,
                   lik_scale=meta["scales"][loss], loc=rec["tables"][0], scale=rec["tables"][1],
                   df=rec["tables"][2] if family == "studentt" else None)
        if tr:
            rec.update(sampler=key.split("/")[1], par=tr["par"], L=tr.get("L", 0))
            rec["scale_mh" if rec["sampler"] == "mh" else "step"] = tr["par"]
    return grouped


def g21_target(rec):
    return rr.Target(rec["dims"], rec["acts"], rec["loss"], rec["x"], rec["y"], scale=rec["lik_scale"],
                     prior=pr.make_prior(rec["family"], rec["loc"], rec["scale"], rec["df"]))


# ------------------------------------------------------------------------------------------------ the loop, written once
def _of(targets, c):
    return targets[c] if isinstance(targets, (list, tuple)) else targets


def start_state(sampler, targets, par, th0):
    """The state the draws of ``sampler`` carry for C chains from th0 [C, P]: theta, target, grad, and RAM's factors or
    AM's moments."""
    C, P = th0.shape
    start = [_of(targets, c).value_and_grad(t) for c, t in enumerate(th0)]
    st = dict(theta=th0.copy(), target=np.array([s[0] for s in start]), grad=np.array([s[1] for s in start]))
    if sampler == "ram":
        st["chol"] = np.stack([par["chol0"] * np.eye(P)] * C)
    if sampler == "am":
        st["am"] = [dict(mean=np.zeros(P), cov_sum=np.zeros((P, P)), cov=par["cov0"] * np.eye(P), num_accepted=0)
                    for _ in range(C)]
    return st


def advance(sampler, targets, par, st, it, z, u, u_mix=None, blocks=None, L=None):
    """One draw of every chain of ``st`` (in place) from z [C, P] and u [C] (Gibbs: [C, S]) at counter index ``it``.
    Returns (accepted, margin, log_rate, branch): per chain, per sub-step for Gibbs; margin = |log u - log rate| with HMC's
    log rate clipped at 0 (its decision is u < min(exp(log rate), 1)); branch is AM's, empty otherwise."""
    th, tv, gr = st["theta"], st["target"], st["grad"]
    P = th.shape[1]
    acc, margin, rate, branch = [], [], [], []
    for c in range(th.shape[0]):
        tgt = _of(targets, c)
        zc, uc = z[c], u[c]
        if sampler == "hmc":
            th[c], tv[c], gr[c], a, lr = pr.hmc_draw(tgt.value_and_grad, th[c], tv[c], gr[c], zc, uc, par["step"], par["L"])
            rate.append(lr)
            lr = min(lr, 0.0)  # the decision is u < min(exp(log rate), 1)
        elif sampler == "mala":
            th[c], tv[c], gr[c], a, lr = pr.mala_draw(tgt.value_and_grad, th[c], tv[c], gr[c], zc, uc, par["step"])
        elif sampler == "mh":
            th[c], tv[c], a, lr = pr.mh_draw(tgt.log_target, th[c], tv[c], zc, uc, par["scale"])
        elif sampler == "ram":
            th[c], tv[c], st["chol"][c], a, lr = ram_draw(tgt.log_target, th[c], tv[c], st["chol"][c], zc, uc, it + 1,
                                                          par["a"], par["g"])
        elif sampler == "am":
            am = st["am"][c]
            w = am_draw(tgt.log_target, th[c], tv[c], am["mean"], am["cov_sum"], am["cov"], am["num_accepted"],
                        par["cov0"] * np.eye(P), zc, u_mix[c], uc, it, 0, par["l"], par["b"], par["c"], par["t0"], par["eps"])
            th[c], tv[c], a, lr = w["theta"], w["target"], w["accepted"], w["log_rate"]
            st["am"][c] = {k: w[k] for k in ("mean", "cov_sum", "cov", "num_accepted")}
            branch.append(w["branch"])
        elif sampler == "gibbs":
            th[c], tv[c], a, lr, mg_ = gibbs_draw(tgt.log_target, th[c], tv[c], blocks, [par["scale"]] * len(blocks), zc, uc)
            acc.append(a); margin.append(mg_); rate.append(lr)
            continue
        elif sampler == "mh_tril":
            th[c], tv[c], a, lr = mh_mvn_draw(tgt.log_target, th[c], tv[c], L, zc, uc)
        else:
            th[c], tv[c], gr[c], a, lr = mala_mvn_draw(tgt.value_and_grad, th[c], tv[c], gr[c], L, zc, uc, par["step"])
        acc.append(int(a)); margin.append(abs(np.log(uc) - lr))
        if sampler != "hmc":
            rate.append(lr)
    return np.array(acc), np.array(margin), np.array(rate), np.array(branch)


def run_case(sampler, targets, par, d, blocks=None):
    """Completes the inputs ``d`` (th0 [C, P], z [steps, C, P], u, u_mix, and L for the dense proposals) with what the f64
    restatements make of them: per step the states [C, P], targets [C], decisions, margins and log rates, plus AM's
    branches.  ``targets`` is one target for all chains or a list of one per chain."""
    st = start_state(sampler, targets, par, d["th0"])
    out = dict(theta=[], target=[], accepted=[], margin=[], branch=[], log_rate=[])
    for it in range(d["z"].shape[0]):
        acc, margin, rate, branch = advance(sampler, targets, par, st, it, d["z"][it], d["u"][it], d["u_mix"][it],
                                            blocks=blocks, L=d.get("L"))
        out["theta"].append(st["theta"].copy()); out["target"].append(st["target"].copy())
        out["accepted"].append(acc); out["margin"].append(margin); out["branch"].append(branch); out["log_rate"].append(rate)
    d.update({k: np.array(v) for k, v in out.items()})
    d["final"] = st
    return d


# ------------------------------------------------------------------------------------------------ the cases
# Steps and scales per sampler and shape, chosen on the CPU so that every case of tests/test_cross_gpu.py both accepts and
# rejects at least five times (tests/test_cross_host.py holds them to it): the starts are 0.3 N(0, 1) draws, far from
# the mode on 150 rows, so the 150-row shapes take smaller steps than the 40-row ones.
PAR = dict(
    hmc=dict(L=4, step=dict(fix=0.06, dyn=0.09, dyn128=0.045, lds1=0.09, lds3=0.02, waves=0.05, bce=0.25)),
    mala=dict(step=dict(fix=0.012, dyn=0.02, dyn128=0.005, lds1=0.02, lds3=0.0012, waves=0.006, bce=0.15)),
    mh=dict(scale=dict(fix=0.08, dyn=0.1, dyn128=0.05, lds1=0.1, lds3=0.02, waves=0.06, bce=0.3)),
    ram=dict(a=0.234, g=0.7, chol0=dict(fix=0.08, dyn=0.1, dyn128=0.05, lds1=0.1, lds3=0.02, waves=0.06, bce=0.3)),
    am=dict(l=0.3, b=0.5, c=dict(fix=0.08, dyn=0.1, dyn128=0.05, lds1=0.1, lds3=0.02, waves=0.06, bce=0.3), eps=1e-2, t0=2,
            cov0=0.01),
    gibbs=dict(scale=dict(fix=0.3, dyn=0.35, dyn128=0.15, lds1=0.35, lds3=0.08, waves=0.2, bce=0.8)),
    mh_tril=dict(scale=dict(fix=0.1, dyn=0.12, dyn128=0.06, lds1=0.12, lds3=0.025, waves=0.07, bce=0.35)),
    mala_tril=dict(step=dict(fix=0.01, dyn=0.01, dyn128=0.001, lds1=0.01, lds3=0.0001, waves=0.005, bce=0.01),
                   scale=dict(fix=0.1, dyn=0.12, dyn128=0.02, lds1=0.12, lds3=0.004, waves=0.07, bce=0.35)),
)


# (sampler, shape, loss): a factor on the sampler's step or scale where the table above leaves a likelihood's cases short of
# five accepts or five rejects (a CE target is flatter at these starts than a Poisson one); MALA's step, a variance, takes
# the factor squared beside its dense proposal's scale
TUNE = {
    ('hmc', 'fix', 'ce'): 3, ('hmc', 'dyn', 'poisson'): 2, ('hmc', 'dyn', 'ce'): 4, ('hmc', 'dyn128', 'poisson'): 1.5,
    ('hmc', 'dyn128', 'ce'): 4, ('hmc', 'lds1', 'poisson'): 1.5, ('hmc', 'lds1', 'ce'): 4, ('hmc', 'lds3', 'laplace'): 1.5,
    ('hmc', 'lds3', 'poisson'): 1.5, ('hmc', 'lds3', 'ce'): 3, ('hmc', 'lds3', 'gauss'): 1.5, ('hmc', 'waves', 'poisson'): 1.5,
    ('hmc', 'bce', 'bce'): 2, ('mala', 'fix', 'laplace'): 1.5, ('mala', 'fix', 'ce'): 4, ('mala', 'dyn', 'ce'): 6,
    ('mala', 'dyn128', 'ce'): 3, ('mala', 'lds1', 'poisson'): 1.5, ('mala', 'lds1', 'ce'): 6, ('mala', 'lds3', 'poisson'): 3,
    ('mala', 'lds3', 'ce'): 12, ('mala', 'lds3', 'gauss'): 1.5, ('mala', 'lds3', 'laplace'): 3, ('mala', 'waves', 'poisson'): 1.5,
    ('mala_tril', 'dyn128', 'poisson'): 0.67, ('mala_tril', 'dyn128', 'gauss'): 2, ('mala_tril', 'lds3', 'gauss'): 0.33,
    ('mala_tril', 'lds3', 'poisson'): 0.67,
}
KNOB = dict(hmc="step", mala="step", mh="scale", ram="chol0", am="c", gibbs="scale", mh_tril="scale", mala_tril="scale")


def par_of(sampler, shape, loss=None):
    par = {k: (v[shape] if isinstance(v, dict) else v) for k, v in PAR[sampler].items()}
    m = TUNE.get((sampler, shape, loss), 1.0)
    par[KNOB[sampler]] *= m
    if sampler == "mala_tril":
        par["step"] *= m * m
    return par


def _rounded(a, round_to):
    return a if round_to is None or a is None else np.asarray(a).astype(round_to).astype(np.float64)


def cross_case(sampler, family, loss, shape, temp=False, seed=0, C=11, steps=5, round_to=None):
    """The inputs of ``steps`` draws of C chains of one of SAMPLERS on one of SHAPES under a prior of one of FAMILIES
    (distinct loc, scale and df per parameter; a Normal prior has loc != 0 too) and one of LOSSES, and what the f64
    restatements make of them (``run_case``).  ``temp`` gives every chain its own temperature in [0.3, 1];
    ``round_to=np.float32`` rounds the rows, the tables, the start, z, u, the temperatures and the dense factor to what an
    f32 plan holds, so that the restatement starts from the device's numbers."""
    sh = SHAPES[shape]
    if sampler not in SAMPLERS or family not in FAMILIES or loss not in sh["losses"]:
        raise ValueError(f"no such case: {sampler} / {family} / {loss} on {shape}")
    if shape == "waves" and sampler not in WAVE_SAMPLERS:
        raise ValueError(f"{sampler} has no row-wave form")
    dims, acts, N = sh["dims"], sh["acts"], sh["N"]
    P = num_params(dims)
    x, y = (_rounded(a, round_to) for a in rows_for(dims, loss, N, seed=20 + seed))
    loc, scale, df = (_rounded(a, round_to) for a in pr.distinct_tables(P, 100 + seed))
    prior = pr.make_prior(family, loc, scale, df)
    par = par_of(sampler, shape, loss)
    rng = np.random.default_rng(11000 + 10 * seed + SAMPLERS.index(sampler))
    blocks = node_blocks(dims)
    S = len(blocks)
    d = dict(sampler=sampler, family=family, loss=loss, shape=shape, dims=dims, acts=acts, x=x, y=y, loc=loc, scale=scale,
             df=df if family == "studentt" else None, par=par, lik=LIK_CODE[loss], lik_scale=LIK_SCALE[loss], blocks=blocks,
             th0=_rounded(0.3 * rng.standard_normal((C, P)), round_to), z=_rounded(rng.standard_normal((steps, C, P)), round_to),
             u=_rounded(rng.random((steps, C, S) if sampler == "gibbs" else (steps, C)), round_to),
             u_mix=_rounded(rng.random((steps, C)), round_to))
    d["temps"] = _rounded(0.3 + 0.7 * rng.random(C), round_to) if temp else None
    if sampler in ("mh_tril", "mala_tril"):
        d["L"] = np.tril(_rounded(pr.dense_lower(P, par["scale"], 50 + seed), round_to))
    d["target"] = make_target(dims, acts, loss, x, y, prior)
    d["targets"] = [make_target(dims, acts, loss, x, y, prior, temperature=float(t)) for t in d["temps"]] if temp \
        else d["target"]
    return run_case(sampler, d["targets"], par, d, blocks=blocks)


def decision_stats(d, f32=False):
    """(accepts, rejects, undecided) of a case: undecided are the decisions whose margin is at most 1e-9, or in f32 at most
    2e-3 max(1, |log rate|) -- what the device may legitimately decide the other way."""
    acc, margin = np.concatenate([a.ravel() for a in d["accepted"]]), np.concatenate([m.ravel() for m in d["margin"]])
    rate = np.concatenate([r.ravel() for r in d["log_rate"]])
    with np.errstate(invalid="ignore"):
        tol = 2e-3 * np.maximum(1.0, np.abs(rate)) if f32 else np.full(rate.shape, 1e-9)
    tol = np.where(np.isfinite(tol), tol, 1e-9)  # a log rate of -inf is a clear rejection
    return int(acc.sum()), int(acc.size - acc.sum()), int((margin <= tol).sum())
