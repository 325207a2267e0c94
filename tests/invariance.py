"""Invariance from exact draws: the harness of tests/test_invariance_host.py and tests/test_invariance_gpu.py.
TEST INFRASTRUCTURE ONLY, numpy only.

C independent chains start from exact draws of a target pi and run n iterations of a transition.  If the transition leaves
pi invariant, every chain's state is still an exact draw of pi and the chains are independent: the ensemble is an iid sample
of pi, whatever the mixing.  Its moments are held against those of a second, larger exact sample by Welch's z, one z per
feature, and ``threshold(K_TOTAL)`` is the two-sided normal quantile at which the whole GPU file raises a false alarm with
probability 1e-3 (Bonferroni over the K_TOTAL z-scores it asserts on): derived, not measured.

What is here: the targets (Gaussian mixtures as tests/test_dist_gpu.py builds them, linear-Gaussian posteriors in closed
form) with ``exact_draws``; ``features`` / ``z_scores`` / ``threshold``; the case table ``CASES`` with every step and scale
(chosen on the CPU from the transitions below alone); and vectorised numpy transitions over [C, P] -- batched
transcriptions of tests/dist_restatement.py (hmc_draw, mala_draw, mh_draw), mh_mvn_restatement, mala_mvn_restatement,
hmc_metric_restatement, gibbs_restatement and pt_restatement.between -- with the mutant switches that show the test's
power.  The transitions calibrate the test on the CPU; the device test uses only the targets, the table and the
statistics."""
import functools
import statistics
import zlib

import numpy as np

from tests import dist_restatement as dr

N_ITERS, C_GPU, N_REF = 16, 16384, 65536       # the device test's iterations, chains and reference draws
LADDER_T = (1.0, 0.6, 0.3, 0.1)
CROSS = 8                                       # cross products among the first min(P, CROSS) coordinates


# ------------------------------------------------------------------------------------------------ targets
class Target:
    """A Gaussian mixture sum_k w_k N(mean_k, cov_k) as the tables (c, mean, prec) of tests/dist_restatement.py.  ``c``
    given: the log-density is c_k - d^T prec_k d / 2 with that constant (a posterior with its evidence left in)."""

    def __init__(self, weights, means, covs, c=None):
        w = np.asarray(weights, np.float64)
        self.means, self.covs = np.asarray(means, np.float64), np.asarray(covs, np.float64)
        self.probs = w / w.sum()
        self.c, self.mean, self.prec = dr.tables(w, self.means, self.covs, normalized=c is None)
        if c is not None:
            self.c = np.asarray(c, np.float64)
        self.chol = np.linalg.cholesky(self.covs)
        self.M, self.P = self.means.shape

    def value_grad(self, theta, temp=None, grad=True):
        """(log p [C], grad [C, P]) at theta [C, P], times ``temp`` (a number or [C]) where there is one."""
        d = theta[None] - self.mean[:, None, :]                       # [M, C, P]
        v = np.matmul(d, self.prec)                                    # prec_k is symmetric
        a = self.c[:, None] - 0.5 * np.einsum("kci,kci->kc", d, v)
        if self.M == 1:
            val, g = a[0], -v[0]
        else:
            A = a.max(0)
            e = np.exp(a - A)
            s = e.sum(0)
            val = A + np.log(s)
            g = -np.einsum("kc,kci->ci", e, v) / s[:, None] if grad else None
        if temp is not None:
            temp = np.asarray(temp, np.float64)
            val = val * temp
            g = g * (temp[:, None] if temp.ndim else temp) if grad else None
        return (val, g) if grad else val

    def value(self, theta, temp=None):
        return self.value_grad(theta, temp, grad=False)


def exact_draws(target, n, rng, t=None):
    """n exact draws [n, P] of a Target, of a mixture (weights, means, covs) or of a Gaussian (mean, cov): the component
    by its weight, then mean_k + chol(cov_k) z.  ``t``: the law of the density to the power t, which for one Gaussian is
    N(mean, cov / t) -- a distribution plan multiplies its whole log-density by the temperature, an MLP plan its
    likelihood and its prior, so this is the tempered law of both.  A tempered mixture of several components has no
    such form and is refused."""
    if not isinstance(target, Target):
        target = Target(*target) if len(target) == 3 else Target([1.0], np.asarray(target[0])[None], np.asarray(target[1])[None])
    if t is not None and t != 1.0 and target.M > 1:
        raise ValueError("a tempered mixture of several components has no exact sampler here")
    k = rng.choice(target.M, size=n, p=target.probs) if target.M > 1 else np.zeros(n, int)
    z = rng.standard_normal((n, target.P))
    x = target.means[k] + np.einsum("nij,nj->ni", target.chol[k], z) / np.sqrt(1.0 if t is None else t)
    return x


def mixture(P, M):
    """The mixture tests.test_dist_gpu._mixture(P, M) builds (the device test holds the two tables against each other)."""
    w, means, covs, _ = dr.random_mixture(P, M, seed=100 * P + M)
    return Target(w, means, covs)


LIK_SCALE, PRIOR_SIGMA = 0.7, 2.0


def linear_gaussian(D, N, seed=3):
    """x [N, D], y [N, 1] and the Target of a one-layer plan (dims [D, 1], identity, bias) under a Gaussian likelihood of
    scale 0.7 and a N(0, 2^2) prior, theta = (w, b): Gaussian with precision X^T X / s^2 + I / sigma^2.  D = 3 is
    tests.regression_restatement.linear_gaussian() to the bit.  The Target's constant is the log-target at the mean,
    evidence included, so that ``value`` is what the plan's log_target returns."""
    s, sigma = LIK_SCALE, PRIOR_SIGMA
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D))
    w = np.array([0.8, -0.5, 0.3]) if D == 3 else 0.8 * np.cos(1.3 * np.arange(D))
    y = x @ w + 0.2 + s * rng.standard_normal(N)
    X = np.concatenate([x, np.ones((N, 1))], 1)
    prec = X.T @ X / s ** 2 + np.eye(D + 1) / sigma ** 2
    cov = np.linalg.inv(prec)
    mean = cov @ X.T @ y / s ** 2
    r = y - X @ mean
    c = (-0.5 * r @ r / s ** 2 - N * np.log(s * np.sqrt(2 * np.pi))
         - 0.5 * mean @ mean / sigma ** 2 - (D + 1) * np.log(sigma * np.sqrt(2 * np.pi)))
    tgt = Target([1.0], mean[None], ((cov + cov.T) / 2)[None], c=[c])
    tgt.prec = ((prec + prec.T) / 2)[None]
    return x, y[:, None], tgt


# dims [3, 1]: the register-resident evaluation; [12, 1], N = 70: the LDS tile loop; [200, 1]: the layerwise path ("bgemm")
LINEAR = {"lin3": (3, 50), "lin12": (12, 70), "lin200": (200, 70)}


@functools.lru_cache(maxsize=None)
def target_of(name):
    if name in LINEAR:
        return linear_gaussian(*LINEAR[name])[2]
    P, M = (int(v) for v in name[3:].split("_"))
    return mixture(P, M)


# ------------------------------------------------------------------------------------------------ statistics
def n_features(P):
    m = min(P, CROSS)
    return 2 * P + m * (m - 1) // 2 + 2


def features(theta, logp):
    """[n, n_features(P)]: every coordinate, every square, the products theta_i theta_j (i < j) of the first min(P, 8)
    coordinates, log p and its square.  On the device side ``logp`` is the target the kernel carries over the chain's
    temperature, so a stale cached target shows here as well."""
    theta, logp = np.asarray(theta, np.float64), np.asarray(logp, np.float64)
    m = min(theta.shape[1], CROSS)
    i, j = np.triu_indices(m, 1)
    return np.concatenate([theta, theta * theta, theta[:, i] * theta[:, j], logp[:, None], logp[:, None] ** 2], 1)


def feature_name(P, k):
    m = min(P, CROSS)
    i, j = np.triu_indices(m, 1)
    names = [f"theta[{a}]" for a in range(P)] + [f"theta[{a}]^2" for a in range(P)] + \
        [f"theta[{a}]*theta[{b}]" for a, b in zip(i, j)] + ["logp", "logp^2"]
    return names[k]


def moments(x):
    """(n, mean, unbiased variance) per column."""
    x = np.asarray(x, np.float64)
    return x.shape[0], x.mean(0), x.var(0, ddof=1)


def reference_moments(target, n_ref, rng, t=None, chunk=8192):
    """``moments`` of the features of n_ref exact draws, accumulated chunk by chunk around the first chunk's mean."""
    shift, s1, s2, done = None, 0.0, 0.0, 0
    while done < n_ref:
        k = min(chunk, n_ref - done)
        th = exact_draws(target, k, rng, t)
        f = features(th, target.value(th))
        if shift is None:
            shift = f.mean(0)
        s1, s2, done = s1 + (f - shift).sum(0), s2 + ((f - shift) ** 2).sum(0), done + k
    m = s1 / n_ref
    return n_ref, shift + m, (s2 - n_ref * m * m) / (n_ref - 1)


def z_scores(a, b):
    """Welch's z per feature, (mean_a - mean_b) / sqrt(var_a / n_a + var_b / n_b); ``a`` and ``b`` are feature arrays
    [n, F] or their ``moments``."""
    (na, ma, va), (nb, mb, vb) = (m if isinstance(m, tuple) else moments(m) for m in (a, b))
    return (ma - mb) / np.sqrt(va / na + vb / nb)


def threshold(k_total):
    """The two-sided normal quantile at which k_total z-scores of exact iid samples raise a false alarm with probability
    1e-3 altogether (Bonferroni): 4.97 for 1500 statistics."""
    return statistics.NormalDist().inv_cdf(1 - 0.5e-3 / k_total)


# ------------------------------------------------------------------------------------------------ the case table
# Steps and scales: chosen on the CPU, from the transitions of this file alone, for a mean acceptance inside ACCEPT_BAND
# from exact starts (tests/test_invariance_host.py holds the table to it).  The factor scales are those of
# tests/test_mh_mvn_gpu.py (0.3, and 0.05 beyond 60 parameters) times ``fscale``; a metric's table is of that size too, and
# the dense-metric steps of mix5_3 and mix65_2 are STEPS' of tests/test_hmc_metric_gpu.py for their sizes (3.5 and 8.0).
ACCEPT_BAND = (0.3, 0.97)
G_INDEXED = 2
CASES = [
    dict(name="hmc/mix2_2/f64", sampler="hmc", target="mix2_2", dtype="f64", step=0.8, L=3),
    dict(name="hmc/mix65_2/f32/step_vec", sampler="hmc", target="mix65_2", dtype="f32", step=0.4, L=3, step_vec=True),
    dict(name="hmc/lin3/f64", sampler="hmc", target="lin3", dtype="f64", step=0.1, L=2),
    dict(name="hmc/lin200/f64/bgemm", sampler="hmc", target="lin200", dtype="f64", step=0.03, L=3, kernel="bgemm"),
    dict(name="hmc/lin12/f32/temp", sampler="hmc", target="lin12", dtype="f32", step=0.1, L=3, temp="halves"),
    dict(name="mala/mix5_3/f64", sampler="mala", target="mix5_3", dtype="f64", step=0.35),
    dict(name="mala/mix65_2/f32", sampler="mala", target="mix65_2", dtype="f32", step=0.3),
    dict(name="mala/lin3/f32/temp", sampler="mala", target="lin3", dtype="f32", step=0.012, temp="halves"),
    dict(name="mh/mix5_3/f32", sampler="mh", target="mix5_3", dtype="f32", scale=0.5),
    dict(name="mh/lin12/f64", sampler="mh", target="lin12", dtype="f64", scale=0.03),
    dict(name="mh_tril/mix5_3/f64/per_chain", sampler="mh_tril", target="mix5_3", dtype="f64", form="per_chain", fscale=1.5),
    dict(name="mh_tril/mix65_2/f32/indexed", sampler="mh_tril", target="mix65_2", dtype="f32", form="indexed", fscale=2.0),
    dict(name="mala_tril/mix5_3/f64/shared", sampler="mala_tril", target="mix5_3", dtype="f64", form="shared", step=0.6,
         fscale=2.0),
    dict(name="mala_tril/mix65_2/f32/indexed", sampler="mala_tril", target="mix65_2", dtype="f32", form="indexed", step=0.1,
         fscale=6.0),
    dict(name="mala_tril/mix5_1/f64/per_chain/temp", sampler="mala_tril", target="mix5_1", dtype="f64", form="per_chain",
         step=0.3, fscale=2.0, temp="halves"),
    dict(name="hmc_metric/dense/mix5_3/f64/shared", sampler="hmc_metric", kind="dense", target="mix5_3", dtype="f64",
         form="shared", step=3.5, L=3, fscale=1.0),
    dict(name="hmc_metric/dense/mix65_2/f32/indexed", sampler="hmc_metric", kind="dense", target="mix65_2", dtype="f32",
         form="indexed", step=8.0, L=3, fscale=1.0),
    dict(name="hmc_metric/diag/mix65_2/f64/per_chain", sampler="hmc_metric", kind="diag", target="mix65_2", dtype="f64",
         form="per_chain", step=8.0, L=3, fscale=1.0),
    dict(name="hmc_metric/diag/lin12/f32", sampler="hmc_metric", kind="diag", target="lin12", dtype="f32", form="shared",
         step=0.2, L=3, fscale=1.0),
    dict(name="gibbs/lin3/f64", sampler="gibbs", target="lin3", dtype="f64", blocks=[[0, 1], [2], [3]],
         scales=[0.1, 0.12, 0.12]),
    dict(name="gibbs/lin12/f32", sampler="gibbs", target="lin12", dtype="f32",
         blocks=[[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12]], scales=[0.06, 0.06, 0.08]),
    dict(name="ladder/mala/mix5_1/f64", sampler="mala", target="mix5_1", dtype="f64", step=0.5, ladder=True),
    dict(name="ladder/hmc/mix64_1/f32", sampler="hmc", target="mix64_1", dtype="f32", step=0.4, L=3, ladder=True),
    dict(name="ladder/mh/mix5_1/f32", sampler="mh", target="mix5_1", dtype="f32", scale=0.6, ladder=True),
]
CASE = {c["name"]: c for c in CASES}


def group_temps(case):
    """The temperature groups of a case, in row order and of equal size: [1] (None on the device), the two halves of a
    temperature vector, or the ladder."""
    if case.get("ladder"):
        return list(LADDER_T)
    return [1.0, 0.5] if case.get("temp") == "halves" else [1.0]


def n_statistics(case):
    return len(group_temps(case)) * n_features(target_of(case["target"]).P)


K_TOTAL = 2705   # sum of n_statistics over CASES: every z-score tests/test_invariance_gpu.py asserts on (the controls,
#                  which must be flagged, add no false alarm); tests/test_invariance_host.py recomputes it


def ladder_q(K=len(LADDER_T)):
    """Partner weights that are not symmetric: log_q[j, i] - log_q[i, j] != 0 for every pair."""
    i, j = np.arange(K)[:, None], np.arange(K)[None, :]
    q = np.exp(-0.5 * np.abs(i - j)) * (1.0 + 0.25 * j)
    np.fill_diagonal(q, 1.0)
    return q


def ladder_tables(t, q):
    """(t [K], log_q [K, K], cdf [K, K]) as tests.pt_restatement.Ladder builds them, in f64."""
    w = np.array(q, np.float64)
    np.fill_diagonal(w, 0.0)
    p = w / np.cumsum(w, axis=1)[:, -1][:, None]
    with np.errstate(divide="ignore"):
        logq = np.log(p)
    np.fill_diagonal(logq, 0.0)
    return np.asarray(t, np.float64), logq, np.cumsum(p, axis=1)


def _seed(case, salt):
    return [zlib.crc32(case["name"].encode()), salt]   # of the name: adding a case leaves the other cases' tables alone


def factors(G, P, rng, scale):
    """tests.test_ram_gpu._factors, batched: scale chol(A A^T / P + I / 2) per entry."""
    A = rng.standard_normal((G, P, P)) / np.sqrt(P)
    return scale * np.linalg.cholesky(A @ A.transpose(0, 2, 1) + 0.5 * np.eye(P))


def setup(case, C):
    """What a case adds to its sampler's arguments for C chains (numpy f64; the same on the host and on the device):
    ``temps`` [C] or None, ``step_vec`` [C] or None, ``table`` (factors [P, P] / [G, P, P] or diagonal scales [P] / [G, P])
    with ``index`` [C] int32 or None."""
    tgt = target_of(case["target"])
    P = tgt.P
    ts = group_temps(case)
    s = dict(target=tgt, temps=None if ts == [1.0] else np.repeat(ts, C // len(ts)), step_vec=None, table=None, index=None)
    if case.get("step_vec"):   # per-chain steps in [0.5, 1.5] times the table's
        s["step_vec"] = case["step"] * (0.5 + np.random.default_rng(_seed(case, 1)).random(C))
    if case.get("ladder") and "step" in case:   # one step per temperature: the law at t is wider by 1 / sqrt(t)
        s["step_vec"] = case["step"] / np.sqrt(s["temps"]) if case["sampler"] == "hmc" else case["step"] / s["temps"]
    if "form" in case:
        G = dict(shared=1, per_chain=C, indexed=G_INDEXED)[case["form"]]
        rng = np.random.default_rng(_seed(case, 2))
        size = (0.05 if P > 60 else 0.3) * case["fscale"]
        if case.get("kind") == "diag":
            tab = size * (0.5 + rng.random((G, P)))
        else:
            tab = factors(G, P, rng, size)
        s["table"] = tab[0] if case["form"] == "shared" else tab
        if case["form"] == "indexed":
            s["index"] = ((np.arange(C) + 1) % G_INDEXED).astype(np.int32)
    return s


def start(case, C, rng):
    """theta [C, P]: row block k of C / K rows drawn exactly from the law at the k-th temperature of the case."""
    tgt, ts = target_of(case["target"]), group_temps(case)
    return np.concatenate([exact_draws(tgt, C // len(ts), rng, t) for t in ts])


def case_z(case, theta, logp, rng, n_ref=N_REF, untempered=False):
    """The z-scores of a case's final states, one row of n_features per temperature group, each group against ``n_ref``
    exact draws of its own law (``untempered``: of the law at t = 1, the control that must be flagged)."""
    tgt, ts = target_of(case["target"]), group_temps(case)
    R = theta.shape[0] // len(ts)
    return np.stack([z_scores(features(theta[k * R:(k + 1) * R], logp[k * R:(k + 1) * R]),
                              reference_moments(tgt, n_ref, rng, None if untempered else t)) for k, t in enumerate(ts)])


def worst(z, P):
    """(largest |z|, the name of its feature)."""
    k = int(np.argmax(np.abs(z)))
    return float(np.abs(z).reshape(-1)[k]), feature_name(P, k % z.shape[-1]) + (f" (group {k // z.shape[-1]})" if z.shape[0] > 1 else "")


# ------------------------------------------------------------------------------------------------ the transitions
def _keep(acc, new, old):
    return np.where(acc[:, None] if new.ndim == 2 else acc, new, old)


def _rows(step, C):
    step = np.asarray(step, np.float64)
    return np.broadcast_to(step, (C,))


def mh(tgt, th, t, z, u, scale, temp=None):
    """dist_restatement.mh_draw for [C, P]: (theta, target, accepted)."""
    prop = th + scale * z
    tp = tgt.value(prop, temp)
    acc = np.log(u) < tp - t
    return _keep(acc, prop, th), _keep(acc, tp, t), acc


def mala(tgt, th, t, g, z, u, step, temp=None, mutant=None):
    """dist_restatement.mala_draw for [C, P]: (theta, target, grad, accepted).  ``mutant`` 'no_ratio' drops the proposal
    densities from the log-rate."""
    e = _rows(step, len(th))[:, None]
    loc = th + 0.5 * e * g
    prop = loc + np.sqrt(e) * z
    tp, gp = tgt.value_grad(prop, temp)
    loc2 = prop + 0.5 * e * gp
    qf, qb = ((prop - loc) ** 2).sum(1), ((th - loc2) ** 2).sum(1)
    lr = tp - t
    if mutant != "no_ratio":
        lr = lr + qf / (2 * e[:, 0]) - qb / (2 * e[:, 0])
    acc = np.log(u) < lr
    return _keep(acc, prop, th), _keep(acc, tp, t), _keep(acc, gp, g), acc


def hmc(tgt, th, t, g, p, u, step, L, temp=None):
    """dist_restatement.hmc_draw for [C, P]: (theta, target, grad, accepted)."""
    e = _rows(step, len(th))[:, None]
    h_cur = -t + 0.5 * (p * p).sum(1)
    q, tq, gq = th, t, g
    p = p + 0.5 * e * g
    for k in range(1, L + 1):
        q = q + e * p
        tq, gq = tgt.value_grad(q, temp)
        p = p + (e if k < L else 0.5 * e) * gq
    h_prop = -tq + 0.5 * (p * p).sum(1)
    with np.errstate(over="ignore"):
        acc = u < np.minimum(1.0, np.exp(h_cur - h_prop))
    return _keep(acc, q, th), _keep(acc, tq, t), _keep(acc, gq, g), acc


def _apply(L, index, x, trans=False):
    """Row c of the result is L_c x_c (``trans``: L_c^T x_c) for factors [P, P], [C, P, P] or [G, P, P] with an index."""
    if L.ndim == 2:
        return x @ (L if trans else L.T)
    if index is None:
        return np.einsum("cji,cj->ci" if trans else "cij,cj->ci", L, x)
    out = np.empty_like(x)
    for k in range(L.shape[0]):
        m = index == k
        out[m] = x[m] @ (L[k] if trans else L[k].T)
    return out


def _solve(L, index, r):
    """Row c of the result is L_c^-1 r_c."""
    if L.ndim == 2:
        return np.linalg.solve(L, r.T).T
    if index is None:
        return np.linalg.solve(L, r[:, :, None])[:, :, 0]
    out = np.empty_like(r)
    for k in range(L.shape[0]):
        m = index == k
        out[m] = np.linalg.solve(L[k], r[m].T).T
    return out


def _tril(L):
    return np.tril(L)   # (numpy takes the lower triangle of the last two axes)


def mh_tril(tgt, th, t, L, index, z, u, temp=None):
    """mh_mvn_restatement.mh_mvn_draw for [C, P]: (theta, target, accepted)."""
    prop = th + _apply(_tril(L), index, z)
    tp = tgt.value(prop, temp)
    acc = np.log(u) < tp - t
    return _keep(acc, prop, th), _keep(acc, tp, t), acc


def mala_tril(tgt, th, t, g, L, index, z, u, step, temp=None, mutant=None):
    """mala_mvn_restatement.mala_mvn_draw for [C, P]: (theta, target, grad, accepted).  The constants of the two
    proposal log-densities cancel; what remains is (|L^-1 (theta' - loc)|^2 - |L^-1 (theta - loc')|^2) / 2.  ``mutant``
    'no_ratio' drops it, 'identity_ratio' takes it under the identity instead of L L^T."""
    L = _tril(L)
    e = _rows(step, len(th))[:, None]
    loc = th + 0.5 * e * g
    prop = loc + _apply(L, index, z)
    tp, gp = tgt.value_grad(prop, temp)
    loc2 = prop + 0.5 * e * gp
    lr = tp - t
    if mutant != "no_ratio":
        yf, yb = prop - loc, th - loc2
        if mutant != "identity_ratio":
            yf, yb = _solve(L, index, yf), _solve(L, index, yb)
        lr = lr + 0.5 * (yf * yf).sum(1) - 0.5 * (yb * yb).sum(1)
    acc = np.log(u) < lr
    return _keep(acc, prop, th), _keep(acc, tp, t), _keep(acc, gp, g), acc


def hmc_metric(tgt, th, t, g, kind, table, index, v, u, step, L, temp=None, mutant=None):
    """hmc_metric_restatement.hmc_metric_draw for [C, P] in the whitened velocity v: (theta, target, grad, accepted).
    ``kind`` 'dense' with factors, 'diag' with scales ([P], [C, P] or [G, P] with an index).  ``mutant`` 'kinetic' takes
    the kinetic energy in the wrong variable, |L v|^2 / 2."""
    if kind == "diag":
        s = table if table.ndim == 1 else table[index] if index is not None else table
        mul = tmul = lambda x: s * x
    else:
        F = _tril(table)
        mul, tmul = (lambda x: _apply(F, index, x)), (lambda x: _apply(F, index, x, trans=True))
    kin = (lambda w: 0.5 * (mul(w) ** 2).sum(1)) if mutant == "kinetic" else (lambda w: 0.5 * (w * w).sum(1))
    e = _rows(step, len(th))[:, None]
    h_cur = -t + kin(v)
    q, tq, gq = th, t, g
    v = v + 0.5 * e * tmul(g)
    for k in range(1, L + 1):
        q = q + e * mul(v)
        tq, gq = tgt.value_grad(q, temp)
        v = v + (e if k < L else 0.5 * e) * tmul(gq)
    h_prop = -tq + kin(v)
    with np.errstate(over="ignore"):
        acc = u < np.minimum(np.exp(h_cur - h_prop), 1.0)
    return _keep(acc, q, th), _keep(acc, tq, t), _keep(acc, gq, g), acc


def gibbs(tgt, th, t, blocks, scales, z, u, mode="intended", temp=None):
    """gibbs_restatement.gibbs_draw for [C, P] with u [C, S]: (theta, target, accepted [C, S])."""
    assert mode in ("intended", "reference")
    cur, prop, tcur = th.copy(), th.copy(), t.copy()
    acc = np.zeros((len(th), len(blocks)), bool)
    for s, idx in enumerate(blocks):
        prop[:, idx] = prop[:, idx] + scales[s] * z[:, idx]
        tv = tgt.value(prop, temp)
        a = np.log(u[:, s]) < tv - tcur
        cur[:, idx] = np.where(a[:, None], prop[:, idx], cur[:, idx])
        tcur = np.where(a, tv, tcur)
        acc[:, s] = a
        if mode == "intended":
            prop[:, idx] = cur[:, idx]
    return cur, tcur, acc


def draw_partners(cdf, v):
    """partners [K, R] from uniforms v [K, R] by the inverse CDF of each row (tests.pt_restatement.draw_partners)."""
    K = len(cdf)
    out = np.empty(v.shape, np.int32)
    for i in range(K):
        j = np.searchsorted(cdf[i], v[i], side="right")
        out[i] = np.where(j < K, j, K - 2 if i == K - 1 else K - 1)
    return out


def between(t, logq, theta, target, grad, partners, u, mutant=None):
    """pt_restatement.between in f64 for valid partners [K, R] and u [K, R]: (theta, target, grad, swap [K, R]).
    ``mutant`` 'sign' flips (t_i - t_j) in the log-rate, 'no_rescale' exchanges the targets (and gradients) without the
    factors t_i / t_j."""
    K = len(t)
    R = theta.shape[0] // K
    th, tg = theta.reshape(K, R, -1).copy(), target.reshape(K, R).copy()
    g = None if grad is None else grad.reshape(K, R, -1).copy()
    ar = np.arange(R)
    swaps = np.zeros((K, R), bool)
    log_u = np.log(u)
    for i in range(K):
        j = partners[i]
        ti, tj = t[i], t[j]
        tgi, tgj = tg[i].copy(), tg[j, ar]
        lr = (ti - tj) * (tgj / tj - tgi / ti)
        if mutant == "sign":
            lr = -lr
        lr = lr + (logq[j, i] - logq[i, j])
        m = log_u[i] < lr
        swaps[i] = m
        fi, fj = (ti / tj)[m], (tj / ti)[m]
        if mutant == "no_rescale":
            fi, fj = np.ones_like(fi), np.ones_like(fj)
        rj, rr = j[m], ar[m]
        a, b = th[i, rr].copy(), th[rj, rr].copy()
        th[i, rr], th[rj, rr] = b, a
        tg[i, rr], tg[rj, rr] = tgj[m] * fi, tgi[m] * fj
        if g is not None:
            a, b = g[i, rr].copy(), g[rj, rr].copy()
            g[i, rr], g[rj, rr] = b * fi[:, None], a * fj[:, None]
    return th.reshape(theta.shape), tg.reshape(-1), None if g is None else g.reshape(grad.shape), swaps


# ------------------------------------------------------------------------------------------------ a case on the host
def run_host(case, C, n, rng, mutant=None, mode="intended"):
    """n iterations of a case's transition for C chains from exact starts, variates from ``rng``.  Returns
    dict(theta, logp, accept, swap): the final states, the carried target over the temperature, the mean acceptance of
    the within-chain transition and, on a ladder, of the exchanges."""
    s = setup(case, C)
    tgt, temps, P = s["target"], s["temps"], s["target"].P
    th = start(case, C, rng)
    t, g = tgt.value_grad(th, temps)
    name, step = case["sampler"], s["step_vec"] if s["step_vec"] is not None else case.get("step")
    if case.get("ladder"):
        tl, logq, cdf = ladder_tables(LADDER_T, ladder_q())
        K = len(tl)
    acc_sum = swap_sum = 0.0
    for _ in range(n):
        z = rng.standard_normal((C, P))
        if name == "mh":
            th, t, acc = mh(tgt, th, t, z, rng.random(C), case["scale"], temps)
        elif name == "mala":
            th, t, g, acc = mala(tgt, th, t, g, z, rng.random(C), step, temps, mutant)
        elif name == "hmc":
            th, t, g, acc = hmc(tgt, th, t, g, z, rng.random(C), step, case["L"], temps)
        elif name == "mh_tril":
            th, t, acc = mh_tril(tgt, th, t, s["table"], s["index"], z, rng.random(C), temps)
        elif name == "mala_tril":
            th, t, g, acc = mala_tril(tgt, th, t, g, s["table"], s["index"], z, rng.random(C), step, temps, mutant)
        elif name == "hmc_metric":
            th, t, g, acc = hmc_metric(tgt, th, t, g, case["kind"], s["table"], s["index"], z, rng.random(C), step,
                                       case["L"], temps, mutant)
        elif name == "gibbs":
            th, t, acc = gibbs(tgt, th, t, case["blocks"], case["scales"], z, rng.random((C, len(case["blocks"]))), mode,
                               temps)
        acc_sum += acc.mean()
        if case.get("ladder"):
            partners = draw_partners(cdf, rng.random((K, C // K)))
            th, t, g2, sw = between(tl, logq, th, t, None if name == "mh" else g, partners, rng.random((K, C // K)), mutant)
            g = g if g2 is None else g2
            swap_sum += sw.mean()
    return dict(theta=th, logp=t if temps is None else t / temps, accept=acc_sum / n, swap=swap_sum / n)
