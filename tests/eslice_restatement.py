"""Elliptical slice sampling (Murray, Adams & MacKay 2010) as include/eeyore_amd_eslice.h and DESIGN.md 4.25 state it, in
numpy f64 with explicit normals z and uniforms u.  TEST INFRASTRUCTURE ONLY, numpy only.

The target is N(m, diag s^2) x exp(ell).  ``draw`` is the transition for one chain; ``draw_chains`` loops it over the chains
of a case; ``draw_batch`` is the same transition vectorised over [C, P] for the invariance calibration (the host test holds
the two to each other).  Angles are in turns.  A draw's ``margin`` is the smallest |ell' - log y| over its evaluations and
|a| wherever the sign of a is branched on: a device draw may differ from this file only where the margin is tiny.

``prior_base`` and ``given_base`` build (ell, m, s) the two ways the library does; ``prior_base`` has the two mutant
switches of the host calibration: 'whole_target' slices on the whole log-target under the prior (the prior counts twice),
'untempered_scale' keeps sigma under a temperature where the tempered prior has sigma / sqrt(t)."""
import numpy as np

MAX_SHRINKS = 64           # EY_ESLICE_MAX_SHRINKS
MUTANTS = ("whole_target", "untempered_scale")


def words(max_shrinks=MAX_SHRINKS):
    """The uniforms a draw may read: word 0 the slice height, 1 the first angle, 2 + k the k-th shrink."""
    return 2 + max_shrinks


def _cs(a):
    """cos and sin of a turns, the range reduction done on the turns (what cospi / sinpi do)."""
    r = a - np.round(a)
    return np.cos(2.0 * np.pi * r), np.sin(2.0 * np.pi * r)


def prior_base(parts, mu, sigma, temp=None, mutant=None):
    """(f, m, s) without a base: ``parts(theta) -> (lik, prior)``, both tempered, under the Normal prior N(mu, sigma^2).
    f(theta) -> (ell, target) with ell the likelihood part; s = sigma / sqrt(temp)."""
    assert mutant in (None,) + MUTANTS
    t = 1.0 if temp is None else temp
    s = np.asarray(sigma, np.float64) / (1.0 if mutant == "untempered_scale" else np.sqrt(t))

    def f(th):
        lik, prior = parts(th)
        return (lik + prior if mutant == "whole_target" else lik), lik + prior
    return f, np.asarray(mu, np.float64), s


def given_base(target, m, s):
    """(f, m, s) with the base N(m, diag s^2): ``target(theta)`` is the (tempered) log-target;
    ell = target - sum_i -((theta_i - m_i) / s_i)^2 / 2."""
    m, s = np.asarray(m, np.float64), np.asarray(s, np.float64)

    def f(th):
        tv = target(th)
        d = (th - m) / s
        return tv + 0.5 * np.sum(d * d, axis=-1), tv
    return f, m, s


def draw(f, theta, ell, target, m, s, z, u, max_shrinks=MAX_SHRINKS):
    """One draw of one chain.  ``f(theta) -> (ell, target)``; theta, m, s, z [P]; u [>= 2 + max_shrinks].  Returns
    dict(theta, ell, target, accepted, n_evals, margin, exhausted, neg, pos, margin_ell, margin_angle, logy): the state the
    chain is left in, whether it moved, the evaluations made, the draw's margin, the shrinks made at a negative / a positive
    angle, the two parts of the margin (the smallest |ell' - log y|, the smallest |a| branched on) and log y."""
    assert 1 <= max_shrinks <= MAX_SHRINKS and len(u) >= words(max_shrinks)
    out = dict(theta=np.array(theta, np.float64), ell=ell, target=target, accepted=False, n_evals=0, margin=np.inf,
               exhausted=False, neg=0, pos=0, margin_ell=np.inf, margin_angle=np.inf, logy=np.nan)
    if not np.isfinite(ell):   # 5. stays put without evaluating
        return out
    nu, x = s * z, theta - m
    with np.errstate(divide="ignore"):
        logy = ell + np.log(u[0])
    out["logy"] = logy
    a = u[1]
    lo, hi = a - 1.0, a
    k = 0
    while True:
        c, sn = _cs(a)
        th = m + x * c + nu * sn
        e, t = f(th)
        out["n_evals"] += 1
        if abs(e - logy) < out["margin_ell"]:
            out["margin_ell"] = abs(e - logy)
        out["margin"] = min(out["margin"], out["margin_ell"])
        if e > logy:   # (a NaN compares false)
            out.update(theta=th, ell=e, target=t, accepted=True)
            return out
        if k == max_shrinks:
            out["exhausted"] = True
            return out
        out["margin_angle"] = min(out["margin_angle"], abs(a))
        out["margin"] = min(out["margin"], abs(a))
        if a < 0:
            lo, out["neg"] = a, out["neg"] + 1
        else:
            hi, out["pos"] = a, out["pos"] + 1
        a = lo + (hi - lo) * u[2 + k]
        k += 1


KEYS = ("theta", "ell", "target", "accepted", "n_evals", "margin", "exhausted", "neg", "pos", "margin_ell",
        "margin_angle", "logy")


def draw_chains(fs, theta, ell, target, m, s, z, u, max_shrinks=MAX_SHRINKS):
    """``draw`` for every chain c with its own f = fs[c] and scale s[c] (s [C, P] or [P]): a dict of arrays over the chains."""
    C = len(theta)
    s = np.broadcast_to(s, theta.shape)
    outs = [draw(fs[c], theta[c], ell[c], target[c], m, s[c], z[c], u[c], max_shrinks) for c in range(C)]
    return {k: np.array([o[k] for o in outs]) for k in KEYS}


def draw_batch(f, theta, ell, target, m, s, z, u, max_shrinks=MAX_SHRINKS):
    """``draw`` vectorised over the chains: ``f(theta [n, P], rows [n]) -> (ell [n], target [n])`` for the chains ``rows``;
    s [P] or [C, P].  Returns (theta, ell, target, accepted, n_evals)."""
    C = len(theta)
    theta, ell, target = theta.copy(), ell.copy(), target.copy()
    nu, x = s * z, theta - m
    with np.errstate(divide="ignore"):
        logy = ell + np.log(u[:, 0])
    a = u[:, 1].copy()
    lo, hi = a - 1.0, a.copy()
    live = np.isfinite(ell)
    accepted, n_evals = np.zeros(C, bool), np.zeros(C, int)
    for k in range(max_shrinks + 1):
        r = np.flatnonzero(live)
        if not len(r):
            break
        c, sn = _cs(a[r])
        th = m + x[r] * c[:, None] + nu[r] * sn[:, None]
        e, t = f(th, r)
        n_evals[r] += 1
        ok = e > logy[r]
        w = r[ok]
        theta[w], ell[w], target[w], accepted[w], live[w] = th[ok], e[ok], t[ok], True, False
        r = r[~ok]
        neg = a[r] < 0
        lo[r], hi[r] = np.where(neg, a[r], lo[r]), np.where(neg, hi[r], a[r])
        if k < max_shrinks:
            a[r] = lo[r] + (hi[r] - lo[r]) * u[r, 2 + k]
    return theta, ell, target, accepted, n_evals
