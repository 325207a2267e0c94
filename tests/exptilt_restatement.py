"""A numpy f64 restatement of the exponential-tilt target of ey_plan_create_exptilt (tilt_target in
eeyore_amd/csrc/ey_generic.hip):

    log p(theta) = sum_i [c_i + a_i theta_i - b_i exp(s_i theta_i)],   d/dtheta_i = a_i - b_i s_i exp(s_i theta_i)

The closures below go into the draw functions of tests/dist_restatement.py (hmc_draw, mala_draw, mh_draw),
ram_restatement.ram_draw, am_restatement.am_draw, mh_mvn_restatement.mh_mvn_draw and mala_mvn_restatement.mala_mvn_draw."""
import math

import numpy as np

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def tilt_value_grad(c, a, b, s, theta, temperature=None):
    """(log p, grad log p, S) at theta [P], S = sum_i (|c_i| + |a_i theta_i| + |b_i exp(s_i theta_i)|) being the size of the
    terms the value is summed from (what a tolerance on the value is relative to: terms of both signs cancel).  Nothing is
    clamped: an overflowing exp gives the value -inf and the gradient component -sign(s_i) inf, an underflowing one the
    component a_i exactly, a NaN coordinate a NaN value and component."""
    c, a, b, s = (np.asarray(t, np.float64) for t in (c, a, b, s))
    th = np.asarray(theta, np.float64)
    with np.errstate(all="ignore"):
        be = b * np.exp(s * th)
        val = np.sum(c + a * th - be)
        g = a - be * s
        S = np.sum(np.abs(c) + np.abs(a * th) + np.abs(be))
        if temperature is not None:
            val, g = val * temperature, g * temperature
    return float(val), g, float(S)


def tilt_target_fn(c, a, b, s, temperature=None):
    return lambda th: tilt_value_grad(c, a, b, s, th, temperature)[0]


def tilt_value_grad_fn(c, a, b, s, temperature=None):
    return lambda th: tilt_value_grad(c, a, b, s, th, temperature)[:2]


def tilt_value_grad_batch(c, a, b, s, theta):
    """tilt_value_grad for theta [C, P] at once: ([C], [C, P])."""
    with np.errstate(all="ignore"):
        be = b * np.exp(s * theta)
        return np.sum(c + a * theta - be, axis=1), a - be * s


def random_tilt(P, seed):
    """Reproducible tables (c, a, b, s) [P] with mixed signs of s: |s| in [0.5, 2], a / s in [0.5, 4], b in [0.3, 3]."""
    rng = np.random.default_rng(seed)
    s = (0.5 + 1.5 * rng.random(P)) * np.where(rng.random(P) < 0.5, -1.0, 1.0)
    a = (0.5 + 3.5 * rng.random(P)) * s
    b = 0.3 + 2.7 * rng.random(P)
    c = rng.standard_normal(P)
    return c, a, b, s


def mode(tables):
    """The mode of every coordinate: ln(a / (b s)) / s."""
    c, a, b, s = tables
    return np.log(a / (b * s)) / s


# ---- the tables of the named constructors of eeyore_amd.models.targets, written out once more
def log_gamma(shape, scale, normalized=True):
    k, t = (np.atleast_1d(np.asarray(v, np.float64)) for v in np.broadcast_arrays(shape, scale))
    c = -_lgamma(k) - k * np.log(t) if normalized else np.zeros_like(k)
    return c, k.copy(), 1.0 / t, np.ones_like(k)


def log_inverse_gamma(shape, rate, normalized=True):
    k, r = (np.atleast_1d(np.asarray(v, np.float64)) for v in np.broadcast_arrays(shape, rate))
    c = k * np.log(r) - _lgamma(k) if normalized else np.zeros_like(k)
    return c, -k, r.copy(), -np.ones_like(k)


def log_weibull(scale, concentration, normalized=True):
    lam, k = (np.atleast_1d(np.asarray(v, np.float64)) for v in np.broadcast_arrays(scale, concentration))
    c = np.log(k) - k * np.log(lam) if normalized else np.zeros_like(k)
    return c, k.copy(), lam ** -k, k.copy()


def gumbel(loc, scale, normalized=True):
    mu, beta = (np.atleast_1d(np.asarray(v, np.float64)) for v in np.broadcast_arrays(loc, scale))
    c = -np.log(beta) + mu / beta if normalized else np.zeros_like(mu)
    return c, -1.0 / beta, np.exp(mu / beta), -1.0 / beta


def concat_tables(*tabs):
    return tuple(np.concatenate([t[k] for t in tabs]) for k in range(4))


def mala_chains(tables, theta0, step, n_burn, n_keep, rng):
    """dist_restatement.mala_draw for C chains at once with draws from ``rng``: the kept samples [n_keep, C, P]."""
    th = np.array(theta0, np.float64)
    t, g = tilt_value_grad_batch(*tables, th)
    keep = np.empty((n_keep,) + th.shape)
    sc = np.sqrt(step)
    for it in range(n_burn + n_keep):
        z = rng.standard_normal(th.shape)
        u = rng.random(th.shape[0])
        loc = th + 0.5 * step * g
        prop = loc + sc * z
        tp, gp = tilt_value_grad_batch(*tables, prop)
        loc2 = prop + 0.5 * step * gp
        qf, qb = ((prop - loc) ** 2).sum(1), ((th - loc2) ** 2).sum(1)
        with np.errstate(invalid="ignore"):
            acc = np.log(u) < (tp - t) + qf / (2 * sc * sc) - qb / (2 * sc * sc)
        th = np.where(acc[:, None], prop, th)
        t = np.where(acc, tp, t)
        g = np.where(acc[:, None], gp, g)
        if it >= n_burn:
            keep[it - n_burn] = th
    return keep
