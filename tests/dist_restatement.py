"""A numpy f64 restatement of the Gaussian-mixture target of ey_plan_create_mixture (mix_target in
eeyore_amd/csrc/ey_generic.hip) and of single HMC / MALA / MH draws of the reference
(eeyore/samplers/hmc.py:100-156, mala.py:46-82, metropolis_hastings.py:41-73) written against a ``log_target`` /
``value_and_grad`` callable.  RAM and AM draws are ``ram_restatement.ram_draw`` and ``am_restatement.am_draw``."""
import numpy as np


def tables(weights, means, covs, normalized=True):
    """(c [M], mean [M, P], prec [M, P, P]) as eeyore_amd.models.targets computes them."""
    w = np.asarray(weights, np.float64)
    mean = np.asarray(means, np.float64)
    cov = np.asarray(covs, np.float64)
    P = mean.shape[1]
    prec = np.empty_like(cov)
    c = np.log(w)
    for k in range(len(w)):
        inv = np.linalg.inv(cov[k])
        prec[k] = (inv + inv.T) / 2
        if normalized:
            c[k] -= 0.5 * (P * np.log(2 * np.pi) + np.linalg.slogdet(cov[k])[1])
    return c, mean, prec


def mix_value_grad(c, mean, prec, theta, temperature=None):
    """(log p, grad log p) at theta [P]:  a_k = c_k - d_k . Lambda_k d_k / 2,  log p = A + log sum exp(a_k - A),
    grad = -(sum_k exp(a_k - A) Lambda_k d_k) / s; M = 1 takes no exp / log.  A NaN or an all -inf a gives NaN."""
    c, mean, prec = (np.asarray(a, np.float64) for a in (c, mean, prec))
    th = np.asarray(theta, np.float64)
    with np.errstate(all="ignore"):
        d = th[None, :] - mean                       # [M, P]
        v = np.einsum("kij,kj->ki", prec, d)         # [M, P]
        a = c - 0.5 * np.einsum("ki,ki->k", d, v)
        if len(c) == 1:
            val, g = a[0], -v[0]
        else:
            A = np.max(a)                            # propagates a NaN
            e = np.exp(a - A)
            s = e.sum()
            val, g = A + np.log(s), -(e @ v) / s
        if temperature is not None:
            val, g = val * temperature, g * temperature
    return float(val), g


def mix_target_fn(c, mean, prec, temperature=None):
    return lambda th: mix_value_grad(c, mean, prec, th, temperature)[0]


def mix_value_grad_fn(c, mean, prec, temperature=None):
    return lambda th: mix_value_grad(c, mean, prec, th, temperature)


def hmc_draw(value_and_grad, theta, target, grad, p0, u, step, L):
    """One HMC.draw from the cached (target, grad) with momentum p0 and accept variate u (hmc.py:100-156).
    Returns (theta, target, grad, accepted, rate, h_cur, h_prop)."""
    th, p = np.array(theta, np.float64), np.array(p0, np.float64)
    h_cur = -target + 0.5 * np.dot(p, p)
    p = p + 0.5 * step * grad
    t, g = target, grad
    for k in range(1, L + 1):
        th = th + step * p
        t, g = value_and_grad(th)
        p = p + (step if k < L else 0.5 * step) * g
    h_prop = -t + 0.5 * np.dot(p, p)
    with np.errstate(over="ignore", invalid="ignore"):
        rate = min(1.0, float(np.exp(h_cur - h_prop))) if not np.isnan(h_cur - h_prop) else float("nan")
    acc = bool(u < rate)
    return (th, t, g, acc, rate, h_cur, h_prop) if acc else (np.asarray(theta), target, grad, acc, rate, h_cur, h_prop)


def mala_draw(value_and_grad, theta, target, grad, z, u, step):
    """One MALA.draw (mala.py:46-82).  Returns (theta, target, grad, accepted, log_rate)."""
    sc = np.sqrt(step)
    loc = theta + 0.5 * step * grad
    prop = loc + sc * z
    tp, gp = value_and_grad(prop)
    loc2 = prop + 0.5 * step * gp
    qf, qb = np.dot(prop - loc, prop - loc), np.dot(theta - loc2, theta - loc2)
    log_rate = (tp - target) + qf / (2 * sc * sc) - qb / (2 * sc * sc)
    acc = bool(np.log(u) < log_rate)
    return (prop, tp, gp, acc, log_rate) if acc else (np.asarray(theta), target, grad, acc, log_rate)


def mh_draw(log_target, theta, target, z, u, scale):
    """One MetropolisHastings.draw with the Normal random-walk kernel (metropolis_hastings.py:41-73).
    Returns (theta, target, accepted, log_rate)."""
    prop = theta + scale * z
    tp = log_target(prop)
    log_rate = tp - target
    acc = bool(np.log(u) < log_rate)
    return (prop, tp, acc, log_rate) if acc else (np.asarray(theta), target, acc, log_rate)


def mix_value_grad_batch(c, mean, prec, theta):
    """mix_value_grad for theta [C, P] at once (finite points): ([C], [C, P])."""
    d = theta[:, None, :] - mean[None]                   # [C, M, P]
    v = np.einsum("kij,ckj->cki", prec, d)
    a = c[None] - 0.5 * np.einsum("cki,cki->ck", d, v)
    if len(c) == 1:
        return a[:, 0], -v[:, 0]
    A = a.max(1, keepdims=True)
    e = np.exp(a - A)
    s = e.sum(1, keepdims=True)
    return (A + np.log(s))[:, 0], -np.einsum("ck,cki->ci", e, v) / s


def hmc_chains(c, mean, prec, theta0, step, L, n_burn, n_keep, rng):
    """hmc_draw for C chains at once with draws from ``rng``: the kept samples [n_keep, C, P]."""
    th = np.array(theta0, np.float64)
    t, g = mix_value_grad_batch(c, mean, prec, th)
    keep = np.empty((n_keep,) + th.shape)
    for it in range(n_burn + n_keep):
        p = rng.standard_normal(th.shape)
        u = rng.random(th.shape[0])
        h_cur = -t + 0.5 * (p * p).sum(1)
        q, tq, gq = th, t, g
        p = p + 0.5 * step * gq
        for k in range(1, L + 1):
            q = q + step * p
            tq, gq = mix_value_grad_batch(c, mean, prec, q)
            p = p + (step if k < L else 0.5 * step) * gq
        h_prop = -tq + 0.5 * (p * p).sum(1)
        acc = u < np.minimum(1.0, np.exp(h_cur - h_prop))
        th = np.where(acc[:, None], q, th)
        t = np.where(acc, tq, t)
        g = np.where(acc[:, None], gq, g)
        if it >= n_burn:
            keep[it - n_burn] = th
    return keep


def random_mixture(P, M, seed, spread=2.0, normalized=True):
    """A reproducible well-conditioned mixture: (weights, means, covs, normalized)."""
    rng = np.random.default_rng(seed)
    w = 0.5 + rng.random(M)
    means = spread * rng.standard_normal((M, P))
    covs = np.empty((M, P, P))
    for k in range(M):
        A = rng.standard_normal((P, P)) / np.sqrt(P)
        S = A @ A.T + (0.5 + 0.5 * rng.random()) * np.eye(P)
        covs[k] = (S + S.T) / 2
    return w, means, covs, normalized
