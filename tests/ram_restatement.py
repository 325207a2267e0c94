"""A numpy f64 restatement of the reference's RAM.draw (eeyore/samplers/ram.py:38-70), literal: the factor is
re-factorised with a full Cholesky after every draw.  ``closed_form_update`` is the per-row sweep the kernel k_ram
implements (eeyore_amd/csrc/ey_generic.hip), written as plain numpy loops."""
import numpy as np

from oracle import mlp_oracle as orc


def adapt_h(P, n, g):
    """h = min(1, P n^-g) (ram.py:59) as Python computes it."""
    return min(1, P * n ** (-g))


def alpha_of(log_rate):
    """min(1, exp(log_rate)) as Python's min takes it (ram.py:62): a NaN log-rate gives 1, -inf gives 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = float(np.exp(log_rate))
    return min(1, e)


def refactorised(chol, z, beta):
    """chol(S (I + beta z z^T / |z|^2) S^T) (ram.py:60-63)."""
    P = chol.shape[0]
    M = chol @ (np.eye(P) + beta * np.outer(z, z) / np.dot(z, z)) @ chol.T
    return np.linalg.cholesky(M)


def closed_form_update(S, z, beta):
    """S L_w with L_w = chol(I + beta w w^T), w = z / |z|, one backward sweep per row (the kernel's arithmetic):
    t_k = 1 + beta sum_{j<=k} w_j^2, d_k = sqrt(t_k / t_{k-1}), g_k = beta w_k / sqrt(t_{k-1} t_k),
    S'[i,k] = d_k S[i,k] + g_k sum_{k<j<=i} S[i,j] w_j."""
    P = S.shape[0]
    w = z / np.sqrt(np.dot(z, z))
    d, gm = np.empty(P), np.empty(P)
    for k in range(P):
        pre = 0.0
        for j in range(k):
            pre += w[j] * w[j]
        t0, t1 = 1.0 + beta * pre, 1.0 + beta * (pre + w[k] * w[k])
        d[k], gm[k] = np.sqrt(t1 / t0), beta * w[k] / np.sqrt(t0 * t1)
    out = np.zeros_like(S)
    for i in range(P):
        r = 0.0
        for k in range(i, -1, -1):
            out[i, k] = d[k] * S[i, k] + gm[k] * r
            r += S[i, k] * w[k]
    return out


def ram_draw(log_target, theta, target, chol, z, u, n, a, g):
    """One RAM.draw from (theta, target, chol) with the given z, u and adaptation index n.
    Returns (theta, target, chol, accepted, log_rate)."""
    P = theta.shape[0]
    prop = theta + chol @ z
    tp = log_target(prop)
    log_rate = tp - target
    acc = bool(np.log(u) < log_rate)
    beta = adapt_h(P, n, g) * (alpha_of(log_rate) - a)
    new_chol = refactorised(chol, z, beta)
    return (prop, tp, new_chol, acc, log_rate) if acc else (theta, target, new_chol, acc, log_rate)


def spec_target(rec, temperature=None):
    spec = orc.Spec(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), mu=rec["prior_mu"],
                    sigma=rec["prior_sigma"], temperature=temperature)
    x, y = np.asarray(rec["x"], np.float64), np.asarray(rec["y"], np.float64)
    return lambda th: float(orc.log_target(spec, np.asarray(th, np.float64), x, y))
