"""A numpy restatement of the reference's MALA.draw (eeyore/samplers/mala.py:46-82) with a MultivariateNormalKernel
proposal (eeyore/kernels/multivariate_normal_kernel.py), op for op: the proposal MultivariateNormal(loc, scale_tril=L).sample()
is loc + L z around loc = theta + step/2 grad (:35-36), the log-rate takes both proposal log-densities as torch's
MultivariateNormal.log_prob computes them (-(P log 2 pi + |L^-1 d|^2) / 2 - sum log L_ii, each by one forward substitution),
and only the lower triangle of L counts.  The arithmetic runs in the dtype of ``theta`` (f64 in the tests; f32 where a test
needs the reference arithmetic's own f32 error)."""
import numpy as np

from oracle import mlp_oracle as orc
from tests.dist_restatement import mix_value_grad_fn, tables


def forward_solve(L, r):
    """y with L y = r by column-oriented forward substitution, reading j <= i of L only."""
    r = np.array(r)
    P = r.shape[0]
    y = np.empty_like(r)
    for j in range(P):
        y[j] = r[j] / L[j, j]
        r[j + 1:] = r[j + 1:] - L[j + 1:, j] * y[j]
    return y


def mvn_log_prob(L, loc, x):
    """MultivariateNormal(loc, scale_tril=L).log_prob(x) (torch/distributions/multivariate_normal.py)."""
    dt = x.dtype.type
    P = x.shape[0]
    y = forward_solve(L, x - loc)
    half_log_det = dt(0)
    for j in range(P):
        half_log_det = half_log_det + np.log(L[j, j])
    return dt(-0.5) * (dt(P * np.log(2 * np.pi)) + np.dot(y, y)) - half_log_det


def mala_mvn_draw(value_and_grad, theta, target, grad, L, z, u, step):
    """One draw from (theta, target, grad) with the factor L, the step and the given z, u.
    Returns (theta, target, grad, accepted, log_rate)."""
    theta = np.asarray(theta)
    dt = theta.dtype.type
    P = theta.shape[0]
    loc = theta + dt(0.5) * dt(step) * grad
    Lz = np.zeros(P, theta.dtype)
    for j in range(P):                     # the lower triangle only, a column at a time
        Lz[j:] = Lz[j:] + L[j:, j] * z[j]
    prop = loc + Lz
    tp, gp = value_and_grad(prop)
    log_rate = tp - target                 # mala.py:58
    log_rate = log_rate - mvn_log_prob(L, loc, prop)    # :60
    loc2 = prop + dt(0.5) * dt(step) * gp                # :62
    log_rate = log_rate + mvn_log_prob(L, loc2, theta)  # :64
    acc = bool(np.log(u) < log_rate)
    return (prop, tp, gp, acc, log_rate) if acc else (theta, target, grad, acc, log_rate)


def group_value_grad(rec):
    """(log-target, gradient) of a group of g17_mala_mvn_traces.npz: a mixture (weights / means / covs) or an MLP spec."""
    if "weights" in rec:
        return mix_value_grad_fn(*tables(rec["weights"], rec["means"], rec["covs"], bool(rec["normalized"])))
    spec = orc.Spec(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), mu=rec["prior_mu"],
                    sigma=rec["prior_sigma"])
    x, y = np.asarray(rec["x"], np.float64), np.asarray(rec["y"], np.float64)

    def fn(th):
        t, g = orc.upto_grad_log_target(spec, np.asarray(th, np.float64), x, y)
        return float(t), g
    return fn
