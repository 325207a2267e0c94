"""A numpy f64 restatement of the reference's MetropolisHastings.draw (eeyore/samplers/metropolis_hastings.py:41-73) with
a MultivariateNormalKernel proposal (eeyore/kernels/multivariate_normal_kernel.py): MultivariateNormal(theta,
scale_tril=L).sample() is theta + L z, and only the lower triangle of L counts.  ``symmetric=False`` adds
log q(theta | theta') - log q(theta' | theta), which is zero for this kernel, so one function serves both."""
import numpy as np

from tests.dist_restatement import mix_target_fn, tables
from tests.ram_restatement import spec_target


def mh_mvn_draw(target_fn, theta, target, L, z, u):
    """One draw from (theta, target) with the factor L and the given z, u.
    Returns (theta, target, accepted, log_rate)."""
    prop = theta + np.tril(L) @ z
    tp = target_fn(prop)
    log_rate = tp - target
    acc = bool(np.log(u) < log_rate)
    return (prop, tp, acc, log_rate) if acc else (np.asarray(theta), target, acc, log_rate)


def group_target(rec):
    """The log-target of a group of g16_mh_mvn_traces.npz: a mixture (weights / means / covs) or an MLP spec."""
    if "weights" in rec:
        return mix_target_fn(*tables(rec["weights"], rec["means"], rec["covs"], bool(rec["normalized"])))
    return spec_target(rec)
