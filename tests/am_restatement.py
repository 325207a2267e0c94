"""A numpy f64 restatement of the reference's AM.draw (eeyore/samplers/am.py:61-107) with the transform cov + eps I, and
``chol_left``, the left-looking column Cholesky of the kernel k_am (eeyore_amd/csrc/ey_generic.hip) in its
summation order, written as plain numpy loops."""
import numpy as np

from tests.ram_restatement import spec_target  # noqa: F401  (re-exported: the fixture groups carry the same spec keys)


def chol_left(A):
    """(L, broke): column j of L from A[i,j] - sum_{k<j} L[i,k] L[j,k] (k ascending), the pivot tested for `> 0` (NaN
    fails), the column scaled by the reciprocal of the pivot's root.  Only the lower triangle of A is read.  On a
    breakdown the columns from the failing one on are left as zeros."""
    A = np.asarray(A, np.float64)
    P = A.shape[0]
    L = np.zeros((P, P))
    for j in range(P):
        acc = np.zeros(P - j)
        for k in range(j):  # k ascending, one product added at a time: the kernel's order for every row i >= j
            acc = acc + L[j:, k] * L[j, k]
        s = A[j:, j] - acc
        d = s[0]
        if not d > 0:
            return L, True
        piv = np.sqrt(d)
        rp = 1.0 / piv
        L[j, j] = piv
        L[j + 1:, j] = s[1:] * rp
    return L, False


def am_draw(log_target, theta, target, mean, cov_sum, cov, num_accepted, cov0, z, u_mix, u, idx, offset, l, b, c, t0,
            eps):
    """One AM.draw at counter index ``idx``.  ``cov0`` is the transformed initial covariance; ``u_mix`` is looked at only
    when n = idx + 1 - offset > t0.  Returns a dict: the six state entries, accepted, log_rate, branch (0 isotropic,
    1 factor, 2 breakdown) and the proposal."""
    P = theta.shape[0]
    n = idx + 1 - offset
    branch = 0
    if n > t0 and not u_mix < l:  # am.py:68-73
        L, broke = chol_left(cov)
        branch = 2 if broke else 1
    prop = theta + (b * L) @ z if branch == 1 else theta + c * z
    tp = log_target(prop)
    log_rate = tp - target
    acc = bool(np.log(u) < log_rate)  # :80
    if acc:
        theta, target = prop, tp
        if idx > 0:  # :85
            num_accepted += 1
    mean = ((n - 1) * mean + theta) / n  # :91-93
    cov_sum = cov_sum + np.outer(theta, theta)  # :94
    if n >= t0:  # :95-101
        if num_accepted == 0:
            cov = cov0.copy()
        else:
            cov = (cov_sum - n * np.outer(mean, mean)) / (n - 1) + eps * np.eye(P)
    return dict(theta=theta, target=target, mean=mean, cov_sum=cov_sum, cov=cov, num_accepted=num_accepted, accepted=acc,
                log_rate=log_rate, branch=branch, proposal=prop)
