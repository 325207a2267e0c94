"""Closed-form target densities for ``DistributionModel``: a multivariate normal or a mixture of them.

The reference's ``DistributionModel`` takes any Python closure ``log_pdf(theta, x, y)``
(eeyore/models/distribution_model.py:6-28); a closure cannot be a HIP kernel.  The densities of the reference's own
distribution examples are all of one family, whose value and gradient have closed forms, so that family is what the
kernels serve.  A target object holds the host tables the plan is created from (numpy double, rounded
once to the model's dtype by the library) and is callable as ``log_pdf(theta, x, y)`` with torch ops, the way
``constants.Loss`` can be called.
"""
import math

import numpy as np
import torch


class NormalMixture:
    """log p(theta) = log sum_k exp(c_k - (theta - m_k)^T inv(S_k) (theta - m_k) / 2) on theta in R^P.

    ``normalized=True``: c_k = log w_k - log det(2 pi S_k) / 2 (the weights as given: they need not sum to one);
    ``normalized=False``: c_k = log w_k -- the reference's mixture example
    ``log(exp(-|theta - m_0|^2 / 2) + exp(-|theta - m_1|^2 / 2))`` is ``weights=[1, 1]`` with identity covariances."""

    def __init__(self, weights, means, covs, normalized=True):
        try:
            w = np.asarray(_host(weights), dtype=np.float64)
            mean = np.asarray(_host(means), dtype=np.float64)
            cov = np.asarray(_host(covs), dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"weights, means and covs must be numeric arrays: {err}") from None
        if w.ndim != 1 or w.size < 1:
            raise ValueError(f"weights must be a vector with one entry per component, got shape {w.shape}")
        M = w.size
        if mean.ndim != 2 or mean.shape[0] != M or mean.shape[1] < 1:
            raise ValueError(f"means must be [{M}, P], got shape {mean.shape}")
        P = mean.shape[1]
        if cov.shape != (M, P, P):
            raise ValueError(f"covs must be [{M}, {P}, {P}], got shape {cov.shape}")
        if not (np.all(np.isfinite(w)) and np.all(w > 0)):
            raise ValueError("every weight must be a finite number > 0")
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))):
            raise ValueError("means and covs must be finite")
        prec = np.empty_like(cov)
        c = np.log(w)
        for k in range(M):
            if not np.array_equal(cov[k], cov[k].T):
                raise ValueError(f"covs[{k}] is not symmetric")
            try:
                chol = np.linalg.cholesky(cov[k])
                inv = np.linalg.inv(cov[k])
            except np.linalg.LinAlgError as err:
                raise ValueError(f"covs[{k}] cannot be factorised ({err}): a covariance must be positive definite") from None
            prec[k] = (inv + inv.T) / 2
            if normalized:  # log det(2 pi S) = P log(2 pi) + 2 sum log diag(chol)
                c[k] -= 0.5 * (P * math.log(2 * math.pi) + 2 * np.log(np.diag(chol)).sum())
        self.weights, self.means, self.covs, self.normalized = w, mean, cov, bool(normalized)
        self.c, self.prec = c, prec
        self.M, self.P = M, P
        self._cache = {}

    def _tables(self, like):
        key = (like.dtype, like.device)
        if key not in self._cache:
            self._cache[key] = tuple(torch.as_tensor(a).to(device=like.device, dtype=like.dtype)
                                     for a in (self.c, self.means, self.prec))
        return self._cache[key]

    def __call__(self, theta, x=None, y=None):
        """theta [P] -> 0-d tensor, theta [C, P] -> [C]; differentiable torch ops in theta's dtype on its device."""
        c, mean, prec = self._tables(theta)
        d = theta.unsqueeze(-2) - mean                      # [..., M, P]
        v = torch.einsum('kij,...kj->...ki', prec, d)
        a = c - 0.5 * (d * v).sum(-1)                       # [..., M]
        return a[..., 0] if self.M == 1 else torch.logsumexp(a, dim=-1)

    def __repr__(self):
        return f"{type(self).__name__}(M={self.M}, P={self.P}, normalized={self.normalized})"


class MultivariateNormal(NormalMixture):
    """One component: log N(theta; mean, cov), or with ``normalized=False`` the kernel -(theta - mean)^T inv(cov)
    (theta - mean) / 2 alone."""

    def __init__(self, mean, cov, normalized=True):
        mean = np.asarray(_host(mean), dtype=np.float64)
        cov = np.asarray(_host(cov), dtype=np.float64)
        if mean.ndim != 1:
            raise ValueError(f"mean must be a vector [P], got shape {mean.shape}")
        if cov.ndim != 2:
            raise ValueError(f"cov must be a matrix [P, P], got shape {cov.shape}")
        super().__init__([1.0], mean[None], cov[None], normalized=normalized)


def _host(a):
    if torch.is_tensor(a):
        return a.detach().cpu().numpy()
    if isinstance(a, (list, tuple)) and len(a) and torch.is_tensor(a[0]):
        return [t.detach().cpu().numpy() for t in a]
    return a


TARGETS = (NormalMixture, MultivariateNormal)
