"""Closed-form target densities for ``DistributionModel``: a multivariate normal or a mixture of them, and the separable
exponential-tilt family of Gamma-type densities on the log scale.

The reference's ``DistributionModel`` takes any Python closure ``log_pdf(theta, x, y)``
(eeyore/models/distribution_model.py:6-28); a closure cannot be a HIP kernel.  The densities of the reference's own
distribution examples are of two families, whose values and gradients have closed forms, so those families are what the
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


class ExponentialTilt:
    """log p(theta) = sum_i [c_i + a_i theta_i - b_i exp(s_i theta_i)] on theta in R^P: separable over the coordinates, proper
    when b_i > 0, s_i != 0 and a_i / s_i > 0.  With theta = log x and the Jacobian included it is the density of a Gamma,
    inverse-Gamma or Weibull variable x; a Gumbel density has the form on theta itself (``LogGamma``, ``LogInverseGamma``,
    ``LogWeibull``, ``Gumbel`` build the tables; ``concat`` joins targets coordinate-wise).  ``a``, ``b``, ``s`` and ``c``
    (default 0: the unnormalised density) are scalars or [P] vectors, broadcast against each other."""

    def __init__(self, a, b, s, c=None):
        try:
            tabs = [np.asarray(_host(0.0 if t is None else t), dtype=np.float64) for t in (c, a, b, s)]
        except (TypeError, ValueError) as err:
            raise ValueError(f"a, b, s and c must be numeric scalars or vectors: {err}") from None
        if any(t.ndim > 1 for t in tabs):
            raise ValueError(f"a, b, s and c must be scalars or vectors [P], got shapes {[t.shape for t in tabs]}")
        try:
            c, a, b, s = (np.ascontiguousarray(t) for t in np.broadcast_arrays(*[np.atleast_1d(t) for t in tabs]))
        except ValueError:
            raise ValueError(f"a, b, s and c do not broadcast to one [P]: shapes {[t.shape for t in tabs]}") from None
        if c.size < 1:
            raise ValueError("the target needs at least one coordinate")
        for name, t in (("c", c), ("a", a), ("b", b), ("s", s)):
            if not np.all(np.isfinite(t)):
                raise ValueError(f"{name} must be finite")
        if not np.all(b > 0):
            raise ValueError(f"every b must be > 0, b[{int(np.argmax(~(b > 0)))}] is not")
        if np.any(s == 0):
            raise ValueError(f"every s must be != 0, s[{int(np.argmax(s == 0))}] is 0")
        if not np.all(a / s > 0):
            raise ValueError(f"every a / s must be > 0 (the density is not proper), a[{int(np.argmax(~(a / s > 0)))}] / s is not")
        self.c, self.a, self.b, self.s = c, a, b, s
        self.P = int(c.size)
        self._cache = {}

    def _tables(self, like):
        key = (like.dtype, like.device)
        if key not in self._cache:
            self._cache[key] = tuple(torch.as_tensor(t).to(device=like.device, dtype=like.dtype)
                                     for t in (self.c, self.a, self.b, self.s))
        return self._cache[key]

    def __call__(self, theta, x=None, y=None):
        """theta [P] -> 0-d tensor, theta [C, P] -> [C]; differentiable torch ops in theta's dtype on its device."""
        c, a, b, s = self._tables(theta)
        return (c + a * theta - b * torch.exp(s * theta)).sum(-1)

    def __repr__(self):
        return f"{type(self).__name__}(P={self.P})"


def _positive(**named):
    out = []
    for name, v in named.items():
        try:
            v = np.asarray(_host(v), dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"{name} must be numeric: {err}") from None
        if not (np.all(np.isfinite(v)) and np.all(v > 0)):
            raise ValueError(f"{name} must be finite and > 0")
        out.append(v)
    return out


_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


class LogGamma(ExponentialTilt):
    """theta = log x for x ~ Gamma(shape, scale): log p = shape theta - exp(theta) / scale (the reference's
    ``(v0 - 1) theta - exp(theta) / v1 + theta``), plus -lgamma(shape) - shape log(scale) when ``normalized``."""

    def __init__(self, shape, scale, normalized=True):
        k, t = _positive(shape=shape, scale=scale)
        super().__init__(k, 1.0 / t, 1.0, (-_lgamma(k) - k * np.log(t)) if normalized else None)
        self.normalized = bool(normalized)


class LogInverseGamma(ExponentialTilt):
    """theta = log x for x ~ InverseGamma(shape, rate): log p = -shape theta - rate exp(-theta), plus
    shape log(rate) - lgamma(shape) when ``normalized``."""

    def __init__(self, shape, rate, normalized=True):
        k, r = _positive(shape=shape, rate=rate)
        super().__init__(-k, r, -1.0, (k * np.log(r) - _lgamma(k)) if normalized else None)
        self.normalized = bool(normalized)


class LogWeibull(ExponentialTilt):
    """theta = log x for x ~ Weibull(scale, concentration k): log p = k theta - scale^-k exp(k theta), plus
    log k - k log(scale) when ``normalized``."""

    def __init__(self, scale, concentration, normalized=True):
        lam, k = _positive(scale=scale, concentration=concentration)
        super().__init__(k, lam ** -k, k, (np.log(k) - k * np.log(lam)) if normalized else None)
        self.normalized = bool(normalized)


class Gumbel(ExponentialTilt):
    """theta ~ Gumbel(loc, scale) itself: log p = -theta / scale - exp(loc / scale) exp(-theta / scale), plus
    -log(scale) + loc / scale when ``normalized``."""

    def __init__(self, loc, scale, normalized=True):
        (beta,) = _positive(scale=scale)
        try:
            mu = np.asarray(_host(loc), dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"loc must be numeric: {err}") from None
        if not np.all(np.isfinite(mu)):
            raise ValueError("loc must be finite")
        super().__init__(-1.0 / beta, np.exp(mu / beta), -1.0 / beta, (-np.log(beta) + mu / beta) if normalized else None)
        self.normalized = bool(normalized)


def concat(*targets):
    """One ``ExponentialTilt`` on the coordinates of the given ones, in the order given: a target that mixes families."""
    if not targets or not all(isinstance(t, ExponentialTilt) for t in targets):
        raise ValueError("concat takes one or more ExponentialTilt targets")
    return ExponentialTilt(*(np.concatenate([getattr(t, n) for t in targets]) for n in "abs"),
                           c=np.concatenate([t.c for t in targets]))


def _host(a):
    if torch.is_tensor(a):
        return a.detach().cpu().numpy()
    if isinstance(a, (list, tuple)) and len(a) and torch.is_tensor(a[0]):
        return [t.detach().cpu().numpy() for t in a]
    return a


TARGETS = (NormalMixture, MultivariateNormal, ExponentialTilt, LogGamma, LogInverseGamma, LogWeibull, Gumbel)
