"""Fixed metrics of ``HMC(metric=...)``: Stan's ``diag_e`` and ``dense_e``.

A metric states the inverse mass matrix Sigma = L L^T, an estimate of the target's covariance: the momentum is
p ~ N(0, Sigma^-1) and the kinetic energy p^T Sigma p / 2.  ``DiagMetric(scale)`` holds L = diag(scale) (the standard
deviations), ``DenseMetric(scale_tril)`` a lower-triangular L with a positive diagonal (a Cholesky factor of the covariance).
Two classes, because a bare tensor of shape [C, P] against [P, P] would not say which one it is."""
import torch

_REG, _REG_N = 1e-3, 5.0  # Stan's shrinkage of an estimated metric towards 1e-3 I, with the weight of five draws


def _draws(samples):
    """[n, C, P] draws of a ChainBuffer or a tensor."""
    if hasattr(samples, 'get_samples'):
        samples = samples.get_samples()
    if not torch.is_tensor(samples) or samples.dim() != 3 or samples.shape[0] < 2:
        shape = tuple(samples.shape) if torch.is_tensor(samples) else type(samples).__name__
        raise ValueError(f"from_samples needs [n, C, P] draws with n >= 2 (or a ChainBuffer of them), got {shape}")
    return samples


def _flat(x, per_chain):
    """[C or 1, m, P] from [n, C, P]: the draws of each chain, or all chains' draws pooled."""
    return x.permute(1, 0, 2) if per_chain else x.reshape(1, -1, x.shape[-1])


class DiagMetric:
    """L = diag(scale): ``scale`` [P] for all chains or [C, P] with one vector per chain, finite and > 0."""

    form = 'diag'

    def __init__(self, scale):
        if not torch.is_tensor(scale) or scale.dim() not in (1, 2) or scale.shape[-1] < 1 or scale.shape[0] < 1:
            shape = tuple(scale.shape) if torch.is_tensor(scale) else type(scale).__name__
            raise ValueError(f"DiagMetric: scale must be a [P] or [C, P] tensor, got {shape}")
        if not bool(torch.isfinite(scale).all()):
            raise ValueError("DiagMetric: scale has a non-finite entry")
        if not bool((scale > 0).all()):
            raise ValueError("DiagMetric: every scale must be positive")
        self.scale = scale.detach()

    @property
    def table(self):
        return self.scale

    @property
    def num_params(self):
        return int(self.scale.shape[-1])

    @property
    def per_chain(self):
        return self.scale.dim() == 2

    @classmethod
    def identity(cls, P, dtype=torch.float64, device=None):
        return cls(torch.ones(P, dtype=dtype, device=device))

    @classmethod
    def from_samples(cls, samples, per_chain=False):
        """Stan's regularised estimate from [n, C, P] draws (or a ChainBuffer): variances n/(n+5) s^2 + 1e-3 5/(n+5) with
        s^2 the sample variance (divisor n - 1) of all chains' draws pooled, or of each chain's own with ``per_chain``
        ([C, P]); n is the number of draws a variance is taken over.  Computed by torch on the draws' device."""
        x = _flat(_draws(samples), per_chain)
        n = x.shape[1]
        var = x.var(dim=1, unbiased=True)
        var = (n / (n + _REG_N)) * var + _REG * (_REG_N / (n + _REG_N))
        sd = var.sqrt()
        return cls(sd if per_chain else sd[0])


class DenseMetric:
    """A lower-triangular factor L with a positive diagonal: ``scale_tril`` [P, P] for all chains or [C, P, P] with one
    factor per chain; the lower triangle must be finite, the strict upper triangle is never read."""

    form = 'dense'

    def __init__(self, scale_tril):
        if (not torch.is_tensor(scale_tril) or scale_tril.dim() not in (2, 3) or scale_tril.shape[-1] < 1
                or scale_tril.shape[-1] != scale_tril.shape[-2] or scale_tril.shape[0] < 1):
            shape = tuple(scale_tril.shape) if torch.is_tensor(scale_tril) else type(scale_tril).__name__
            raise ValueError(f"DenseMetric: scale_tril must be a [P, P] or [C, P, P] tensor, got {shape}")
        if not bool(torch.isfinite(torch.tril(scale_tril)).all()):
            raise ValueError("DenseMetric: scale_tril has a non-finite entry in its lower triangle")
        if not bool((torch.diagonal(scale_tril, dim1=-2, dim2=-1) > 0).all()):
            raise ValueError("DenseMetric: scale_tril must have a positive diagonal")
        self.scale_tril = scale_tril.detach()

    @property
    def table(self):
        return self.scale_tril

    @property
    def num_params(self):
        return int(self.scale_tril.shape[-1])

    @property
    def per_chain(self):
        return self.scale_tril.dim() == 3

    @classmethod
    def identity(cls, P, dtype=torch.float64, device=None):
        return cls(torch.eye(P, dtype=dtype, device=device))

    @classmethod
    def from_samples(cls, samples, per_chain=False):
        """Stan's regularised estimate from [n, C, P] draws (or a ChainBuffer): the Cholesky factor (torch.linalg.cholesky,
        on the draws' device) of n/(n+5) S + 1e-3 5/(n+5) I with S the sample covariance (divisor n - 1) of all chains'
        draws pooled, or of each chain's own with ``per_chain`` ([C, P, P])."""
        x = _flat(_draws(samples), per_chain)
        n, P = x.shape[1], x.shape[2]
        d = x - x.mean(dim=1, keepdim=True)
        S = d.transpose(1, 2) @ d / (n - 1)
        S = (n / (n + _REG_N)) * S + _REG * (_REG_N / (n + _REG_N)) * torch.eye(P, dtype=x.dtype, device=x.device)
        L = torch.linalg.cholesky(S)
        return cls(L if per_chain else L[0])
