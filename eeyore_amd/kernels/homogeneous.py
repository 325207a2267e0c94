"""Kernels that are functions of the distance between their arguments, behind the reference's names
(``HomogeneousKernel``, ``IsoSEKernel``, ``RQKernel``, ``PeriodicKernel``; eeyore/kernels/{homogeneous,iso_se,rq,periodic}_kernel.py).

They are what ``stats.mmd`` judges a chain against a direct sample of its target with.  With d2 the squared Euclidean distance
in the difference form sum_j (a_j - b_j)^2 and d = sqrt(d2):

    IsoSEKernel(scale, l)        scale * exp(-d2 / (2 l))
    RQKernel(scale, l, a)        scale * (1 + d2 / (2 a l)) ** -a
    PeriodicKernel(scale, l, p)  scale * exp(-2 sin(d / p)^2 / l)

``K`` / ``symm_K`` / ``sum_K`` / ``sum_symm_K`` (``kernels.Kernel``) evaluate all pairs at once in f64 on whatever device the
samples are on and return the samples' dtype; the two sums of samples on the ROCm device run in the HIP kernel
``ey_kernel_pair_sums`` (one chain, no [n, n] matrix).  A subclass that overrides ``k`` goes pair by pair through its own ``k``."""
import ctypes as ct
import math

import torch

from .proposal import Kernel

_ROWS_AT_ONCE = 1 << 22   # elements of the [rows, n2, p] difference block the host path forms at a time


def as_matrix(x):
    """A sample as an [n, p] tensor: a list of [p] tensors is stacked, a tensor passes (a 1-d one as n points of p = 1)."""
    if not torch.is_tensor(x):
        x = torch.stack([torch.as_tensor(e).reshape(-1) for e in x])
    return x.reshape(-1, 1) if x.dim() == 1 else x


def pair_sqdist(x1, x2):
    """[n1, n2] squared distances in the difference form, in f64, a block of rows at a time."""
    a, b = as_matrix(x1).to(torch.float64), as_matrix(x2).to(torch.float64)
    rows = max(1, _ROWS_AT_ONCE // max(1, b.shape[0] * b.shape[1]))
    return torch.cat([(a[i:i + rows, None, :] - b[None, :, :]).pow(2).sum(-1) for i in range(0, a.shape[0], rows)])


class HomogeneousKernel(Kernel):
    """Base class of the kernels that depend on their arguments through the distance between them."""

    kind = None   # the code ey_kernel_pair_sums knows the kernel function by

    def dist(self, x1, x2):
        return torch.norm(x1 - x2, 2)

    def squared_dist(self, x1, x2):
        return self.dist(x1, x2).pow(2)

    def of_sqdist(self, d2):
        """The kernel function of a tensor of squared distances (the three kernels below define it)."""
        raise NotImplementedError

    def params(self):
        raise NotImplementedError

    def device_kind(self):
        """(kind, params) when the HIP kernel computes exactly this object's ``k``, else None: one of the three kernels
        below whose ``k`` and ``of_sqdist`` have not been overridden."""
        for base in (IsoSEKernel, RQKernel, PeriodicKernel):
            if isinstance(self, base) and type(self).k is base.k and type(self).of_sqdist is base.of_sqdist:
                return base.kind, [float(v) for v in self.params()]
        return None

    def _all_pairs(self, x1, x2):
        if self.device_kind() is None:
            return None
        return self.of_sqdist(pair_sqdist(x1, x2))

    def _pair_sums(self, x1, x2, include_diag):
        a = as_matrix(x1)
        # one call returns all three sums; where only x1's own is wanted, x2 is its first two rows: n + 3 more pairs, not n^2
        b = a[:2] if x2 is None else as_matrix(x2)
        if self.device_kind() is None or not (a.is_cuda and b.is_cuda) or a.dtype != b.dtype or a.shape[1] != b.shape[1]:
            return None
        if a.dtype not in (torch.float32, torch.float64) or (not include_diag and min(a.shape[0], b.shape[0]) < 2):
            return None
        s11, s22, s12 = pair_sums(a[None], b[None], self, layout="cnp", include_diag=include_diag)
        return s11[0, 0], s22[0, 0], s12[0, 0]


class IsoSEKernel(HomogeneousKernel):
    """Isotropic squared exponential kernel: ``scale`` the squared amplitude, ``l`` the squared length scale."""

    kind = 0

    def __init__(self, scale=1., l=1.):
        self.scale = scale
        self.l = l

    def params(self):
        return self.scale, self.l

    def of_sqdist(self, d2):
        return torch.exp(-d2 / (2. * self.l)) * self.scale

    def k(self, x1, x2):
        return self.of_sqdist(self.squared_dist(x1, x2))


class RQKernel(HomogeneousKernel):
    """Rational quadratic kernel: ``a`` > 0 the scale mixture."""

    kind = 1

    def __init__(self, scale=1., l=1., a=1.):
        self.scale = scale
        self.l = l
        self.a = a

    def params(self):
        return self.scale, self.l, self.a

    def of_sqdist(self, d2):
        return (d2 / (2. * self.a * self.l) + 1.).pow(-self.a) * self.scale

    def k(self, x1, x2):
        return self.of_sqdist(self.squared_dist(x1, x2))


class PeriodicKernel(HomogeneousKernel):
    """Periodic kernel: ``p`` a multiple of the period."""

    kind = 2

    def __init__(self, scale=1., l=1., p=2.):
        self.scale = scale
        self.l = l
        self.p = p

    def params(self):
        return self.scale, self.l, self.p

    def of_sqdist(self, d2):
        return torch.exp(-torch.sin(torch.sqrt(d2) / self.p).pow(2) * 2. / self.l) * self.scale

    def k(self, x1, x2):
        return self.of_sqdist(self.dist(x1, x2).pow(2))


def pair_sums(x1, x2, kernel, layout="ncp", lengths=None, lengths2=None, include_diag=True):
    """``ey_kernel_pair_sums`` on device tensors: x1 [n1, C, p] (``layout="ncp"``) or [C, n1, p] (``"cnp"``), x2 alike or
    [n2, p] shared by all chains -> (s11, s22, s12), each [C, k] f64 on the device (k = 1 without ``lengths``): the sums of the
    kernel over the pairs of x1's first lengths[t] rows, of x2's first lengths2[t] rows, and across the two.  Nothing is
    checked here beyond what the address arithmetic needs; the C entry point validates the rest."""
    from eeyore_amd import _lib as L
    kind, params = kernel.device_kind()
    x1 = x1.contiguous()
    x2 = x2.contiguous()
    if layout == "ncp":
        n1, C, p = x1.shape
        sn1, sc1 = C * p, p
    elif layout == "cnp":
        C, n1, p = x1.shape
        sn1, sc1 = p, n1 * p
    else:
        raise ValueError("layout must be 'ncp' or 'cnp'")
    if x2.dim() == 2:
        n2, sn2, sc2 = x2.shape[0], p, 0
    elif layout == "ncp":
        n2, sn2, sc2 = x2.shape[0], C * p, p
    else:
        n2, sn2, sc2 = x2.shape[1], p, x2.shape[1] * p
    k = 1 if lengths is None else len(lengths)
    if lengths is None:
        l1 = l2 = None
    else:
        l1 = (ct.c_int64 * k)(*[int(v) for v in lengths])
        l2 = (ct.c_int64 * k)(*[int(v) for v in (lengths2 if lengths2 is not None else [n2] * k)])
    out = torch.empty(3, C, k, dtype=torch.float64, device=x1.device)
    dt = {torch.float32: L.EY_F32, torch.float64: L.EY_F64}[x1.dtype]
    L.check(L.lib().ey_kernel_pair_sums(L.ptr(x1), n1, C, p, sn1, sc1, L.ptr(x2), n2, sn2, sc2, dt, kind,
                                        (ct.c_double * 3)(*(params + [math.nan])[:3]), l1, l2, k, int(bool(include_diag)),
                                        L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]),
                                        ct.c_void_p(torch.cuda.current_stream(x1.device).cuda_stream)),
            "ey_kernel_pair_sums")
    return out[0], out[1], out[2]
