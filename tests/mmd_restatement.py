"""numpy f64 restatement of what ey_kernel_pair_sums computes (include/eeyore_amd.h): the three sums of a homogeneous
kernel function over pairs of rows, for every prefix length.  Squared distances in the difference form, the full kernel
matrices built tile by tile with a loop over the pairs of tiles, prefix sums read off them.  No torch, and nothing of the
device kernel's bucket scheme: every prefix is summed on its own.  Also the tests' tolerance (``bound``)."""
import numpy as np

TILE = 32


def kfun(kind, params, d2):
    scale, l = params[0], params[1]
    if kind == 0:
        return scale * np.exp(-d2 / (2.0 * l))
    if kind == 1:
        a = params[2]
        return scale * (1.0 + d2 / (2.0 * a * l)) ** (-a)
    if kind == 2:
        return scale * np.exp(-2.0 * np.sin(np.sqrt(d2) / params[2]) ** 2 / l)
    raise ValueError(kind)


def kernel_matrix(a, b, kind, params):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(0, a.shape[0], TILE):
        for j in range(0, b.shape[0], TILE):
            d = a[i:i + TILE, None, :] - b[None, j:j + TILE, :]
            out[i:i + TILE, j:j + TILE] = kfun(kind, params, (d * d).sum(-1))
    return out


def symm_sum(m, n, include_diag):
    """The reference's sum_symm_K of the first n rows from their kernel matrix: pairs below the diagonal twice."""
    s = 2.0 * np.tril(m[:n, :n], -1).sum()
    return s + np.trace(m[:n, :n]) if include_diag else s


def pair_sums(x1, x2, kind, params, len1=None, len2=None, include_diag=True):
    """x1 [n1, p], x2 [n2, p] -> (s11 [k], s22 [k], s12 [k])."""
    len1 = [x1.shape[0]] if len1 is None else list(len1)
    len2 = [x2.shape[0]] if len2 is None else list(len2)
    m11, m22, m12 = kernel_matrix(x1, x1, kind, params), kernel_matrix(x2, x2, kind, params), kernel_matrix(x1, x2, kind, params)
    s11 = np.array([symm_sum(m11, a, include_diag) for a in len1])
    s22 = np.array([symm_sum(m22, b, include_diag) for b in len2])
    s12 = np.array([m12[:a, :b].sum() for a, b in zip(len1, len2)])
    return s11, s22, s12


def squared_mmd(s11, s22, s12, len1, len2, biased=True):
    a, b = np.asarray(len1, np.float64), np.asarray(len2, np.float64)
    if biased:
        return s11 / (a * a) + s22 / (b * b) - 2.0 * s12 / (a * b)
    return s11 / (a * (a - 1)) + s22 / (b * (b - 1)) - 2.0 * s12 / (a * b)


# Tolerance of a sum of N terms against another f64 evaluation of it (the fixture, or the restatement above).  Every term is
# >= 0 and <= scale.  A term's error has two sources: d2 carries up to p rounding errors, which the kernel function passes on
# multiplied by at most max x e^-x < 0.37 (IsoSE; the analogous factors of RQ and Periodic are <= 1), and exp / pow / sin /
# sqrt add a few ulp (8 allowed): (p + 8) ulp of scale per term.  Summing the N terms in any order adds at most N ulp of the
# partial sums on top, which the same allowance covers.  Hence |sum - sum'| <= N scale (p + 8) 2^-52, absolute.
ULP = 2.0 ** -52


def bound(n_terms, scale, p):
    return np.asarray(n_terms, np.float64) * scale * (p + 8) * ULP


def terms_symm(n, include_diag):
    n = np.asarray(n, np.float64)
    return n * n if include_diag else n * (n - 1)


def bound_squared_mmd(scale, p):
    """bound() pushed through squared_mmd's normalisers: each of s11 / N11, s22 / N22 carries scale (p + 8) 2^-52 (the
    normaliser is the number of terms, with or without the diagonal) and 2 s12 / (n1 n2) twice that."""
    return 4.0 * scale * (p + 8) * ULP
