"""Maximum mean discrepancy between two samples under a kernel (eeyore/stats/discrepancy.py:3-19): the reference's check of
a chain against a direct sample of a known target.

    biased:    sum_symm_K(x1) / n1^2 + sum_symm_K(x2) / n2^2 - 2 sum_K(x1, x2) / (n1 n2)              (diagonals included)
    unbiased:  sum_symm_K(x1) / (n1 (n1 - 1)) + sum_symm_K(x2) / (n2 (n2 - 1)) - 2 sum_K(x1, x2) / (n1 n2)   (without them)

The samples are lists of [p] tensors or [n, p] tensors, on any device (``kernels.Kernel``).  For every chain of a stored run
at once, and for the curve against the number of draws, see ``stats.batched.mmd_chains`` / ``ChainBuffer.mmd``."""
import torch


def squared_mmd(x1, x2, kernel, biased=True):
    n1, n2 = len(x1), len(x2)
    sums = kernel._pair_sums(x1, x2, biased) if hasattr(kernel, "_pair_sums") else None
    if sums is not None:   # samples on the ROCm device under one of the three homogeneous kernels: all three sums from one launch
        first = x1[0]
        d1, d2 = (n1 ** 2, n2 ** 2) if biased else (n1 * (n1 - 1), n2 * (n2 - 1))
        return (sums[0] / d1 + sums[1] / d2 - 2 * sums[2] / (n1 * n2)).reshape(1).to(first.dtype)
    cross = 2 * kernel.sum_K(x1, x2) / (n1 * n2)
    if biased:
        return (kernel.sum_symm_K(x1, include_diag=True) / (n1 ** 2)
                + kernel.sum_symm_K(x2, include_diag=True) / (n2 ** 2) - cross)
    return (kernel.sum_symm_K(x1, include_diag=False) / (n1 * (n1 - 1))
            + kernel.sum_symm_K(x2, include_diag=False) / (n2 * (n2 - 1)) - cross)


def mmd(x1, x2, kernel):
    """sqrt of the biased estimate, not clamped (as the reference): the estimate is >= 0 in exact arithmetic, but where the
    two samples coincide its three terms cancel to rounding, which can leave a tiny negative number and so NaN."""
    return torch.sqrt(squared_mmd(x1, x2, kernel, biased=True))
