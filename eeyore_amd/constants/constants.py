"""``loss_functions`` and ``torch_to_np_types`` (eeyore/constants/constants.py:7,15-18).

Each loss is a small object: calling it evaluates the reference's formula with torch ops (so ``model.loss(out, y)``
keeps working in user code), while the samplers only read ``.code`` -- the likelihood code of the C ABI
(include/eeyore_amd.h: enum ey_lik) -- and run the fused kernels.

The regression losses (``gaussian_loss``, ``laplace_loss``, ``poisson_loss`` and their dict entries 'regression',
'robust_regression', 'count_regression') also carry ``.scale``, the fixed noise scale the plan is created with."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Laplace, Normal

from eeyore_amd.stats.loss import binary_cross_entropy

torch_to_np_types = {torch.float32: np.float32, torch.float64: np.float64}


class Loss:
    def __init__(self, name, code, fn, scale=None):
        self.name, self.code, self._fn, self.scale = name, code, fn, scale

    def __call__(self, output, target):
        return self._fn(output, target)

    def __repr__(self):
        scale = "" if self.scale is None else f", scale={self.scale}"
        return f"Loss({self.name!r}, code={self.code}{scale})"


def _bce_sum(probabilities, y):
    return binary_cross_entropy(probabilities, y, reduction='sum')


def _ce_sum(logits, y_onehot):
    return F.cross_entropy(logits, torch.argmax(y_onehot, 1), reduction='sum')


def _checked_scale(scale):
    scale = float(scale)
    if not math.isfinite(scale) or not scale > 0.0:
        raise ValueError(f"the likelihood scale must be finite and > 0, got {scale}")
    return scale


def gaussian_loss(scale=1.0):
    """``-Normal(output, scale).log_prob(target).sum()``: a Gaussian likelihood with one fixed noise scale for all outputs
    (likelihood code 2, EY_LIK_GAUSS_SUM)."""
    scale = _checked_scale(scale)
    return Loss('regression', 2, lambda out, y: -Normal(out, scale).log_prob(y).sum(), scale=scale)


def laplace_loss(scale=1.0):
    """``-Laplace(output, scale).log_prob(target).sum()``: the robust alternative (code 3, EY_LIK_LAPLACE_SUM)."""
    scale = _checked_scale(scale)
    return Loss('robust_regression', 3, lambda out, y: -Laplace(out, scale).log_prob(y).sum(), scale=scale)


def poisson_loss():
    """``nn.PoissonNLLLoss(log_input=True, full=False, reduction='sum')``: the network output is the log-rate and the
    ``log(target!)`` term is left out, so ``-loss`` is the Poisson log-density up to a constant in the target (code 4,
    EY_LIK_POISSON_SUM)."""
    return Loss('count_regression', 4, lambda out, y: F.poisson_nll_loss(out, y, log_input=True, full=False,
                                                                         reduction='sum'))


loss_functions = {
    'binary_classification': Loss('binary_classification', 0, _bce_sum),
    'multiclass_classification': Loss('multiclass_classification', 1, _ce_sum),
    'regression': gaussian_loss(1.0),
    'robust_regression': laplace_loss(1.0),
    'count_regression': poisson_loss(),
}
