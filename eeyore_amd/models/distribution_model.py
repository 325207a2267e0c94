import torch
import torch.nn as nn

from .base import LogTargetModel
from .targets import ExponentialTilt, NormalMixture
from eeyore_amd.plan import Plan


class DistributionModel(LogTargetModel):
    """A plain density on theta with the reference's constructor, ``theta`` parameter and ``summary``
    (eeyore/models/distribution_model.py:6-28).  ``log_pdf`` must be one of ``eeyore_amd.models.targets``
    (``NormalMixture``, ``MultivariateNormal``, or an ``ExponentialTilt`` such as ``LogGamma``): an arbitrary closure has no
    HIP kernel.  ``log_target`` and
    ``upto_grad_log_target`` are one call into the library each, for one chain (theta [P]) or C chains ([C, P]); the data
    batch is ignored, as the reference's distribution closures ignore it."""

    def __init__(self, log_pdf, num_params, temperature=None, dtype=torch.float64, device='cpu', requires_grad=True):
        super().__init__(temperature=temperature, dtype=dtype, device=device)
        if not isinstance(log_pdf, (NormalMixture, ExponentialTilt)):
            raise ValueError("log_pdf must be one of eeyore_amd.models.targets (NormalMixture, MultivariateNormal, or an "
                             "ExponentialTilt such as LogGamma): the kernels implement Gaussian mixtures and separable "
                             "exponential tilts; an arbitrary Python closure cannot be a HIP kernel")
        if int(num_params) != log_pdf.P:
            raise ValueError(f"num_params = {num_params}, but the target is a density on R^{log_pdf.P}")
        self.log_pdf = log_pdf
        self.theta = nn.Parameter(
            data=torch.empty(num_params, dtype=self.dtype, device=self.device), requires_grad=requires_grad
        )
        object.__setattr__(self, "_hip_plan", None)

    def summary(self, hashsummary=False):
        print(self)
        print("-" * 80)
        print(f"Number of distribution parameters: {self.num_params()}")
        print("-" * 80)

    def _plan(self, x=None, y=None):
        """This model's C-ABI plan (``Plan.mixture`` or ``Plan.exp_tilt``); the batch is ignored."""
        plan = self._hip_plan
        if plan is None:
            t = self.log_pdf
            if isinstance(t, ExponentialTilt):
                plan = Plan.exp_tilt(t.c, t.a, t.b, t.s, self.dtype, self.device)
            else:
                plan = Plan.mixture(t.c, t.means, t.prec, self.dtype, self.device)
            object.__setattr__(self, "_hip_plan", plan)
        return plan

    def _evaluate(self, theta, grad):
        self.set_params(theta if theta.dim() == 1 else theta[0])  # distribution_model.py:21
        th = theta.detach()
        single = th.dim() == 1
        th = (th.unsqueeze(0) if single else th).to(device=self.device, dtype=self.dtype).contiguous()
        plan = self._plan()
        out = plan.log_target_grad(th, temp=self.temperature) if grad else (plan.log_target(th, temp=self.temperature)[0],)
        return tuple(o[0] for o in out) if single else out

    def log_target(self, theta, x=None, y=None):
        """theta [P] -> 0-d tensor; theta [C, P] -> [C]."""
        return self._evaluate(theta, False)[0]

    def upto_grad_log_target(self, theta, x=None, y=None):
        """theta [P] -> (0-d, [P]); theta [C, P] -> ([C], [C, P])."""
        return self._evaluate(theta, True)
