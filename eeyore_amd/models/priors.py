"""From a ``torch.distributions`` prior to the tables of ``ey_plan_set_prior_family`` (include/eeyore_amd.h).

The reference sums ``prior.log_prob(theta)`` over the parameters for whatever distribution ``model.prior`` holds
(eeyore/models/bayesian_model.py:46-50).  The generic kernels evaluate the elementwise families below; a Cauchy prior is a
Student-t prior with one degree of freedom.
"""
import torch
from torch.distributions import Cauchy, Laplace, Normal, StudentT

from eeyore_amd import _lib as L
from eeyore_amd._lib import EY_PRIOR_LAPLACE, EY_PRIOR_NORMAL, EY_PRIOR_STUDENT_T  # noqa: F401  (re-exported)

FAMILIES = {Normal: L.EY_PRIOR_NORMAL, Laplace: L.EY_PRIOR_LAPLACE, StudentT: L.EY_PRIOR_STUDENT_T,
            Cauchy: L.EY_PRIOR_STUDENT_T}
FAMILY_NAMES = {L.EY_PRIOR_NORMAL: "Normal", L.EY_PRIOR_LAPLACE: "Laplace", L.EY_PRIOR_STUDENT_T: "StudentT"}
_ACCEPTED = "torch.distributions.Normal, Laplace, StudentT and Cauchy"


def prior_tables(prior, num_params):
    """``(family, loc, scale, df)`` of an elementwise prior over ``num_params`` parameters: ``family`` one of
    ``EY_PRIOR_NORMAL / _LAPLACE / _STUDENT_T``, ``loc`` and ``scale`` tensors of shape ``[num_params]`` (scalar parameters
    of the distribution are expanded), ``df`` one more for a Student-t or Cauchy prior (all ones for Cauchy) and ``None``
    otherwise.  ``ValueError`` for any other distribution class -- the exact classes count: a subclass, an ``Independent``
    wrapper or a mixture has another ``log_prob`` -- and for a batch shape other than ``[num_params]``."""
    family = FAMILIES.get(type(prior))
    if family is None:
        raise ValueError(f"a prior of type {type(prior).__name__} has no HIP kernel: the elementwise priors served are "
                         f"{_ACCEPTED} with batch shape [{num_params}]")
    # (a Normal prior of batch shape [] or [1] keeps broadcasting over the parameters, as it always has here)
    lenient = family == L.EY_PRIOR_NORMAL and tuple(prior.batch_shape) in ((), (1,))
    if (tuple(prior.batch_shape) != (num_params,) and not lenient) or tuple(prior.event_shape) != ():
        raise ValueError(f"the prior's batch shape must be [{num_params}] (one distribution per parameter), got "
                         f"{list(prior.batch_shape)}; the elementwise priors served are {_ACCEPTED}")
    shape = (num_params,)
    loc = torch.broadcast_to(prior.loc, shape)
    scale = torch.broadcast_to(prior.scale, shape)
    df = None
    if isinstance(prior, StudentT):
        df = torch.broadcast_to(prior.df, shape)
    elif isinstance(prior, Cauchy):
        df = torch.ones_like(scale)
    return family, loc, scale, df
