import math

import torch

from .base import SingleChainSerialSampler, default_counter
from eeyore_amd.kernels import MultivariateNormalKernel, NormalKernel


class MALA(SingleChainSerialSampler):
    """Metropolis-adjusted Langevin algorithm (eeyore/samplers/mala.py:9-82) as one ``ey_mala_step`` per draw:
    proposal theta + step/2 grad + sqrt(step) z (the reference's default ``NormalKernel``, mala.py:35-41), one
    evaluation at the proposal, log-rate with both proposal densities, accept iff log u < log-rate.

    ``kernel`` may be a ``MultivariateNormalKernel``: its ``scale_tril`` L, ``[P, P]`` for all chains or ``[C, P, P]`` with
    one factor per chain, gives the proposal theta + step/2 grad + L z, one ``ey_mala_tril_step`` per draw (at most 128
    parameters).  ``step`` then enters the mean only: the proposal covariance is L L^T as given, the reference's semantics
    (mala.py:46-82 with kernel.sample / log_prob / set_density_params), not a preconditioned MALA.  The kernel's own
    ``loc`` is not used: the proposal is always centred at ``kernel_mean(current)``.  ``_set_tril(factors, index)`` is
    the one ``MetropolisHastings`` uses.  Any other user-supplied ``kernel`` has no HIP counterpart and is rejected."""

    keys = ['sample', 'target_val', 'grad_val', 'accepted']

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, step=0.1, kernel=None,
                 chain=None, rng=None, seed=0, chain_offset=0, temperature=None):
        super().__init__(default_counter(counter, dataloader))
        if kernel is not None and not isinstance(kernel, MultivariateNormalKernel):
            raise ValueError("MALA: only the default NormalKernel(theta + step/2 grad, sqrt(step)) proposal or a "
                             "MultivariateNormalKernel is fused into the HIP step")
        self._configure(model, dataloader, theta0, chain, rng, seed, chain_offset, temperature)
        self.step = step
        self._tril = self._tril_index = None
        if kernel is not None:
            self._set_tril(kernel.scale_tril)
        if theta0 is not None:
            self.set_current(theta0.clone().detach(), data=data0)

    def set_current(self, theta, data=None):
        x, y = super().set_current(theta, data=data)
        self._theta = self._state_tensor(theta)
        self._target, self._grad = self.model._plan(x, y).log_target_grad(self._theta, temp=self._temp())
        self._publish(torch.zeros(self.num_chains, dtype=torch.uint8))
        self.current['accepted'] = None

    def kernel_mean(self, state):
        return state['sample'] + 0.5 * self.step * state['grad_val']

    @property
    def kernel(self):
        """The proposal density at the current state, materialised on demand (the step itself never builds it)."""
        loc = self.kernel_mean(self.current)
        if self._tril is not None:
            idx = self._tril_index
            return MultivariateNormalKernel(loc, self._tril if idx is None else self._tril[idx.long()])
        return NormalKernel(loc, torch.full_like(loc, math.sqrt(self.step)))

    def _run_block(self, plan, k, rec):
        step, step_vec = self._step_args()
        if self._tril is not None:
            return plan.mala_tril_run(self._theta, self._target, self._grad, step, self._tril, k, index=self._tril_index,
                                      step_vec=step_vec, temp=self._temp(), seed=self.seed, it=self._iter,
                                      chain_offset=self.chain_offset, **rec)
        return plan.mala_run(self._theta, self._target, self._grad, step, k, step_vec=step_vec, temp=self._temp(),
                             seed=self.seed, it=self._iter, chain_offset=self.chain_offset, **rec)

    def draw(self, x, y, savestate=False):
        plan = self.model._plan(x, y)
        temp = self._temp()
        if self.counter.num_batches != 1:  # mala.py:49-51
            self._target, self._grad = plan.log_target_grad(self._theta, temp=temp)
        z, u = self._draw_randoms(*self._theta.shape)
        step, step_vec = self._step_args()
        if self._tril is not None:
            out = plan.mala_tril_step(self._theta, self._target, self._grad, step, self._tril, index=self._tril_index, z=z,
                                      u=u, step_vec=step_vec, temp=temp, seed=self.seed, it=self._iter,
                                      chain_offset=self.chain_offset)
        else:
            out = plan.mala_step(self._theta, self._target, self._grad, step, z=z, u=u, step_vec=step_vec, temp=temp,
                                 seed=self.seed, it=self._iter, chain_offset=self.chain_offset)
        self._finish_draw(out, savestate)
