import torch
from torch.distributions import Normal

from .base import ChainBuffer, SingleChainSerialSampler, default_counter
from eeyore_amd import _lib as L


class EllipticalSlice(SingleChainSerialSampler):
    """Elliptical slice sampling (Murray, Adams & MacKay 2010) as one ``ey_eslice_step`` per draw: a
    Gaussian base N(m, diag s^2) times exp(ell), sampled with no free parameter, no rejection and no gradient -- a draw
    shrinks an angle bracket on the ellipse through the state and a draw of the base until a point lies on the slice, one
    value-only evaluation per point, one wave per chain.

    ``base=None``: the model's elementwise Normal prior is the base (at a temperature t its scale is sigma / sqrt(t)) and
    ell the log-likelihood.  ``base``: a ``torch.distributions.Normal`` with one distribution per parameter, for any model
    the generic kernels hold in LDS -- a ``DistributionModel``, or an MLP under a Laplace, Student-t or Cauchy prior; ell is
    then the log-target minus the base's exponent, and the sampler is efficient where the base resembles the target.
    ``max_shrinks`` (at most 64) caps the shrinks of a draw; a chain whose bracket is exhausted stays where it is.

    ``theta0`` [C, P] or [P]; ``rng='torch'`` draws the normals and the draw's table of uniforms on the host (the word
    layout of include/eeyore_amd_eslice.h), ``rng='philox'`` uses the in-kernel streams.  ``accepted`` is 1 where the chain
    moved; ``last`` carries ``n_evals``, the evaluations of the last draw, and a chain whose keys include 'n_evals' records
    them."""

    keys = ['sample', 'target_val', 'accepted', 'n_evals']

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, base=None, max_shrinks=64, chain=None,
                 rng=None, seed=0, chain_offset=0, temperature=None):
        super().__init__(default_counter(counter, dataloader))
        if int(max_shrinks) != max_shrinks or not 1 <= max_shrinks <= L.EY_ESLICE_MAX_SHRINKS:
            raise ValueError(f"EllipticalSlice: max_shrinks must be an integer in [1, {L.EY_ESLICE_MAX_SHRINKS}]")
        self.max_shrinks = int(max_shrinks)
        P = model.num_params()
        self._base_loc = self._base_scale = None
        if base is None:
            if not hasattr(model, 'prior'):
                raise ValueError("EllipticalSlice: a model without a prior (a DistributionModel) has nothing to slice "
                                 "under; give base=torch.distributions.Normal(loc, scale)")
            if type(model.prior) is not Normal:  # (the exact class counts, as models.priors.prior_tables has it)
                raise ValueError(f"EllipticalSlice: without a base the model's prior must be an elementwise Normal (it is "
                                 f"{type(model.prior).__name__}); give base=torch.distributions.Normal(loc, scale)")
        else:
            if not isinstance(base, Normal):
                raise ValueError("EllipticalSlice: base must be a torch.distributions.Normal with one distribution per "
                                 "parameter")
            try:
                loc = torch.broadcast_to(base.loc.detach(), (P,))
                scale = torch.broadcast_to(base.scale.detach(), (P,))
            except RuntimeError:
                raise ValueError(f"EllipticalSlice: base must hold one distribution per parameter (batch shape "
                                 f"{tuple(base.batch_shape)}, the model has {P} parameters)") from None
            if not bool((torch.isfinite(scale) & (scale > 0)).all()) or not bool(torch.isfinite(loc).all()):
                raise ValueError("EllipticalSlice: the base's scale must be positive and finite and its location finite "
                                 "in every coordinate")
            self._base_loc = loc.to(device=model.device, dtype=model.dtype).contiguous().clone()
            self._base_scale = scale.to(device=model.device, dtype=model.dtype).contiguous().clone()
        self.base = base
        self._configure(model, dataloader, theta0, chain, rng, seed, chain_offset, temperature)
        if theta0 is not None:
            self.set_current(theta0.clone().detach(), data=data0)

    def _base(self):
        return dict(base_loc=self._base_loc, base_scale=self._base_scale)

    def _evaluate_target(self, plan):
        self._ell, self._target = plan.eslice_ell(self._theta, temp=self._temp(), **self._base())

    def set_current(self, theta, data=None):
        x, y = super().set_current(theta, data=data)
        self._theta = self._state_tensor(theta)
        self._evaluate_target(self.model._plan(x, y))
        self._publish(torch.zeros(self.num_chains, dtype=torch.uint8))
        self.current['accepted'] = None
        self.current['n_evals'] = None

    def set_temperature(self, temperature):
        """New temperatures [C] for the chains: the carried target is rescaled as every sampler's is; ell is re-evaluated
        at the next draw's start where it cannot be (with a base, ell is not a multiple of the temperature)."""
        old = self._temp()
        super().set_temperature(temperature)
        if getattr(self, '_ell', None) is None:
            return
        if self._base_loc is None:
            kw = dict(device=self._ell.device, dtype=self._ell.dtype)
            t_old = torch.ones((), **kw) if old is None else torch.as_tensor(old, **kw)
            new = self._temp()
            t_new = torch.ones((), **kw) if new is None else torch.as_tensor(new, **kw)
            self._ell *= (t_new / t_old).expand(self._ell.shape[0]).contiguous()
        else:
            self._stale = True

    def _publish_evals(self, out):
        self.current['n_evals'] = out['n_evals'] if self.batched else int(out['n_evals'][0].item())

    def _randoms(self, C, P):
        """(z [C, P], u [C, S]) from the global torch generator, or (None, None) for the in-kernel streams."""
        if self.rng != 'torch':
            return None, None
        return self._randn(C, P), torch.rand(C, 2 + self.max_shrinks, dtype=self.model.dtype, device=self.model.device)

    def _fresh(self, plan):
        if self.counter.num_batches != 1 or getattr(self, '_stale', False):  # ell and the target belong to another batch
            self._evaluate_target(plan)
            self._stale = False

    def draw(self, x, y, savestate=False):
        """One elliptical slice draw of every chain."""
        plan = self.model._plan(x, y)
        self._fresh(plan)
        z, u = self._randoms(*self._theta.shape)
        out = plan.eslice_step(self._theta, self._target, self._ell, z=z, u=u, max_shrinks=self.max_shrinks,
                               temp=self._temp(), seed=self.seed, it=self._iter, chain_offset=self.chain_offset,
                               **self._base())
        self._publish_evals(out)
        self._finish_draw(out, savestate)

    # -- blocks of draws per launch: the base class's loop on ey_eslice_run, with the record an EllipticalSlice chain may ask for
    def _can_fuse(self, verbose):
        return (self.fused_block > 0 and self.batched and self.rng == 'philox' and not verbose
                and self.counter.num_batches == 1 and isinstance(self.chain, ChainBuffer)
                and set(self.chain.keys) <= {'sample', 'target_val', 'accepted', 'n_evals'})

    def _draw_block(self, x, y, k, savestate):
        plan = self.model._plan(x, y)
        self._fresh(plan)
        rec = {}
        if savestate:
            C, dev = self.num_chains, self._theta.device
            views = self.chain.block(k, dict(sample=self._theta, target_val=self._target,
                                             accepted=torch.empty(C, dtype=torch.uint8, device=dev),
                                             n_evals=torch.empty(C, dtype=torch.int32, device=dev)))
            rec = dict(samples=views.get('sample'), targets=views.get('target_val'), accepted_rec=views.get('accepted'),
                       n_evals_rec=views.get('n_evals'))
        if not savestate and k > 1 and plan._moments is not None:
            for _ in range(k):  # attached chain moments are replayed from records a burn-in block does not keep
                out = self._run_block(plan, 1, {})
                self._iter += 1
        else:
            out = self._run_block(plan, k, rec)
            self._iter += k
        self._publish(out['accepted'])
        self._publish_evals(out)
        self.last = out
        if savestate:
            self.chain.commit(k)

    def _run_block(self, plan, k, rec):
        return plan.eslice_run(self._theta, self._target, self._ell, k, max_shrinks=self.max_shrinks, temp=self._temp(),
                               seed=self.seed, it=self._iter, chain_offset=self.chain_offset, **self._base(), **rec)
