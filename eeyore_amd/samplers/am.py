import math
import warnings

import torch

from .base import SingleChainSerialSampler, default_counter


class Ridge:
    """The transform that defines textbook adaptive Metropolis, cov -> cov + eps I, as a small callable (usable as the
    reference's ``transform`` too).  ``AM`` recognises it and fuses the ridge into its kernel."""

    def __init__(self, eps):
        eps = float(eps)
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"Ridge: eps must be finite and >= 0, got {eps}")
        self.eps = eps

    def __call__(self, cov):
        return cov + self.eps * torch.eye(cov.shape[-1], dtype=cov.dtype, device=cov.device)

    def __repr__(self):
        return f"Ridge({self.eps})"


class SoftAbs:
    """The transform of the reference's AM examples, cov -> softabs(cov, a) (``eeyore_amd.stats.softabs``), as a small
    callable: the running covariance of the first draws is rank deficient, softabs lifts its null space to 1 / a.  ``AM``
    recognises it and runs the eigen-decomposition inside its kernel, in f64 whatever the model's dtype.  Called on a
    device tensor it is ``stats.batched.softabs`` (the kernel's own function), otherwise ``stats.softabs``."""

    def __init__(self, a=1000.0):
        a = float(a)
        if not (math.isfinite(a) and a > 0.0):
            raise ValueError(f"SoftAbs: a must be finite and > 0, got {a}")
        self.a = a

    def __call__(self, cov):
        from eeyore_amd import stats
        return stats.batched.softabs(cov, self.a) if cov.is_cuda else stats.softabs(cov, self.a)

    def __repr__(self):
        return f"SoftAbs({self.a})"


class AM(SingleChainSerialSampler):
    """Adaptive Metropolis (Haario et al. 2001; eeyore/samplers/am.py:8-107) as one ``ey_am_step`` per draw.  With
    n = counter.idx + 1 - offset: propose theta + c z while n <= t0; afterwards, with probability l, theta + c z, else
    theta + (b chol(cov)) z.  Accept iff log u < log-rate, then always update running_mean and cov_sum and, from n >= t0
    on, set cov <- cov0 while nothing was accepted, else transform((cov_sum - n mean mean^T) / (n - 1)).  The
    factorisation runs inside the kernel.

    ``transform``: None, ``Ridge(eps)`` or ``SoftAbs(a)`` (both fused into the kernel) or any callable on a [P, P]
    covariance (one launch per draw, the covariance passing through the callable in torch between launches).  A model
    beside which the work matrix of ``SoftAbs`` does not fit in LDS takes that callable path with the same object, after
    one warning.  ``theta0`` [P] is the reference's
    single chain (torch random draws in the reference's order: z, the mixture uniform only when n > t0, u); [C, P] runs C
    chains on the in-kernel Philox streams.  ``cov0`` is [P, P] (shared) or [C, P, P].

    A covariance that cannot be factorised makes the reference raise; here the chain proposes theta + c z for that draw
    and its ``breakdowns`` counter grows.  ``on_breakdown='raise'`` (the default) raises RuntimeError after the launch,
    ``'isotropic'`` lets the run go on.  Limits: P <= 128 and t0 >= 2 (the reference divides by zero below)."""

    keys = ['sample', 'target_val', 'accepted']
    max_params = 128

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, cov0=None, l=0.05, b=1., c=1.,
                 t0=2, transform=None, chain=None, rng=None, seed=0, chain_offset=0, temperature=None,
                 on_breakdown='raise'):
        P = model.num_params()
        if P > self.max_params:
            raise ValueError(f"AM: the model has {P} parameters; the kernel keeps the covariance in LDS and serves at "
                             f"most {self.max_params}")
        if int(t0) != t0 or t0 < 2:
            raise ValueError(f"AM: t0 must be an integer >= 2 (the covariance divides by n - 1), got {t0}")
        if not 0.0 <= float(l) <= 1.0:
            raise ValueError(f"AM: the mixture weight l must lie in [0, 1], got {l}")
        if not (math.isfinite(float(b)) and math.isfinite(float(c))):
            raise ValueError(f"AM: b and c must be finite, got b = {b}, c = {c}")
        if on_breakdown not in ('raise', 'isotropic'):
            raise ValueError(f"AM: on_breakdown must be 'raise' or 'isotropic', got {on_breakdown!r}")
        if transform is not None and not callable(transform):
            raise ValueError("AM: transform must be None, a Ridge or a callable")
        super().__init__(default_counter(counter, dataloader))
        self._configure(model, dataloader, theta0, chain, rng, seed, chain_offset, temperature)
        self.l, self.b, self.c, self.t0 = float(l), float(b), float(c), int(t0)
        self.transform, self.on_breakdown = transform, on_breakdown
        self._generic = transform is not None and not isinstance(transform, (Ridge, SoftAbs))
        self._eps = transform.eps if isinstance(transform, Ridge) else 0.0
        self._softabs_a = transform.a if isinstance(transform, SoftAbs) else None
        kw = dict(dtype=model.dtype, device=model.device)
        self.cov0 = cov0.clone().detach().to(**kw) if cov0 is not None else torch.eye(P, **kw)
        self._check_cov(self.cov0)
        if transform is not None:  # am.py:26-27: once, here
            self.cov0 = self._transformed(self.cov0)
        self.cov0 = self.cov0.contiguous()
        C = self.num_chains
        self._nacc = torch.zeros(C, dtype=torch.int32, device=model.device)
        self._breakdowns = torch.zeros(C, dtype=torch.int32, device=model.device)
        self._seen = torch.zeros(C, dtype=torch.int32)
        self._block_iter0 = None
        if theta0 is not None:
            self.set_all(theta0.clone().detach(), data=data0)

    def _check_cov(self, cov):
        P = self.model.num_params()
        if tuple(cov.shape) not in ((P, P), (self.num_chains, P, P)):
            raise ValueError(f"AM: a covariance must be [{P}, {P}] or [{self.num_chains}, {P}, {P}], "
                             f"got {tuple(cov.shape)}")

    def _transformed(self, cov):
        if cov.dim() == 2 or isinstance(self.transform, (Ridge, SoftAbs)):
            return self.transform(cov)
        return torch.stack([self.transform(m) for m in cov])

    def _can_fuse(self, verbose):
        if self._softabs_a is not None and super()._can_fuse(verbose):
            self._route(self.model._plan(*next(iter(self.dataloader))))
        return not self._generic and super()._can_fuse(verbose)

    def _evaluate_target(self, plan):
        lik, prior = plan.log_target(self._theta, temp=self._temp())
        self._target = lik + prior

    def set_current(self, theta, data=None):
        x, y = super().set_current(theta, data=data)
        self._theta = self._state_tensor(theta)
        self._evaluate_target(self.model._plan(x, y))
        self._publish(torch.zeros(self.num_chains, dtype=torch.uint8))
        self.current['accepted'] = None

    def set_cov(self, cov=None):
        """cov <- ``cov`` as given (not transformed, am.py:40-41), the transformed cov0 when None; running_mean and
        cov_sum restart from zero (:44-47)."""
        cov = self.cov0 if cov is None else cov.detach().to(dtype=self.model.dtype, device=self.model.device)
        self._check_cov(cov)
        C, P = self.num_chains, self.model.num_params()
        self._cov = cov.expand(C, P, P).contiguous().clone()
        self._mean = torch.zeros(C, P, dtype=self.model.dtype, device=self.model.device)
        self._cov_sum = torch.zeros(C, P, P, dtype=self.model.dtype, device=self.model.device)

    def set_all(self, theta, data=None, cov=None):
        super().set_all(theta, data=data)
        self.set_cov(cov=cov)

    def reset(self, theta, data=None, reset_counter=True, reset_chain=True):
        super().reset(theta, data=data, reset_counter=reset_counter, reset_chain=reset_chain)
        self._nacc.zero_()  # am.py:55

    @staticmethod
    def _sym(lower):
        """The symmetric matrix whose lower triangle the kernel maintains."""
        lo = torch.tril(lower)
        return lo + torch.tril(lower, -1).transpose(-1, -2)

    @property
    def cov(self):
        """The proposal covariance: [P, P] for a single chain, [C, P, P] for C chains."""
        return self._expose(self._sym(self._cov))

    @property
    def cov_sum(self):
        return self._expose(self._sym(self._cov_sum))

    @property
    def running_mean(self):
        return self._expose(self._mean)

    @property
    def num_accepted(self):
        return self._nacc if self.batched else int(self._nacc[0].item())

    @property
    def breakdowns(self):
        """How often each chain's covariance could not be factorised (the draw then proposed theta + c z)."""
        return self._breakdowns if self.batched else int(self._breakdowns[0].item())

    def _index(self):
        idx = self.counter.idx
        if self._block_iter0 is not None:  # a block issued one iteration at a time does not advance the counter
            idx += self._iter - self._block_iter0
        return idx

    def _am_args(self):
        return dict(l=self.l, b=self.b, c=self.c, eps=self._eps, t0=self.t0, temp=self._temp(), seed=self.seed,
                    it=self._iter, chain_offset=self.chain_offset, breakdowns=self._breakdowns,
                    softabs_a=self._softabs_a)

    def _route(self, plan):
        """A SoftAbs whose work matrix does not fit beside this plan's model: the callable path, said once."""
        if self._softabs_a is not None and not plan.am_softabs_fits():
            warnings.warn(f"AM: the work matrix of {self.transform!r} does not fit in LDS beside this model "
                          f"({self.model.num_params()} parameters, {self.model.dtype}); the transform runs between "
                          "launches, one launch per draw", RuntimeWarning, stacklevel=3)
            self._softabs_a, self._generic = None, True

    def _state(self):
        return self._theta, self._target, self._mean, self._cov_sum, self._cov, self._nacc, self.cov0

    def _check_breakdowns(self):
        if self.on_breakdown != 'raise':
            return
        now = self._breakdowns.cpu()
        grew = (now > self._seen).nonzero().flatten().tolist()
        self._seen = now
        if grew:
            raise RuntimeError(f"AM: the covariance of chain(s) {grew} could not be factorised (a pivot was not positive); "
                               "the draw proposed theta + c z instead.  Give a transform such as Ridge(eps), or "
                               "on_breakdown='isotropic' to continue")

    def _run_block(self, plan, k, rec):
        out = plan.am_run(*self._state(), self._index(), k, **self._am_args(), **rec)
        self._check_breakdowns()
        return out

    def _draw_block(self, x, y, k, savestate):
        self._block_iter0 = self._iter
        try:
            super()._draw_block(x, y, k, savestate)
        finally:
            self._block_iter0 = None

    def _retransform(self, n):
        """The generic callable: the kernel ran with eps = 0; what it recomputed (n >= t0, something accepted, am.py:99-101)
        passes through ``transform`` in torch."""
        if n < self.t0:
            return
        for c in (self._nacc > 0).nonzero().flatten().tolist():
            self._cov[c] = self.transform(self._sym(self._cov[c]))

    def draw(self, x, y, savestate=False, offset=0):
        plan = self.model._plan(x, y)
        self._route(plan)
        if self.counter.num_batches != 1:  # am.py:64-65
            self._evaluate_target(plan)
        idx = self._index()
        n = idx + 1 - offset
        z = u_mix = u = None
        if self.rng == 'torch':  # the reference's order: randn(P), rand(1) for the mixture only when n > t0, rand(1)
            C, P = self._theta.shape
            z = self._randn(C, P)
            u_mix = self._rand(C) if n > self.t0 else None
            u = self._rand(C)
        out = plan.am_step(*self._state(), idx, offset=offset, z=z, u_mix=u_mix, u=u, **self._am_args())
        if self._generic:
            self._retransform(n)
        self._check_breakdowns()
        self._finish_draw(out, savestate)
