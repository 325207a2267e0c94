import math

import torch

from .base import SingleChainSerialSampler, default_counter


class RAM(SingleChainSerialSampler):
    """Robust adaptive Metropolis (Vihola 2012; eeyore/samplers/ram.py:7-70) as one ``ey_ram_step`` per draw: propose
    theta + S z with the chain's lower-triangular factor S (``chol_cov``), accept iff log u < log-rate, then always adapt
    S <- chol(S (I + h (alpha - a) z z^T / |z|^2) S^T), h = min(1, P n^-g), n = counter.idx + 1 - offset.  The factor is
    updated in closed form inside the kernel.

    ``theta0`` [P] is the reference's single chain (random draws from the global torch generator, z then u, as the
    reference draws them); [C, P] runs C chains on the in-kernel Philox streams.  ``cov0`` is [P, P] (shared) or
    [C, P, P].  Limits: P <= 128 (the factor lives in LDS) and 0 < a < 1 (the reference accepts any ``a``; from a = 1 on
    its re-factorisation can fail mid-run)."""

    keys = ['sample', 'target_val', 'accepted']
    max_params = 128

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, cov0=None, a=0.234, g=0.7,
                 chain=None, rng=None, seed=0, chain_offset=0, temperature=None):
        P = model.num_params()
        if P > self.max_params:
            raise ValueError(f"RAM: the model has {P} parameters; the kernel keeps the factor in LDS and serves at most "
                             f"{self.max_params}")
        if not 0.0 < float(a) < 1.0:
            raise ValueError(f"RAM: the target acceptance a must lie in (0, 1), got {a}")
        if not math.isfinite(float(g)):
            raise ValueError(f"RAM: the decay exponent g must be finite, got {g}")
        super().__init__(default_counter(counter, dataloader))
        self._configure(model, dataloader, theta0, chain, rng, seed, chain_offset, temperature)
        self.a, self.g = float(a), float(g)
        kw = dict(dtype=model.dtype, device=model.device)
        self.cov0 = cov0.clone().detach().to(**kw) if cov0 is not None else torch.eye(P, **kw)
        self._check_cov(self.cov0)
        self._block_iter0 = None
        if theta0 is not None:
            self.set_all(theta0.clone().detach(), data=data0)

    def _check_cov(self, cov):
        P = self.model.num_params()
        if tuple(cov.shape) not in ((P, P), (self.num_chains, P, P)):
            raise ValueError(f"RAM: a covariance must be [{P}, {P}] or [{self.num_chains}, {P}, {P}], "
                             f"got {tuple(cov.shape)}")

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
        """chol_cov = cholesky(cov), cov0 when ``cov`` is None.  (The reference's ``cov or self.cov0`` raises for any
        covariance of more than one element)"""
        cov = self.cov0 if cov is None else cov.detach().to(dtype=self.model.dtype, device=self.model.device)
        self._check_cov(cov)
        P = self.model.num_params()
        chol = torch.linalg.cholesky(cov.cpu()).to(self.model.device)  # once per reset: the factor is then the kernel's
        self._chol = chol.expand(self.num_chains, P, P).contiguous()

    def set_all(self, theta, data=None, cov=None):
        super().set_all(theta, data=data)
        self.set_cov(cov=cov)

    @property
    def chol_cov(self):
        """The current lower-triangular factor: [P, P] for a single chain, [C, P, P] for C chains."""
        return self._expose(self._chol)

    @chol_cov.setter
    def chol_cov(self, value):
        P = self.model.num_params()
        v = value.detach().to(dtype=self.model.dtype, device=self.model.device)
        self._chol = torch.tril(v).expand(self.num_chains, P, P).contiguous()

    def _adapt_index(self, offset=0):
        n = self.counter.idx + 1 - offset
        if self._block_iter0 is not None:  # a block issued one iteration at a time does not advance the counter
            n += self._iter - self._block_iter0
        return n

    def _run_block(self, plan, k, rec):
        return plan.ram_run(self._theta, self._target, self._chol, self._adapt_index(), k, a=self.a, g=self.g,
                            temp=self._temp(), seed=self.seed, it=self._iter, chain_offset=self.chain_offset, **rec)

    def _draw_block(self, x, y, k, savestate):
        self._block_iter0 = self._iter
        try:
            super()._draw_block(x, y, k, savestate)
        finally:
            self._block_iter0 = None

    def draw(self, x, y, savestate=False, offset=0):
        plan = self.model._plan(x, y)
        if self.counter.num_batches != 1:  # ram.py:41-42
            self._evaluate_target(plan)
        z, u = self._draw_randoms(*self._theta.shape)
        out = plan.ram_step(self._theta, self._target, self._chol, self._adapt_index(offset), a=self.a, g=self.g, z=z,
                            u=u, temp=self._temp(), seed=self.seed, it=self._iter, chain_offset=self.chain_offset)
        self._finish_draw(out, savestate)
