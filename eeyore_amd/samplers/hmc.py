import torch

from .base import TRIL_MAX_P, SingleChainSerialSampler, default_counter
from .metric import DenseMetric, DiagMetric
from eeyore_amd.tuners import HMCDATuner, PerChainDATuner, WindowedAdaptation
from eeyore_amd import _lib as L


class HMC(SingleChainSerialSampler):
    """Hamiltonian Monte Carlo with the reference's constructor and surface (eeyore/samplers/hmc.py:8-170).

    One ``draw`` is one call of ``ey_hmc_step``: momentum draw, L leapfrog steps, Hamiltonians, accept and state
    update for every chain, fused in a HIP kernel.  Extensions over the reference: ``theta0`` may be [C, P]
    (C chains advanced together); ``rng`` ('torch' = momentum/uniform from the global torch generator as
    hmc.py:134,148 do, 'philox' = in-kernel counter-based stream keyed by (seed, chain, iteration));
    ``recompute_initial_grad=True`` re-evaluates the gradient at the start of each trajectory exactly as hmc.py:104
    does (same values, one more evaluation); ``step`` may be a [C] tensor and ``temperature`` a [C] tensor.
    ``chain`` defaults to a fresh chain per sampler (the reference's default argument is one ChainList shared by
    every sampler, hmc.py:11).  ``init_step_mode``: how a tuner without a starting step gets one -- 'intended'
    (default: the step-doubling heuristic hmc.py:38-77 set out to write) or 'reference' (what those lines compute,
    integer powers included; see ``init_step``).

    ``metric``: a fixed Euclidean metric, ``DiagMetric(scale)`` or ``DenseMetric(scale_tril)`` (Stan's diag_e / dense_e),
    stating the inverse mass matrix Sigma = L L^T: the momentum is p ~ N(0, Sigma^-1), the kinetic energy p^T Sigma p / 2, and
    one ``draw`` is one call of ``ey_hmc_metric_step`` (a dense metric: at most 128 parameters).  The kernel works in the
    whitened velocity v = L^T p, and that is what ``current['momentum']`` holds with a metric (rng='torch'): the momentum
    itself is p = L^-T v.  A metric per chain is [C, P] / [C, P, P]; ``_set_metric(metric, index)`` takes a table with an
    int32 [C] index naming each chain's entry, in the manner of ``_set_tril``.  Tuners adapt draw by draw (the in-kernel
    dual averaging of the fused kernels is not used with a metric), ``init_step_mode='reference'`` and ``leapfrog`` have no
    metric form and raise ``ValueError``.  Without a metric nothing changes.

    ``tuner=WindowedAdaptation(num_steps, ...)`` with a metric: ``run`` makes the whole burn-in Stan's warm-up on the device
    (ey_hmc_metric_warmup, ey_metric_from_moments) -- a handful of launches that adapt each chain's step by
    dual averaging and re-estimate the metric at the end of doubling windows from moments kept inside the kernel, nothing
    stored or read back between draws.  ``metric`` is the starting metric and its form the form adapted; 'diag' / 'dense'
    are shorthands for the identity of that form.  After burn-in ``metric`` is the adapted ``DiagMetric`` / ``DenseMetric``,
    ``step`` the [C] averaged steps, and the run goes on as any run under a fixed metric.  It needs C chains on the in-kernel
    streams with a full batch: ``ValueError`` otherwise, saying which condition failed.

    ``metric_kernel='fused'`` (default 'generic': nothing changes) runs every call the sampler makes under a diagonal metric
    -- ``draw``, the blocks of ``run``, ``init_step`` / ``init_step_per_chain`` and the whole ``WindowedAdaptation`` warm-up --
    on the matrix cores (EY_HMC_METRIC_FUSED, include/eeyore_amd_hmc_metric_fused.h): for the f32
    MLP(4-32-32-dK) plans whose ``plan.kernel`` is 'mfma32', with ``metric`` a ``DiagMetric`` or 'diag'.  Without a metric or
    with a dense one the constructor raises ``ValueError``; a launch on any other plan raises ``ValueError`` naming
    ``plan.kernel``."""

    keys = ['sample', 'target_val', 'grad_val', 'momentum', 'hamiltonian', 'accepted']

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, step=0.1, num_steps=10,
                 tuner=None, chain=None, rng=None, seed=0, chain_offset=0, recompute_initial_grad=False,
                 temperature=None, init_step_mode='intended', metric=None, metric_kernel='generic'):
        super().__init__(default_counter(counter, dataloader))
        if metric_kernel not in ('generic', 'fused'):
            raise ValueError("HMC: metric_kernel must be 'generic' or 'fused'")
        if metric_kernel == 'fused' and not (metric == 'diag' if isinstance(metric, str) else isinstance(metric, DiagMetric)):
            raise ValueError("HMC: metric_kernel='fused' serves a diagonal metric only (metric='diag' or a DiagMetric)")
        self.metric_kernel = metric_kernel
        self._configure(model, dataloader, theta0, chain, rng, seed, chain_offset, temperature)
        if init_step_mode not in ('intended', 'reference'):
            raise ValueError("init_step_mode must be 'intended' or 'reference'")
        if metric is not None and init_step_mode == 'reference':
            raise ValueError("HMC: init_step_mode='reference' restates the reference's identity-mass heuristic and has no "
                             "metric form; use 'intended' with a metric")
        if isinstance(metric, str):  # the identity of that form
            if metric not in ('diag', 'dense'):
                raise ValueError("HMC: metric must be a DiagMetric, a DenseMetric, 'diag' or 'dense'")
            metric = (DiagMetric if metric == 'diag' else DenseMetric).identity(
                model.num_params(), dtype=model.dtype, device=model.device)
        self._set_metric(metric)
        self.tuner = tuner
        self.recompute_initial_grad = recompute_initial_grad
        self.step, self.num_steps = step, num_steps
        if isinstance(tuner, HMCDATuner):
            if tuner.e0 is None:  # find a starting step size, then let dual averaging shrink towards it (hmc.py:17-27)
                self.init_step(theta0.clone().detach(), intended=init_step_mode == 'intended')
                if not self.step > 0:
                    # 'reference' mode, halving direction: the reference's 2**(-1) on an integer tensor is 0 and its
                    # tuner.num_steps then divides by zero (hmc.py:27,60); the same exception class, with the reason
                    raise ZeroDivisionError(
                        "HMC.init_step (init_step_mode='reference') collapsed the step to 0 as eeyore's integer "
                        "torch.pow(2, -1) does; pass init_step_mode='intended' or give the tuner a starting step e0")
                if tuner.eub is not None:
                    self.step = min(tuner.eub, self.step)
                tuner.set_m(self.step)
            else:
                self.step = tuner.e0
            self.num_steps = tuner.num_steps(self.step)
        elif isinstance(tuner, PerChainDATuner):
            self.step, self.num_steps = tuner.step, tuner.num_steps()
        elif isinstance(tuner, WindowedAdaptation):
            self.num_steps = tuner.num_steps()
            self._check_windowed(False)
        if theta0 is not None:
            self.set_current(theta0.clone().detach(), data=data0)

    # -- energies (hmc.py:84-98); momentum may carry a leading chain axis
    def potential_energy(self, position, x, y):
        return -self.model.log_target(position, x, y)

    def upto_grad_potential_energy(self, position, x, y):
        target_val, grad_val = self.model.upto_grad_log_target(position, x, y)
        return -target_val, -grad_val

    def log_proposal(self, momentum):
        return -0.5 * momentum.pow(2).sum(-1)

    def kinetic_energy(self, momentum):
        return -self.log_proposal(momentum)

    def hamiltonian(self, potential, momentum):
        return potential + self.kinetic_energy(momentum)

    def set_current(self, theta, data=None):
        x, y = super().set_current(theta, data=data)
        self._theta = self._state_tensor(theta)
        self._target, self._grad = self.model._plan(x, y).log_target_grad(self._theta, temp=self._temp())
        self._publish(torch.zeros(self.num_chains, dtype=torch.uint8))
        self.current['accepted'] = None

    def _set_metric(self, metric, index=None):
        """Take a ``DiagMetric`` / ``DenseMetric`` (or None: identity mass, the plain kernels) to the device, checked:
        one entry for all chains, one per chain, or a table of G entries with ``index`` (int32 [C]) naming the entry of
        every chain."""
        if getattr(self, 'metric_kernel', 'generic') == 'fused' and not isinstance(metric, DiagMetric):
            raise ValueError("HMC: metric_kernel='fused' serves a diagonal metric only")
        self.metric = metric
        self._metric = self._metric_form = self._metric_index = None
        if metric is None:
            return
        if not isinstance(metric, (DiagMetric, DenseMetric)):
            raise ValueError("HMC: metric must be a DiagMetric or a DenseMetric")
        P = self.model.num_params()
        if metric.num_params != P:
            raise ValueError(f"HMC: the metric is for {metric.num_params} parameters, the model has {P}")
        if metric.form == 'dense' and P > TRIL_MAX_P:
            raise ValueError(f"HMC: a DenseMetric is limited to {TRIL_MAX_P} parameters (the model has {P}): the factor "
                             "lives in LDS; a DiagMetric has no such limit")
        if index is None and metric.per_chain and metric.table.shape[0] != self.num_chains:
            raise ValueError(f"HMC: the metric holds {metric.table.shape[0]} entries for {self.num_chains} chains: give "
                             "one entry or one per chain")
        self._metric = metric.table.to(device=self.model.device, dtype=self.model.dtype).contiguous()
        self._metric_form = metric.form
        if index is not None:
            self._metric_index = torch.as_tensor(index).to(device=self.model.device, dtype=torch.int32).contiguous()

    def _metric_flags(self, plan):
        """The bits a call under the metric adds to its flags on ``plan``: EY_HMC_METRIC_FUSED with metric_kernel='fused',
        once the plan has said that the fused kernel serves it."""
        if getattr(self, 'metric_kernel', 'generic') != 'fused':
            return 0
        if plan.hmc_metric_kernel(L.EY_HMC_METRIC_FUSED) != 'mfma32':
            raise ValueError(f"HMC: metric_kernel='fused' serves the plans of the mfma32 family; this plan's kernel "
                             f"(plan.kernel) is '{plan.kernel}'; use metric_kernel='generic'")
        return L.EY_HMC_METRIC_FUSED

    def _metric_of(self, c):
        """Chain c's own entry of the metric table, as a table of one."""
        if self._metric.dim() == (1 if self._metric_form == 'diag' else 2):
            return self._metric
        g = c if self._metric_index is None else int(self._metric_index[c])
        return self._metric[g].contiguous()

    def leapfrog(self, position0, momentum0, x, y):
        """(position_L, momentum_L, target_val, grad_val) as hmc.py:100-124: L steps, L+1 gradient evaluations, the
        final momentum negated."""
        if self._metric is not None:
            raise ValueError("HMC.leapfrog has no metric form yet (ey_hmc_leapfrog integrates with identity mass); "
                             "construct the sampler without a metric to use it")
        single = position0.dim() == 1
        th, p = self._state_tensor(position0), self._state_tensor(momentum0)
        step, step_vec = self._step_args()
        t, g = self.model._plan(x, y).leapfrog(th, p, step, self.num_steps, step_vec=step_vec, temp=self._temp())
        return (th[0], p[0], t[0], g[0]) if single else (th, p, t, g)

    def init_step(self, theta, intended=False):
        """First step size for the dual-averaging tuner, as ``HMC.init_step`` (hmc.py:38-77) computes it for chain 0:
        from step 1 with one leapfrog step per trial, the same momentum in every trial, r = exp(H_cur - H_prop).

        The reference's direction a = 2 (r > 1/2) - 1 is an integer tensor, so its ``torch.pow(2, -a)`` / ``torch.pow(2, a)``
        (:60, :67) are integer powers and 2**(-1) is 0: for a = +1 the step doubles until r underflows to 0 (or is NaN),
        for a = -1 it becomes 0 at once (``tuner.num_steps`` then raises ZeroDivisionError, :27).  ``intended=False``
        reproduces exactly that (pinned by the G9 fixture; the constructor's ``init_step_mode='reference'``);
        ``intended=True`` -- what the constructor uses unless told otherwise -- gives what :58-77 set out to write
        (Hoffman & Gelman 2014, algorithm 4: double or halve until r crosses 1/2), which is also what
        ``init_step_per_chain`` does.  (x, y) is the first batch of the loader and h_start is computed once, as in the
        full-batch case of the reference; with minibatches the reference draws a new batch per trial.)"""
        x, y = next(iter(self.dataloader))
        self.step, self.num_steps = 1., 1
        th = (theta if theta.dim() == 1 else theta[0]).to(self.model.device, self.model.dtype)
        momentum = torch.randn(self.model.num_params(), dtype=self.model.dtype, device=self.model.device)
        if self._metric is not None:
            # with a metric: the ratio exp(H_cur - H_prop) of one leapfrog step of ey_hmc_metric_step on cloned state,
            # `momentum` being the whitened velocity of every trial
            if not intended:
                raise ValueError("HMC.init_step: intended=False has no metric form")
            plan = self.model._plan(x, y)
            th1 = self._state_tensor(th)
            temp = self._temp()
            temp = temp[:1] if torch.is_tensor(temp) and temp.dim() == 1 else temp
            t1, g1 = plan.log_target_grad(th1, temp=temp)
            m0, half = self._metric_of(0), torch.full((1,), 0.5, dtype=self.model.dtype, device=self.model.device)

            def ratio_after_one_step():
                out = plan.hmc_metric_step(th1.clone(), t1.clone(), g1.clone(), self.step, 1, m0, self._metric_form,
                                           v0=momentum[None].contiguous(), u=half, temp=temp,
                                           flags=self._metric_flags(plan))
                return torch.exp(out['h_cur'] - out['h_prop']).item()
        else:
            h_start = self.hamiltonian(-self.model.log_target(th.clone(), x, y), momentum)

            def ratio_after_one_step():
                _, p_new, t_new, _ = self.leapfrog(th, momentum, x, y)
                return torch.exp(h_start - self.hamiltonian(-t_new, p_new)).item()

        ratio = ratio_after_one_step()
        direction = 1 if ratio > 0.5 else -1
        if intended:
            threshold, factor = 2. ** (-direction), 2. ** direction
        else:
            threshold, factor = (0, 2) if direction == 1 else (2, 0)
        for _ in range(2200):  # f64 steps leave the representable range long before
            if not (ratio ** direction if ratio != 0 or direction == 1 else float('inf')) > threshold:
                break
            self.step = factor * self.step
            ratio = ratio_after_one_step()
        self.step = float(self.step)

    def init_step_per_chain(self, theta, max_trials=60, momentum=None):
        """One starting step size PER CHAIN for ``theta`` [C, P]: Hoffman & Gelman's heuristic
        (2014, algorithm 4) for every chain at once -- each trial is one launch of ``ey_hmc_leapfrog`` with the per-chain
        step vector; chains whose ratio has crossed 1/2 keep their step.  ``momentum`` [C, P]: the momentum of every trial
        (with a metric: the whitened velocity); default: drawn from the global torch generator.  Returns steps [C] on the
        device."""
        x, y = next(iter(self.dataloader))
        plan = self.model._plan(x, y)
        th0 = self._state_tensor(theta)
        C, P = th0.shape
        if momentum is None:
            momentum = torch.randn(C, P, dtype=self.model.dtype, device=self.model.device)
        elif (tuple(momentum.shape) != (C, P) or momentum.dtype != self.model.dtype or momentum.device != th0.device
              or not momentum.is_contiguous()):
            raise ValueError(f"init_step_per_chain: momentum must be a contiguous [{C}, {P}] tensor of the model's dtype on "
                             "its device")
        t0, g0 = plan.log_target_grad(th0, temp=self._temp())
        h_start = -t0 + 0.5 * momentum.pow(2).sum(-1)
        step = torch.ones(C, dtype=self.model.dtype, device=self.model.device)

        def ratio_after_one_step():
            if self._metric is not None:  # one leapfrog step of ey_hmc_metric_step on cloned state, v0 = momentum
                out = plan.hmc_metric_step(th0.clone(), t0.clone(), g0.clone(), 0.0, 1, self._metric, self._metric_form,
                                           index=self._metric_index, v0=momentum, u=torch.full_like(step, 0.5),
                                           step_vec=step, temp=self._temp(), flags=self._metric_flags(plan))
                return torch.exp(out['h_cur'] - out['h_prop'])
            th, p = th0.clone(), momentum.clone()
            t, _ = plan.leapfrog(th, p, 0.0, 1, step_vec=step, temp=self._temp())
            return torch.exp(h_start - (-t + 0.5 * p.pow(2).sum(-1)))

        ratio = torch.nan_to_num(ratio_after_one_step(), nan=0.0)
        direction = torch.where(ratio > 0.5, 1.0, -1.0).to(step.dtype)
        for _ in range(max_trials):
            active = ratio.pow(direction) > torch.pow(2.0, -direction)
            if not bool(active.any()):
                break
            step = torch.where(active, step * torch.pow(2.0, direction), step)
            ratio = torch.nan_to_num(ratio_after_one_step(), nan=0.0)
        return step

    # -- the windowed warm-up (tuners.WindowedAdaptation)
    def _check_windowed(self, verbose):
        """ValueError unless the warm-up can run in blocks: each message names the condition that failed."""
        who = "HMC with tuner=WindowedAdaptation"
        if not self.batched:
            raise ValueError(f"{who}: one chain (theta0 of shape [P]) cannot be warmed up in blocks; give theta0 of shape "
                             "[C, P]")
        if self.rng != 'philox':
            raise ValueError(f"{who}: rng='torch' draws on the host; the warm-up runs on the in-kernel streams "
                             "(rng='philox')")
        if self.counter is not None and getattr(self.counter, 'num_batches', 1) != 1:
            raise ValueError(f"{who}: minibatches ({self.counter.num_batches} batches per epoch) change the target between "
                             "draws; the warm-up needs the full batch")
        if verbose:
            raise ValueError(f"{who}: verbose=True prints between draws; the warm-up runs whole blocks of draws per launch")
        if self._metric is None:
            raise ValueError(f"{who}: no metric given; pass metric='diag', 'dense' or a starting DiagMetric / DenseMetric")
        if self.tuner.pooled:
            temp = self._temp()
            if torch.is_tensor(temp) and temp.dim() == 1:
                raise ValueError(f"{who}: pooled=True estimates one metric from all chains, which a per-chain temperature "
                                 "vector makes samples of different targets; use pooled=False")
            if self._metric_index is not None:
                raise ValueError(f"{who}: pooled=True estimates one metric from all chains, which a metric index table "
                                 "gives different metrics; use pooled=False")

    def run(self, num_epochs, num_burnin_epochs, verbose=False, verbose_step=100):
        """As ``SingleChainSerialSampler.run``; with ``tuner=WindowedAdaptation`` the burn-in is the tuner's warm-up, a few
        launches per window, and the sampling phase the blocks of ``ey_hmc_metric_run`` of any run under a metric."""
        if not isinstance(self.tuner, WindowedAdaptation):
            return super().run(num_epochs, num_burnin_epochs, verbose=verbose, verbose_step=verbose_step)
        self._check_windowed(verbose)
        counter = self.counter
        counter.set_epoch_info(num_epochs, num_burnin_epochs)
        x, y = next(iter(self.dataloader))
        plan = self.model._plan(x, y)
        plan.detach_da()

        def advance(k):
            for _ in range(k):
                counter.increment_idx()

        if counter.idx < counter.num_burnin_iters:
            self.tuner.warm_up(self, plan, counter.num_burnin_iters - counter.idx, on_block=advance)
            self._publish(self.last['accepted'])
            self.current['momentum'] = self.current['hamiltonian'] = None
        fuse = self._can_fuse(False)
        while counter.idx < counter.num_iters:
            if fuse:
                k = min(self.fused_block, counter.num_iters - counter.idx)
                self._draw_block(x, y, k, savestate=True)
            else:
                k = 1
                self.draw(x, y, savestate=True)
            advance(k)

    def _run_block(self, plan, k, rec):
        step, step_vec = self._step_args()
        flags = L.EY_RECOMPUTE_INITIAL_GRAD if self.recompute_initial_grad else 0
        if self._metric is not None:
            flags |= self._metric_flags(plan)
            out = plan.hmc_metric_run(self._theta, self._target, self._grad, step, self.num_steps, self._metric,
                                      self._metric_form, k, index=self._metric_index, step_vec=step_vec, temp=self._temp(),
                                      seed=self.seed, it=self._iter, chain_offset=self.chain_offset, flags=flags, **rec)
        else:
            out = plan.hmc_run(self._theta, self._target, self._grad, step, self.num_steps, k, step_vec=step_vec,
                               temp=self._temp(), seed=self.seed, it=self._iter, chain_offset=self.chain_offset,
                               flags=flags, **rec)
        self.current['momentum'] = None
        self.current['hamiltonian'] = None
        return out

    def draw(self, x, y, savestate=False):
        """One HMC iteration of every chain (hmc.py:126-170)."""
        plan = self.model._plan(x, y)
        temp = self._temp()
        if self.counter.num_batches != 1:
            # minibatching: the cached target/gradient belong to another batch (hmc.py:129-131)
            self._target, self._grad = plan.log_target_grad(self._theta, temp=temp)
        p0, u = self._draw_randoms(*self._theta.shape)
        step, step_vec = self._step_args()
        flags = L.EY_RECOMPUTE_INITIAL_GRAD if self.recompute_initial_grad else 0
        if self._metric is not None:  # p0 is then the whitened velocity v = L^T p
            flags |= self._metric_flags(plan)
            out = plan.hmc_metric_step(self._theta, self._target, self._grad, step, self.num_steps, self._metric,
                                       self._metric_form, index=self._metric_index, v0=p0, u=u, temp=temp,
                                       step_vec=step_vec, seed=self.seed, it=self._iter, chain_offset=self.chain_offset,
                                       flags=flags)
        else:
            out = plan.hmc_step(self._theta, self._target, self._grad, step, self.num_steps, p0=p0, u=u, temp=temp,
                                step_vec=step_vec, seed=self.seed, it=self._iter, chain_offset=self.chain_offset,
                                flags=flags)
        self._publish(out['accepted'])
        self.current['momentum'] = None if p0 is None else self._expose(p0)
        self.current['hamiltonian'] = self._expose(out['h_cur'])
        if isinstance(self.tuner, HMCDATuner) and self.counter.idx < self.counter.num_burnin_iters:
            last_burnin = self.counter.idx == self.counter.num_burnin_iters - 1
            self.step, self.num_steps = self.tuner.tune(out['rate'].mean().item(), self.counter.idx,
                                                        return_e=not last_burnin)
        elif isinstance(self.tuner, PerChainDATuner) and self.counter.idx < self.counter.num_burnin_iters:
            last_burnin = self.counter.idx == self.counter.num_burnin_iters - 1
            self.step, _ = self.tuner.tune(out['rate'], self.counter.idx, return_e=not last_burnin)
        self._iter += 1
        self.last = out
        if savestate:
            self.chain.detach_and_update(self.current)
