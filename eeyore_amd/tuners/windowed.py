"""Stan's warm-up for ``HMC(metric=...)``, on the device: per-chain dual averaging of the step and a metric re-estimated at
the end of doubling windows, with short buffers at both ends that adapt the step only (Stan reference manual, "Automatic
parameter tuning").

All chains share the launches, so the number of leapfrog steps is fixed (as in ``PerChainDATuner``).  Nothing a draw makes
is stored: ``ey_hmc_metric_warmup`` adapts each chain's step and accumulates each chain's running moments inside the kernel
that makes the draws, and ``ey_metric_from_moments`` turns the moments into the next metric -- pooled over all chains by
default, so that a 25-draw window already holds 25 C draws.  A warm-up is a function of (seed, chain_offset, theta0) alone."""
import math

from .dual_averaging import Tuner


class WindowedAdaptation(Tuner):
    gamma, t0, kappa = 0.05, 10, 0.75  # dual averaging, as HMCDATuner / PerChainDATuner
    # The momenta of the step-size searches (HMC.init_step_per_chain) come from ey_philox_normal under a key of their own:
    # the sampler's (seed, chain_offset) with iteration index SEARCH_ITER + k for the search made before burn-in draw k.  No
    # draw reaches iteration 2^40, so a search never sees the momentum a draw uses.
    SEARCH_ITER = 1 << 40

    def __init__(self, num_steps, d=0.8, init_buffer=75, term_buffer=50, base_window=25, pooled=True, eub=None):
        for name, v, low in (("num_steps", num_steps, 1), ("init_buffer", init_buffer, 0), ("term_buffer", term_buffer, 0),
                             ("base_window", base_window, 1)):
            if int(v) != v or v < low:
                raise ValueError(f"WindowedAdaptation: {name} must be an integer >= {low}")
        if not 0.0 < d < 1.0:
            raise ValueError("WindowedAdaptation: the target acceptance d must lie in (0, 1)")
        if eub is not None and not eub > 0:
            raise ValueError("WindowedAdaptation: eub must be positive")
        self.fixed_num_steps = int(num_steps)
        self.d, self.eub = float(d), eub
        self.logeub = None if eub is None else math.log(eub)
        self.init_buffer, self.term_buffer, self.base_window = int(init_buffer), int(term_buffer), int(base_window)
        self.pooled = bool(pooled)
        self.history = []  # one entry per window end of the last warm-up
        self.state = None  # [C, 3] float64 on the device: (barh, logbare, mu) of the last warm-up

    def num_steps(self, e=None):
        return self.fixed_num_steps

    def coefficients(self, t):
        """(1/(t + t0), sqrt(t)/gamma, t^-kappa): the row of the dual-averaging table for the t-th adapting draw, t >= 1."""
        return 1.0 / (t + self.t0), math.sqrt(t) / self.gamma, t ** (-self.kappa)

    def buffers(self, n):
        """(init, term, base) for a burn-in of n draws: the constructor's, or 15 % / 10 % / the rest when they do not fit."""
        init, term, base = self.init_buffer, self.term_buffer, self.base_window
        if init + base + term > n:
            init, term = int(0.15 * n), int(0.1 * n)
            base = n - init - term
        return init, term, base

    def windows(self, n):
        """[(start, end)] of the metric windows of a burn-in of n draws, as Stan lays them out: none below 20 draws; from
        the end of the initial buffer, each window twice as long as the one before; a window whose successor would not
        fit before the terminal buffer is stretched to it."""
        n = int(n)
        if n < 20:
            return []
        init, term, base = self.buffers(n)
        out, start, size, last = [], init, base, n - term
        while start < last:
            end = start + size
            if end + 2 * size > last:
                end = last
            out.append((start, end))
            start, size = end, 2 * size
        return out

    def phases(self, n):
        """[(start, end, adapts_metric)]: the burn-in cut at the window ends, with the buffers around the windows."""
        wins = self.windows(n)
        if not wins:
            return [(0, int(n), False)] if n > 0 else []
        out = [(0, wins[0][0], False)] + [(s, e, True) for s, e in wins] + [(wins[-1][1], int(n), False)]
        return [p for p in out if p[1] > p[0]]

    # ------------------------------------------------------------------ the warm-up itself
    def start_steps(self, sampler, plan, k):
        """A starting step per chain at the chains' current state and under the sampler's current metric, for the search
        made before burn-in draw k: Hoffman & Gelman's heuristic on momenta from the key documented above."""
        C = sampler.num_chains
        momentum = plan.philox_normal(C, sampler.seed, self.SEARCH_ITER + k, sampler.chain_offset)
        step = sampler.init_step_per_chain(sampler._theta, momentum=momentum)
        if self.eub is not None:
            step = step.clamp(max=self.eub)
        return step.contiguous()

    def restart(self, step):
        """The dual-averaging state [C, 3] that starts over from ``step``: barh = logbare = 0, mu = log(10 step)."""
        import torch
        state = torch.zeros(step.shape[0], 3, dtype=torch.float64, device=step.device)
        state[:, 2] = torch.log(10 * step.to(torch.float64))
        return state

    def table(self, t, k, device):
        """Rows t .. t + k - 1 of the dual-averaging table, on the device."""
        import torch
        return torch.tensor([self.coefficients(t + j) for j in range(k)], dtype=torch.float64, device=device)

    def warm_up(self, sampler, plan, n, on_block=None):
        """Run the ``n`` burn-in draws of ``sampler`` (an HMC with a metric, from its current state and iteration index) in
        launches of at most ``sampler.fused_block`` draws.  Leaves the sampler's state, ``sampler.step`` (the [C] averaged
        steps) and ``sampler.metric``; ``history`` says what happened at each window end.  ``on_block(k)`` is called after
        every launch of k draws (the sampler advances its counters there)."""
        import torch
        from eeyore_amd import _lib as L
        from eeyore_amd.samplers.metric import DenseMetric, DiagMetric
        form, C, P = sampler._metric_form, sampler.num_chains, sampler.model.num_params()
        dev = sampler._theta.device
        block = sampler.fused_block if sampler.fused_block > 0 else 1
        if plan._moments is not None:  # attached chain moments are replayed from records a burn-in block does not keep
            block = 1
        flags = L.EY_RECOMPUTE_INITIAL_GRAD if sampler.recompute_initial_grad else 0
        flags |= sampler._metric_flags(plan)  # HMC(metric_kernel='fused'): EY_HMC_METRIC_FUSED; otherwise nothing
        # a sampler with a warm-up launch of its own (NUTS: ey_nuts_warmup) gives it as _warmup_launch(plan, num_steps, k,
        # **the keywords below); HMC has none and goes through ey_hmc_metric_warmup
        launch = getattr(sampler, '_warmup_launch', None)
        self.history = []
        step = self.start_steps(sampler, plan, 0)
        state, t = self.restart(step), 1
        mean = torch.zeros(C, P, dtype=torch.float64, device=dev)
        M2 = torch.zeros((C, P) if form == 'diag' else (C, P, P), dtype=torch.float64, device=dev)
        for start, end, adapts in self.phases(n):
            done = 0
            while start + done < end:
                k = min(block, end - start - done)
                last = start + done + k == n
                kw = dict(index=sampler._metric_index, step_vec=step, temp=sampler._temp(), seed=sampler.seed,
                          it=sampler._iter, chain_offset=sampler.chain_offset, flags=flags, da_state=state,
                          da_table=self.table(t, k, dev), d=self.d, log_eub=self.logeub, final_avg=last,
                          mean=mean if adapts else None, M2=M2 if adapts else None, count=done)
                if launch is not None:
                    out = launch(plan, self.fixed_num_steps, k, **kw)
                else:
                    out = plan.hmc_metric_warmup(sampler._theta, sampler._target, sampler._grad, 0.0, self.fixed_num_steps,
                                                 sampler._metric, form, k, **kw)
                done, t = done + k, t + k
                sampler._iter += k
                sampler.last = out
                if on_block is not None:
                    on_block(k)
            if not adapts:
                continue
            # the end of a window: the next metric, moments from zero, a new starting step, dual averaging from t = 1
            prev = sampler._metric
            if self.pooled:
                table, status = plan.metric_from_moments(mean, M2, done, form, pooled=True)
                failed = int(status.sum())
                if failed:
                    table = prev
            else:
                entry = (P,) if form == 'diag' else (P, P)
                table = (prev if prev.dim() == len(entry) + 1 and prev.shape[0] == C and sampler._metric_index is None
                         else (prev[sampler._metric_index.long()] if sampler._metric_index is not None
                               else prev.expand((C,) + entry))).contiguous().clone()
                table, status = plan.metric_from_moments(mean, M2, done, form, pooled=False, table=table)
                failed = int(status.sum())
            self.history.append(dict(draw=end, failed=failed, updated=failed < (1 if self.pooled else C)))
            if self.history[-1]['updated']:
                sampler._set_metric((DiagMetric if form == 'diag' else DenseMetric)(table))
            mean.zero_()
            M2.zero_()
            step = self.start_steps(sampler, plan, end)
            state, t = self.restart(step), 1
        self.state = state
        sampler.step = step
        return step
