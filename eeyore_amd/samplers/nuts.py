import torch

from .base import ChainBuffer
from .hmc import HMC
from .metric import DenseMetric, DiagMetric
from eeyore_amd.tuners import HMCDATuner, PerChainDATuner
from eeyore_amd import _lib as L

NUTS_MAX_P = 128  # ey_nuts_step keeps the tree's vectors in LDS, in either metric form, unless tree='device' or 'fused'


class NUTS(HMC):
    """The No-U-Turn sampler under a fixed Euclidean metric: ``HMC(metric=...)`` without ``num_steps``.

    One ``draw`` is one call of ``ey_nuts_step``: multinomial NUTS in the whitened velocity of
    ``HMC``'s metric path -- the tree doubles backward or forward until the generalised U-turn criterion fails between its
    edges or inside the new subtree, a leaf's energy error exceeds 1000 (a divergent draw), or ``max_depth`` (at most 10)
    doublings are made; one wave per chain, so trees of different depth cost load balance only.  ``metric=None`` is the
    identity ``DiagMetric``; otherwise as ``HMC`` ('diag', 'dense', a ``DiagMetric`` / ``DenseMetric``, per chain or
    indexed through ``_set_metric``).  At most 128 parameters in either form with ``tree='lds'``, the default.

    ``tree='device'`` keeps the tree's vectors in a workspace in device memory instead (include/eeyore_amd_nuts_tree.h,
    DESIGN.md 4.27): the same draw for any number of parameters whose evaluation fits LDS, under a diagonal metric only
    (``metric=None``, 'diag' or a ``DiagMetric``; a dense one raises ``ValueError``).  The workspace, (12 + 2 max_depth)
    vectors per chain, is attached to the plan a launch is about to run on and grows with the largest call.

    ``tree='fused'`` is ``tree='device'`` with every leapfrog step on the matrix cores (include/eeyore_amd_nuts_fused.h,
    DESIGN.md 4.28): for the f32 MLP(4-32-32-dK) plans whose ``plan.kernel`` is 'mfma32', under the same diagonal metrics and
    in the same workspace; a launch on any other plan raises ``ValueError`` naming ``plan.kernel``.

    ``theta0`` [C, P] or [P]; ``rng='torch'`` draws the velocity and the draw's table of uniforms on the host (the word
    layout of include/eeyore_amd_nuts.h), ``rng='philox'`` uses the in-kernel streams.  ``PerChainDATuner`` / ``HMCDATuner``
    adapt the step draw by draw on the draw's mean accept statistic; ``tuner=WindowedAdaptation(...)`` runs the whole
    warm-up of ``HMC`` through ``ey_nuts_warmup`` (the tuner's ``num_steps`` is unused).  ``last`` carries depth,
    n_leapfrog, divergent and accept_stat of the last draw; a chain whose keys include 'depth' / 'divergent' records them.
    ``leapfrog`` and ``init_step_mode='reference'`` have no NUTS form and raise ``ValueError``."""

    keys = ['sample', 'target_val', 'grad_val', 'accepted', 'depth', 'divergent']

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, step=0.1, max_depth=10, metric=None,
                 tuner=None, chain=None, rng=None, seed=0, chain_offset=0, recompute_initial_grad=False, temperature=None,
                 init_step_mode='intended', tree='lds'):
        if tree not in ('lds', 'device', 'fused'):
            raise ValueError("NUTS: tree must be 'lds' or 'device', or 'fused' for the plans of the mfma32 family")
        if init_step_mode == 'reference':
            raise ValueError("NUTS: init_step_mode='reference' restates the reference's identity-mass heuristic and has no "
                             "metric form; use 'intended'")
        if int(max_depth) != max_depth or not 1 <= max_depth <= L.EY_NUTS_MAX_DEPTH:
            raise ValueError(f"NUTS: max_depth must be an integer in [1, {L.EY_NUTS_MAX_DEPTH}]")
        P = model.num_params()
        if tree == 'lds' and P > NUTS_MAX_P:
            raise ValueError(f"NUTS is limited to {NUTS_MAX_P} parameters (the model has {P}): the tree lives in LDS; "
                             "pass tree='device' for a diagonal metric")
        if tree != 'lds' and (metric == 'dense' or isinstance(metric, DenseMetric)):
            raise ValueError(f"NUTS: tree='{tree}' serves a diagonal metric only (metric=None, 'diag' or a DiagMetric)")
        self.tree = tree
        if metric is None:
            metric = DiagMetric.identity(P, dtype=model.dtype, device=model.device)
        self.max_depth = int(max_depth)
        super().__init__(model, theta0=theta0, dataloader=dataloader, data0=data0, counter=counter, step=step, num_steps=1,
                         tuner=tuner, chain=chain, rng=rng, seed=seed, chain_offset=chain_offset,
                         recompute_initial_grad=recompute_initial_grad, temperature=temperature,
                         init_step_mode=init_step_mode, metric=metric)
        self.num_steps = None  # there is none: the trajectory ends itself

    def leapfrog(self, position0, momentum0, x, y):
        raise ValueError("NUTS.leapfrog: a NUTS trajectory has no fixed length; use HMC.leapfrog")

    def _set_metric(self, metric, index=None):
        if getattr(self, 'tree', 'lds') != 'lds' and isinstance(metric, DenseMetric):
            raise ValueError(f"NUTS: tree='{self.tree}' serves a diagonal metric only")
        super()._set_metric(metric, index)

    def _flags(self, plan):
        """The flags of a launch on ``plan``; with tree='device' or 'fused' the plan first gets a workspace for this
        sampler's tree."""
        flags = L.EY_RECOMPUTE_INITIAL_GRAD if self.recompute_initial_grad else 0
        if self.tree == 'device':
            plan.attach_nuts_tree(self.num_chains, self.max_depth)
            flags |= L.EY_NUTS_TREE_DEVICE
        elif self.tree == 'fused':
            if plan.nuts_kernel(L.EY_NUTS_FUSED) != 'mfma32':
                raise ValueError(f"NUTS: tree='fused' serves the plans of the mfma32 family; this plan's kernel "
                                 f"(plan.kernel) is '{plan.kernel}'; use tree='device'")
            plan.attach_nuts_tree(self.num_chains, self.max_depth)
            flags |= L.EY_NUTS_FUSED
        return flags

    # -- one draw
    def _nuts_randoms(self, C, P):
        """(v0 [C, P], u [C, S]) from the global torch generator, or (None, None) for the in-kernel streams."""
        if self.rng != 'torch':
            return None, None
        S = 1 + 2 * L.EY_NUTS_MAX_DEPTH + 2 ** self.max_depth
        return self._randn(C, P), torch.rand(C, S, dtype=self.model.dtype, device=self.model.device)

    def _publish_nuts(self, out):
        for k in ('depth', 'divergent'):
            self.current[k] = out[k] if self.batched else int(out[k][0].item())
        self.current['momentum'] = self.current['hamiltonian'] = None

    def draw(self, x, y, savestate=False):
        """One NUTS iteration of every chain."""
        plan = self.model._plan(x, y)
        temp = self._temp()
        if self.counter.num_batches != 1:  # minibatching: the cached target / gradient belong to another batch
            self._target, self._grad = plan.log_target_grad(self._theta, temp=temp)
        v0, u = self._nuts_randoms(*self._theta.shape)
        step, step_vec = self._step_args()
        flags = self._flags(plan)
        out = plan.nuts_step(self._theta, self._target, self._grad, step, self.max_depth, self._metric, self._metric_form,
                             index=self._metric_index, v0=v0, u=u, step_vec=step_vec, temp=temp, seed=self.seed,
                             it=self._iter, chain_offset=self.chain_offset, flags=flags)
        self._publish(out['accepted'])
        self._publish_nuts(out)
        burning = self.counter.idx < self.counter.num_burnin_iters
        last_burnin = self.counter.idx == self.counter.num_burnin_iters - 1
        if isinstance(self.tuner, HMCDATuner) and burning:
            self.step, _ = self.tuner.tune(out['accept_stat'].mean().item(), self.counter.idx, return_e=not last_burnin)
        elif isinstance(self.tuner, PerChainDATuner) and burning:
            self.step, _ = self.tuner.tune(out['accept_stat'], self.counter.idx, return_e=not last_burnin)
        self._iter += 1
        self.last = out
        if savestate:
            self.chain.detach_and_update(self.current)

    # -- blocks of draws per launch: HMC.run's loop on ey_nuts_run, with the two records a NUTS chain may ask for
    def _can_fuse(self, verbose):
        return (self.fused_block > 0 and self.batched and self.rng == 'philox' and not verbose
                and self.counter.num_batches == 1 and isinstance(self.chain, ChainBuffer)
                and set(self.chain.keys) <= {'sample', 'target_val', 'accepted', 'depth', 'divergent'})

    def _draw_block(self, x, y, k, savestate):
        plan = self.model._plan(x, y)
        rec = {}
        if savestate:
            C, dev = self.num_chains, self._theta.device
            views = self.chain.block(k, dict(sample=self._theta, target_val=self._target,
                                             accepted=torch.empty(C, dtype=torch.uint8, device=dev),
                                             depth=torch.empty(C, dtype=torch.int32, device=dev),
                                             divergent=torch.empty(C, dtype=torch.uint8, device=dev)))
            rec = dict(samples=views.get('sample'), targets=views.get('target_val'), accepted_rec=views.get('accepted'),
                       depth_rec=views.get('depth'), divergent_rec=views.get('divergent'))
        if not savestate and k > 1 and plan._moments is not None:
            for _ in range(k):  # attached chain moments are replayed from records a burn-in block does not keep
                out = self._run_block(plan, 1, {})
                self._iter += 1
        else:
            out = self._run_block(plan, k, rec)
            self._iter += k
        self._publish(out['accepted'])
        self._publish_nuts(out)
        self.last = out
        if savestate:
            self.chain.commit(k)

    def _run_block(self, plan, k, rec):
        step, step_vec = self._step_args()
        flags = self._flags(plan)
        return plan.nuts_run(self._theta, self._target, self._grad, step, self.max_depth, self._metric, self._metric_form,
                             k, index=self._metric_index, step_vec=step_vec, temp=self._temp(), seed=self.seed,
                             it=self._iter, chain_offset=self.chain_offset, flags=flags, **rec)

    # -- the hook of tuners.WindowedAdaptation.warm_up: the sampler's own warm-up launch (the tuner's num_steps is unused)
    def _warmup_launch(self, plan, num_steps, k, **kw):
        kw['flags'] = kw.get('flags', 0) | self._flags(plan)
        return plan.nuts_warmup(self._theta, self._target, self._grad, 0.0, self.max_depth, self._metric,
                                self._metric_form, k, **kw)
