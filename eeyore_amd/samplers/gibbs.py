import json

import torch

from .base import SingleChainSerialSampler, default_counter
from eeyore_amd.itertools import chunk_evenly


class Gibbs(SingleChainSerialSampler):
    """Node-blocked Metropolis within Gibbs (eeyore/samplers/gibbs.py:10-102) as one ``ey_gibbs_step`` per draw: the
    parameter blocks of the model (``model.par_block_indices(b)``: the incoming weights and the bias of one node) are
    visited in order, each cut into sub-blocks by ``node_subblock_size[b]`` (``chunk_evenly``; ``None`` keeps the block
    whole); every sub-block gets a Normal random-walk proposal of scale ``scales[b]`` and its own accept/reject decision on
    the whole log-target.  All S sub-steps of a draw run inside one kernel.

    ``mode='intended'`` (default) restores a rejected sub-block before the next sub-step, a valid Metropolis-within-Gibbs.
    ``mode='reference'`` leaves it in the proposal vector for the rest of the draw as the reference does, so later
    sub-steps evaluate a vector the chain is not at.

    ``theta0`` [P] is the reference's single chain (random draws from the global torch generator in the reference's
    order: per sub-step the block's normals, then one uniform); [C, P] runs C chains on the in-kernel Philox streams.
    ``current['accepted']`` holds one flag per sub-step: [S] for a single chain, [C, S] otherwise."""

    keys = ['sample', 'target_val', 'accepted']

    def __init__(self, model, theta0=None, dataloader=None, data0=None, counter=None, scales=1., node_subblock_size=None,
                 chain=None, rng=None, seed=0, chain_offset=0, temperature=None, mode='intended'):
        if mode not in ('intended', 'reference'):
            raise ValueError(f"Gibbs: mode must be 'intended' or 'reference', got {mode!r}")
        if not hasattr(model, 'num_par_blocks'):
            raise NotImplementedError(
                f"Gibbs: {type(model).__name__} has no parameter blocks (the blocks are the nodes of an MLP); a "
                "DistributionModel is sampled with HMC, MALA, MetropolisHastings, RAM or AM")
        self.model, self.mode = model, mode
        nb = model.num_par_blocks()
        kw = dict(dtype=model.dtype, device=model.device)
        if isinstance(scales, (float, int)):
            self.scales = torch.full([nb], float(scales), **kw)
        elif isinstance(scales, torch.Tensor):
            self.scales = scales.to(**kw)
        elif isinstance(scales, (list, tuple)):
            self.scales = torch.tensor(scales, **kw)
        else:
            raise ValueError("Gibbs: scales must be a float, a list or a tensor with one entry per parameter block")
        if tuple(self.scales.shape) != (nb,):
            raise ValueError(f"Gibbs: the model has {nb} parameter blocks, scales has shape {tuple(self.scales.shape)}")
        if not bool((torch.isfinite(self.scales) & (self.scales > 0)).all()):
            raise ValueError("Gibbs: every scale must be a positive finite number")
        self.node_subblock_size = nb * [None] if node_subblock_size is None else list(node_subblock_size)
        if len(self.node_subblock_size) != nb:
            raise ValueError(f"Gibbs: the model has {nb} parameter blocks, node_subblock_size has "
                             f"{len(self.node_subblock_size)} entries")
        for size in self.node_subblock_size:
            if size is not None and (int(size) != size or size < 1):
                raise ValueError(f"Gibbs: a sub-block size must be None or a positive integer, got {size!r}")
        blocks, host_scales = self.get_blocks(), self.scales.cpu().tolist()
        self._substeps = [idx for per_block in blocks for idx in per_block]
        self._substep_scales = [host_scales[b] for b, per_block in enumerate(blocks) for _ in per_block]
        if not self._substeps:
            raise ValueError("Gibbs: node_subblock_size leaves no sub-block to visit (chunk_evenly gives no chunk for a "
                             "block shorter than its sub-block size)")
        self.num_substeps = len(self._substeps)
        super().__init__(default_counter(counter, dataloader))
        self._configure(model, dataloader, theta0, chain, rng, seed, chain_offset, temperature)
        self._table = None
        if theta0 is not None:
            self.set_current(theta0.clone().detach(), data=data0)

    # -- blocks
    def get_blocks(self):
        """For every parameter block b the list of its sub-blocks (index lists), as the reference's ``get_blocks``."""
        blocks = []
        for b in range(self.model.num_par_blocks()):
            indices = self.model.par_block_indices(b)
            size = self.node_subblock_size[b]
            blocks.append([indices] if size is None else list(chunk_evenly(indices, size)))
        return blocks

    def save_blocks(self, path='gibbs_lbocks.txt', mode='w'):
        with open(path, mode) as file:
            json.dump(self.get_blocks(), file)

    def _block_table(self, plan):
        """The device block table: built once per sampler (and again only if the model's plan was replaced)."""
        if self._table is None or self._table_plan is not plan:
            self._table, self._table_plan = plan.gibbs_table(self._substeps, self._substep_scales), plan
        return self._table

    # -- state
    def _accepted_shape(self):
        return (self.num_chains, self.num_substeps)

    def _evaluate_target(self, plan):
        lik, prior = plan.log_target(self._theta, temp=self._temp())
        self._target = lik + prior

    def set_current(self, theta, data=None):
        x, y = super().set_current(theta, data=data)
        self._theta = self._state_tensor(theta)
        self._evaluate_target(self.model._plan(x, y))
        self._publish(None)

    def _publish(self, accepted):
        cur = self.current
        cur['sample'] = self._expose(self._theta)
        cur['target_val'] = self._expose(self._target)
        cur['accepted'] = None if accepted is None else self._expose(accepted)
        if not self.batched:
            self.model.set_params(cur['sample'])

    def _torch_randoms(self):
        """z [C, P] and u [C, S] from the global torch generator in the reference's order: per sub-step the sub-block's
        normals (gibbs.py:84-86), then one uniform (:90).  Parameters outside every sub-block get no draw."""
        C, P = self._theta.shape
        z = torch.zeros(C, P, dtype=self.model.dtype, device=self.model.device)
        u = torch.empty(C, self.num_substeps, dtype=self.model.dtype, device=self.model.device)
        for s, idx in enumerate(self._substeps):
            z[:, idx] = self._randn(C, len(idx))
            u[:, s] = self._rand(C)
        return z, u

    def _run_block(self, plan, k, rec):
        return plan.gibbs_run(self._theta, self._target, self._block_table(plan), k, mode=self.mode, temp=self._temp(),
                              seed=self.seed, it=self._iter, chain_offset=self.chain_offset, **rec)

    def draw(self, x, y, savestate=False):
        plan = self.model._plan(x, y)
        if self.counter.num_batches != 1:  # gibbs.py:71-72
            self._evaluate_target(plan)
        z, u = self._torch_randoms() if self.rng == 'torch' else (None, None)
        out = plan.gibbs_step(self._theta, self._target, self._block_table(plan), z=z, u=u, mode=self.mode,
                              temp=self._temp(), seed=self.seed, it=self._iter, chain_offset=self.chain_offset)
        self._finish_draw(out, savestate)
