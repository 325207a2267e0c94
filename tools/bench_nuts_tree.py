"""What the tree in device memory costs: time per leaf of ``nuts_run`` with EY_NUTS_TREE_DEVICE on one
MI355X, 4096 chains, f32, against code that was there before it.

    python tools/bench_nuts_tree.py [--chains 4096] [--draws 4] [--repeats 7] > profiles/nuts_tree_bench.txt

1. MLP(4-32-32-3) on Iris (N = 150, P = 1315) under a diagonal metric: a step so small that every tree stops at
   max_depth = 6 (checked from n_leapfrog and the depth record: 63 leaves a draw), against ``hmc_metric_run`` with 63
   leapfrog steps a draw under the same metric on the same plan -- the same evaluations, kicks and drifts without a tree.
2. N(0, Sigma) at P = 128 under a diagonal metric: the same trees with the flag and without (k_nuts, the tree in LDS).

Every figure is the time of one launch of ``--draws`` draws between two device events, after a warm-up launch of each
kind; the two kinds alternate ``--repeats`` times in one process, and the median, the smallest and the largest are
printed.  The chains restart from the same state before every launch, so every launch does the same work."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd import _lib as L
from eeyore_amd.datasets import XYDataset
from eeyore_amd.plan import Plan

DEV = "cuda:0"
F32 = torch.float32
MAX_DEPTH = 6
LEAVES = 2 ** MAX_DEPTH - 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(kinds, repeats):
    """kinds: {name: launch()}.  One warm-up launch each, then ``repeats`` rounds in turn: {name: [ms]}."""
    for fn in kinds.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in kinds}
    for _ in range(repeats):
        for k, fn in kinds.items():
            out[k].append(timed(fn))
    return out


def line(name, ms, draws, chains):
    per_leaf = [1e3 * t / (draws * LEAVES) for t in ms]
    med = statistics.median(per_leaf)
    print(f"{name:34s} {med:9.1f} us per leaf of {chains} chains (min {min(per_leaf):.1f}, max {max(per_leaf):.1f}; "
          f"{len(ms)} launches of {draws} draws x {LEAVES} leaves)")
    return med


def state(plan, C, seed):
    gen = torch.Generator().manual_seed(seed)
    th = (0.1 * torch.randn(C, plan.P, generator=gen)).to(DEV)
    tv, gr = plan.log_target_grad(th)
    return th, tv.contiguous(), gr.contiguous()


def nuts_launch(plan, st, step, scales, draws, flags, check):
    C = st[0].shape[0]
    depth_rec = torch.empty(draws, C, dtype=torch.int32, device=DEV)

    def launch():
        th, tv, gr = (t.clone() for t in st)
        out = plan.nuts_run(th, tv, gr, step, MAX_DEPTH, scales, "diag", draws, seed=1, flags=flags, depth_rec=depth_rec)
        if check:  # (outside the timed launches: the first call)
            torch.cuda.synchronize()
            assert bool((depth_rec == MAX_DEPTH).all()) and bool((out["n_leapfrog"] == LEAVES).all()), \
                "a tree stopped before max_depth: the step is too large for this comparison"
            assert int(out["divergent"].sum()) == 0 and bool(torch.isfinite(th).all())
    return launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    C = a.chains
    print(f"# {torch.cuda.get_device_name(0)}; {C} chains, f32, max_depth {MAX_DEPTH}: every tree has {LEAVES} leaves")

    # 1. the network
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=F32, device=DEV)
    plan = Plan([4, 32, 32, 3], [1, 1, 1], [L.EY_ACT_SIGMOID, L.EY_ACT_SIGMOID, L.EY_ACT_NONE], L.EY_LIK_CE_SUM, F32, DEV)
    plan.set_data(iris.x.contiguous(), iris.y.contiguous())
    plan.set_prior(torch.zeros(plan.P), torch.full((plan.P,), 3.0).sqrt())
    scales = (0.5 + torch.rand(plan.P, generator=torch.Generator().manual_seed(2))).to(DEV)
    st, step = state(plan, C, 3), 1e-4
    ws = plan.attach_nuts_tree(C, MAX_DEPTH)
    print(f"# 1. MLP(4-32-32-3) on Iris, N = {len(iris)}, P = {plan.P}, diagonal metric, step {step}; the tree's workspace: "
          f"{ws.numel()} bytes = {ws.numel() / 2 ** 20:.1f} MiB ({ws.numel() // C} a chain)")
    nuts_launch(plan, st, step, scales, a.draws, L.EY_NUTS_TREE_DEVICE, True)()

    def hmc():
        th, tv, gr = (t.clone() for t in st)
        plan.hmc_metric_run(th, tv, gr, step, LEAVES, scales, "diag", a.draws, seed=1)

    ms = alternate({"tree": nuts_launch(plan, st, step, scales, a.draws, L.EY_NUTS_TREE_DEVICE, False), "hmc": hmc},
                   a.repeats)
    t_tree = line("nuts_run, tree in device memory", ms["tree"], a.draws, C)
    t_hmc = line("hmc_metric_run, 63 steps a draw", ms["hmc"], a.draws, C)
    print(f"ratio, leaf of the tree : leapfrog step without one = {t_tree / t_hmc:.3f}")
    plan.detach_nuts_tree()

    # 2. P = 128: the same trees in LDS and in device memory
    P, draws2 = 128, 8 * a.draws   # (an evaluation of this target is short: more draws a launch)
    rng = np.random.default_rng(17)
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    cov = A @ A.T + 0.5 * np.eye(P)
    prec = np.linalg.inv(cov)
    mvn = Plan.mixture(np.ones(1), np.zeros((1, P)), ((prec + prec.T) / 2)[None], F32, DEV)
    scales = (0.5 + torch.rand(P, generator=torch.Generator().manual_seed(2))).to(DEV)
    st, step = state(mvn, C, 3), 1e-4
    ws = mvn.attach_nuts_tree(C, MAX_DEPTH)
    print(f"# 2. N(0, Sigma), P = {P}, diagonal metric, step {step}; the tree's workspace: {ws.numel() / 2 ** 20:.1f} MiB")
    for flags in (L.EY_NUTS_TREE_DEVICE, 0):
        nuts_launch(mvn, st, step, scales, draws2, flags, True)()
    ms = alternate({"tree": nuts_launch(mvn, st, step, scales, draws2, L.EY_NUTS_TREE_DEVICE, False),
                    "lds": nuts_launch(mvn, st, step, scales, draws2, 0, False)}, a.repeats)
    t_tree = line("nuts_run, tree in device memory", ms["tree"], draws2, C)
    t_lds = line("nuts_run, tree in LDS", ms["lds"], draws2, C)
    print(f"ratio, tree in device memory : tree in LDS = {t_tree / t_lds:.3f}")


if __name__ == '__main__':
    main()
