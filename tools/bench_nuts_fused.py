"""What NUTS on the matrix cores costs per leaf: ``nuts_run`` with EY_NUTS_FUSED on one MI355X, 4096 chains,
MLP(4-32-32-3) on Iris (N = 150, P = 1315), f32, against the path it replaces and against the fused HMC kernel.

    python tools/bench_nuts_fused.py [--chains 4096] [--draws 4] [--repeats 7] > profiles/nuts_fused_bench.txt

The shape of tools/bench_nuts_tree.py: a diagonal metric, max_depth 6 and a step of 1e-4, so small that every tree stops at
max_depth (checked from n_leapfrog and the depth record: 63 leaves a draw).  Three kinds of launch alternate ``--repeats``
times in one process after a warm-up launch of each, every one timed between two device events, restarted from the same
state:
  (a) ``nuts_run`` with EY_NUTS_FUSED: k_nuts_mfma;
  (b) ``nuts_run`` with EY_NUTS_TREE_DEVICE alone: k_nuts_ws on the generic evaluation, what served this plan before;
  (c) ``hmc_run`` with 63 leapfrog steps a draw on the same plan: k_mfma32, the same evaluations without a tree or a metric.
The median, the smallest and the largest time per leaf (or step) are printed, then the two ratios against their bars:
(a) <= 3 x (c), and (a) at least 5 times faster than (b)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd import _lib as L
from eeyore_amd.datasets import XYDataset
from eeyore_amd.plan import Plan
from tools.bench_nuts_tree import DEV, F32, LEAVES, MAX_DEPTH, alternate, line, nuts_launch, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    C = a.chains
    print(f"# {torch.cuda.get_device_name(0)}; {C} chains, f32, max_depth {MAX_DEPTH}: every tree has {LEAVES} leaves")
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=F32, device=DEV)
    plan = Plan([4, 32, 32, 3], [1, 1, 1], [L.EY_ACT_SIGMOID, L.EY_ACT_SIGMOID, L.EY_ACT_NONE], L.EY_LIK_CE_SUM, F32, DEV)
    plan.set_data(iris.x.contiguous(), iris.y.contiguous())
    plan.set_prior(torch.zeros(plan.P), torch.full((plan.P,), 3.0).sqrt())
    scales = (0.5 + torch.rand(plan.P, generator=torch.Generator().manual_seed(2))).to(DEV)
    st, step = state(plan, C, 3), 1e-4
    ws = plan.attach_nuts_tree(C, MAX_DEPTH)
    print(f"# MLP(4-32-32-3) on Iris, N = {len(iris)}, P = {plan.P}, kernel {plan.kernel}, products {plan.f32_products}, diagonal "
          f"metric, step {step}; the tree's workspace: {ws.numel() / 2 ** 20:.1f} MiB ({ws.numel() // C} bytes a chain)")
    assert plan.nuts_kernel(L.EY_NUTS_FUSED) == "mfma32" and plan.nuts_kernel(L.EY_NUTS_TREE_DEVICE) == "generic"
    for flags in (L.EY_NUTS_FUSED, L.EY_NUTS_TREE_DEVICE):  # every tree has 63 leaves, on both paths
        nuts_launch(plan, st, step, scales, a.draws, flags, True)()

    def hmc():
        th, tv, gr = (t.clone() for t in st)
        plan.hmc_run(th, tv, gr, step, LEAVES, a.draws, seed=1)

    ms = alternate({"fused": nuts_launch(plan, st, step, scales, a.draws, L.EY_NUTS_FUSED, False),
                    "parent": nuts_launch(plan, st, step, scales, a.draws, L.EY_NUTS_TREE_DEVICE, False), "hmc": hmc}, a.repeats)
    t_a = line("(a) nuts_run, EY_NUTS_FUSED", ms["fused"], a.draws, C)
    t_b = line("(b) nuts_run, EY_NUTS_TREE_DEVICE", ms["parent"], a.draws, C)
    t_c = line("(c) hmc_run, 63 steps a draw", ms["hmc"], a.draws, C)
    print(f"ratio (a) : (c), leaf of the fused tree : fused leapfrog step = {t_a / t_c:.3f}   (bar: <= 3; "
          f"{'met' if t_a <= 3 * t_c else 'MISSED'})")
    print(f"ratio (b) : (a), the path it replaces : the fused kernel = {t_b / t_a:.2f}   (bar: >= 5; "
          f"{'met' if t_b >= 5 * t_a else 'MISSED'})")
    plan.detach_nuts_tree()


if __name__ == '__main__':
    main()
