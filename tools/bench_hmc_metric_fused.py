"""What HMC under a diagonal metric costs per leapfrog step on the matrix cores: ``hmc_metric_run`` with
EY_HMC_METRIC_FUSED on one MI355X, 4096 chains, MLP(4-32-32-3) on Iris (N = 150, P = 1315), f32, against the path it replaces
and against the fused HMC kernel without a metric.

    python tools/bench_hmc_metric_fused.py [--chains 4096] [--draws 25] [--steps 20] [--repeats 7] > profiles/hmc_metric_fused_bench.txt

A diagonal metric with scales in [0.5, 1.5], ``--steps`` leapfrog steps a draw, launches of ``--draws`` draws.  Three kinds
of launch alternate ``--repeats`` times in one process after a warm-up launch of each, every one timed between two device
events, restarted from the same state:
  (a) ``hmc_metric_run`` with EY_HMC_METRIC_FUSED: k_hmc_metric_mfma;
  (b) ``hmc_metric_run`` without it: k_hmc_metric on the generic evaluation, what served this plan before;
  (c) ``hmc_run`` on the same plan: k_mfma32, the same evaluations without a metric.
The median, the smallest and the largest time per leapfrog step are printed, then the two ratios against their bars:
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
from tools.bench_nuts_tree import DEV, F32, alternate, state


def line(name, ms, draws, steps, chains):
    per_step = [1e3 * t / (draws * steps) for t in ms]
    med = statistics.median(per_step)
    print(f"{name:44s} {med:9.1f} us per leapfrog step of {chains} chains (min {min(per_step):.1f}, max {max(per_step):.1f}; "
          f"{len(ms)} launches of {draws} draws x {steps} steps)")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=25)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    C, step = a.chains, 0.005
    print(f"# {torch.cuda.get_device_name(0)}; {C} chains, f32, {a.steps} leapfrog steps a draw, launches of {a.draws} draws")
    iris = XYDataset.from_eeyore('iris', yndmin=1, yonehot=True, dtype=F32, device=DEV)
    plan = Plan([4, 32, 32, 3], [1, 1, 1], [L.EY_ACT_SIGMOID, L.EY_ACT_SIGMOID, L.EY_ACT_NONE], L.EY_LIK_CE_SUM, F32, DEV)
    plan.set_data(iris.x.contiguous(), iris.y.contiguous())
    plan.set_prior(torch.zeros(plan.P), torch.full((plan.P,), 3.0).sqrt())
    scales = (0.5 + torch.rand(plan.P, generator=torch.Generator().manual_seed(2))).to(DEV)
    st = state(plan, C, 3)
    print(f"# MLP(4-32-32-3) on Iris, N = {len(iris)}, P = {plan.P}, kernel {plan.kernel}, products {plan.f32_products}, diagonal "
          f"metric with scales in [0.5, 1.5], step {step}")
    assert plan.hmc_metric_kernel(L.EY_HMC_METRIC_FUSED) == "mfma32" and plan.hmc_metric_kernel() == "generic"
    count = torch.zeros(C, dtype=torch.int32, device=DEV)

    def metric_launch(flags):
        def launch():
            th, tv, gr = (t.clone() for t in st)
            plan.hmc_metric_run(th, tv, gr, step, a.steps, scales, "diag", a.draws, seed=1, flags=flags, accept_count=count)
        return launch

    def hmc():
        th, tv, gr = (t.clone() for t in st)
        plan.hmc_run(th, tv, gr, step, a.steps, a.draws, seed=1, accept_count=count)

    rates = {}
    for name, fn in (("fused", metric_launch(L.EY_HMC_METRIC_FUSED)), ("parent", metric_launch(0))):  # both paths move alike
        count.zero_()
        fn()
        torch.cuda.synchronize()
        rates[name] = count.float().mean().item() / a.draws
    print(f"# acceptance of the first launch: {rates['fused']:.3f} with the bit, {rates['parent']:.3f} without")
    ms = alternate({"fused": metric_launch(L.EY_HMC_METRIC_FUSED), "parent": metric_launch(0), "hmc": hmc}, a.repeats)
    t_a = line("(a) hmc_metric_run, EY_HMC_METRIC_FUSED", ms["fused"], a.draws, a.steps, C)
    t_b = line("(b) hmc_metric_run, no bit (k_hmc_metric)", ms["parent"], a.draws, a.steps, C)
    t_c = line("(c) hmc_run (k_mfma32)", ms["hmc"], a.draws, a.steps, C)
    print(f"ratio (a) : (c), step under the metric : fused leapfrog step = {t_a / t_c:.3f}   (bar: <= 3; "
          f"{'met' if t_a <= 3 * t_c else 'MISSED'})")
    print(f"ratio (b) : (a), the path it replaces : the fused kernel = {t_b / t_a:.2f}   (bar: >= 5; "
          f"{'met' if t_b >= 5 * t_a else 'MISSED'})")


if __name__ == '__main__':
    main()
