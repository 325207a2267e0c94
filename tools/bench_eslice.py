"""Elliptical slice sampling on four plans at 4096 chains: draws per second, evaluations per draw, time per
evaluation -- and, for the plans whose ``plan.kernel`` is 'generic', ``ey_mh_run``'s time per draw beside it in the same
process: a random-walk MH draw and one point of an elliptical slice draw are both one value-only evaluation on the generic
kernels plus passes over [P], so the ratio of the two should be near 1.

    python tools/bench_eslice.py [--chains 4096] [--draws 64] [--repeats 5] [--window 0.25] > profiles/eslice_bench.txt

Plans: the headline model MLP(4-32-32-3) on the iris-shaped batch in f32 (plan.kernel 'mfma32': the sampler runs on the
generic evaluation all the same); MLP(2-2-1) on XOR (the register-resident evaluation); a linear regression of dims [12, 1]
on 70 rows (the LDS tile loop); a 32-parameter normal with a base 1.5 times its marginal scale.  Chains start from draws of
the base.  Times are device events around a window of launches of ``--draws`` draws each, back to back and about
``--window`` seconds long, after warm-up launches; the median of ``--repeats`` windows, every launch going on from the state
the one before left; the two samplers alternate window by window."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeyore_amd import _lib as L
from eeyore_amd.datasets import synthetic
from eeyore_amd.plan import Plan

DEV = torch.device("cuda", 0)
F32 = torch.float32


def _t(a, dtype=F32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def plans():
    """(name, plan, base (loc, scale) or None, the scale chains start at) for the four plans."""
    rng = np.random.default_rng(0)
    xs, ys = synthetic.iris_shaped_arrays(seed=0)
    head = Plan([4, 32, 32, 3], [1, 1, 1], [1, 1, 0], 1, F32, DEV)
    head.set_data(_t(xs), _t(ys))
    head.set_prior(torch.zeros(head.P), torch.full((head.P,), float(np.sqrt(3.0))))
    yield "MLP(4-32-32-3) iris f32", head, None, float(np.sqrt(3.0))
    xor = Plan([2, 2, 1], [1, 1], [1, 1], 0, F32, DEV)
    xor.set_data(_t([[0, 0], [0, 1], [1, 0], [1, 1]]), _t([[0], [1], [1], [0]]))
    xor.set_prior(torch.zeros(xor.P), torch.ones(xor.P))
    yield "MLP(2-2-1) xor f32", xor, None, 1.0
    x = rng.standard_normal((70, 12))
    y = x @ (0.8 * np.cos(1.3 * np.arange(12))) + 0.2 + 0.7 * rng.standard_normal(70)
    reg = Plan([12, 1], [1], [0], L.EY_LIK_GAUSS_SUM, F32, DEV)
    reg.set_data(_t(x), _t(y[:, None]))
    reg.set_prior(torch.zeros(reg.P), torch.full((reg.P,), 2.0))
    reg.set_lik_scale(0.7)
    yield "regression [12, 1] N = 70 f32", reg, None, 2.0
    P = 32
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    cov = A @ A.T + 0.5 * np.eye(P)
    prec = np.linalg.inv(cov)
    c = -0.5 * (P * np.log(2 * np.pi) + np.linalg.slogdet(cov)[1])
    mvn = Plan.mixture([c], np.zeros((1, P)), ((prec + prec.T) / 2)[None], F32, DEV)
    scale = 1.5 * np.sqrt(np.diag(cov))
    yield "normal P = 32 with a base f32", mvn, (_t(np.zeros(P)), _t(scale)), scale


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    a = ap.parse_args()
    C, K = a.chains, a.draws
    print(f"# tools/bench_eslice.py: {C} chains, {K} draws per launch, median of {a.repeats} windows of about {a.window} s; "
          f"{torch.cuda.get_device_name(0)}")
    print("# plan | plan.kernel | draws/s x chains | evaluations per draw: mean, max | time per evaluation (all chains) | "
          "ey_mh_run per draw | ratio")
    for name, pl, base, start in plans():
        gen = torch.Generator().manual_seed(1)
        th = (torch.randn(C, pl.P, generator=gen) * torch.as_tensor(start, dtype=F32)).to(DEV).contiguous()
        kw = dict(base_loc=None, base_scale=None) if base is None else dict(base_loc=base[0], base_scale=base[1])
        ell, tv = pl.eslice_ell(th, **kw)
        rec = torch.zeros(K, C, dtype=torch.int32, device=DEV)
        generic = pl.kernel == "generic"
        th2 = th.clone()
        lik, prior = pl.log_target(th2)
        tv2 = (lik + prior).contiguous()
        it = [0]

        def es():
            pl.eslice_run(th, tv, ell, K, seed=3, it=it[0], n_evals_rec=rec, **kw)

        def mh():
            pl.mh_run(th2, tv2, 0.02, K, seed=3, it=it[0])
        es()
        if generic:
            mh()
        torch.cuda.synchronize()
        # a timed window is n launches back to back, n such that it lasts about a.window seconds
        n = max(1, min(512, int(a.window / max(timed(es), 1e-5))))

        def many(fn):
            def run():
                for _ in range(n):
                    fn()
                    it[0] += K
            return run
        t_es, t_mh, means, maxes = [], [], [], []
        for r in range(a.repeats):
            t_es.append(timed(many(es)) / n)
            means.append(float(rec.double().mean()))   # (of the window's last launch)
            maxes.append(int(rec.max()))
            if generic:
                t_mh.append(timed(many(mh)) / n)
        sec, mean = statistics.median(t_es), statistics.median(means)
        per_eval = sec / (K * mean)
        line = (f"{name} | {pl.kernel} | {C * K / sec:.4e} | {mean:.2f}, {max(maxes)} | {per_eval * 1e6:.2f} us | ")
        if generic:
            per_mh = statistics.median(t_mh) / K
            line += f"{per_mh * 1e6:.2f} us | {per_eval / per_mh:.2f}"
        else:
            line += "- | -"
        print(line + f"   ({n} launches a window; per launch: {', '.join(f'{t * 1e3:.3f}' for t in t_es)} ms)")


if __name__ == '__main__':
    main()
