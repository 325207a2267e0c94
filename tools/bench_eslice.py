"""Elliptical slice sampling on four plans at 4096 chains: draws per second, evaluations per draw, time per
evaluation -- and, for the plans whose ``plan.kernel`` is 'generic', ``ey_mh_run``'s time per draw beside it in the same
process: a random-walk MH draw and one point of an elliptical slice draw are both one value-only evaluation on the generic
kernels plus passes over [P], so the ratio of the two should be near 1.

    python tools/bench_eslice.py [--chains 4096] [--draws 64] [--repeats 5] [--window 0.25] > profiles/eslice_bench.txt

Plans: the headline model MLP(4-32-32-3) on the iris-shaped batch in f32 (plan.kernel 'mfma32': since DESIGN.md 4.26 the
sampler runs on the matrix cores there -- profiles/eslice_bench.txt was taken on the generic evaluation, see ``--fused``); MLP(2-2-1) on XOR (the register-resident evaluation); a linear regression of dims [12, 1]
on 70 rows (the LDS tile loop); a 32-parameter normal with a base 1.5 times its marginal scale.  Chains start from draws of
the base.  Times are device events around a window of launches of ``--draws`` draws each, back to back and about
``--window`` seconds long, after warm-up launches; the median of ``--repeats`` windows, every launch going on from the state
the one before left; the two samplers alternate window by window.

    python tools/bench_eslice.py --fused [...] > profiles/eslice_fused_bench.txt

The headline plan alone, three figures from one process: the time per evaluation of the fused kernel on the
matrix cores (k_eslice_mfma), the same under EY_FORCE_GENERIC (k_eslice), and ``ey_mh_run``'s time per draw on the matrix
cores -- one value-only fused evaluation per draw, what a point of the ellipse costs at best.  The three alternate window
by window; each path goes on from its own state."""
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


def fused(a):
    """The headline plan: fused, forced generic, ey_mh_run."""
    C, K = a.chains, a.draws
    name, pl, _, start = next(plans())
    assert pl.kernel == "mfma32" and pl.eslice_kernel() == "mfma32" and pl.eslice_kernel(L.EY_FORCE_GENERIC) == "generic"
    gen = torch.Generator().manual_seed(1)
    th0 = (torch.randn(C, pl.P, generator=gen) * start).to(DEV).contiguous()
    state = {}
    for key in ("fused", "generic"):
        th = th0.clone()
        ell, tv = pl.eslice_ell(th)
        state[key] = (th, tv.contiguous(), ell.contiguous(), torch.zeros(K, C, dtype=torch.int32, device=DEV))
    th2 = th0.clone()
    lik, prior = pl.log_target(th2)
    tv2 = (lik + prior).contiguous()
    it = [0]

    def es(key):
        th, tv, ell, rec = state[key]
        return lambda: pl.eslice_run(th, tv, ell, K, seed=3, it=it[0], n_evals_rec=rec,
                                     flags=L.EY_FORCE_GENERIC if key == "generic" else 0)

    def mh():
        pl.mh_run(th2, tv2, 0.02, K, seed=3, it=it[0])
    runs = dict(fused=es("fused"), generic=es("generic"), mh=mh)
    n = {}
    for key, fn in runs.items():   # warm-up, and the launches of a window
        fn()
        torch.cuda.synchronize()
        n[key] = max(1, min(512, int(a.window / max(timed(fn), 1e-5))))
    times = {key: [] for key in runs}
    means = {key: [] for key in ("fused", "generic")}
    maxes = {key: [] for key in ("fused", "generic")}
    for r in range(a.repeats):
        for key, fn in runs.items():
            def window():
                for _ in range(n[key]):
                    fn()
                    it[0] += K
            times[key].append(timed(window) / n[key])
            if key in means:
                means[key].append(float(state[key][3].double().mean()))
                maxes[key].append(int(state[key][3].max()))
    print(f"# tools/bench_eslice.py --fused: {name}, {C} chains, {K} draws per launch, median of {a.repeats} windows of about "
          f"{a.window} s, the three paths alternating; {torch.cuda.get_device_name(0)}")
    print("# path | kernel | draws/s x chains | evaluations per draw: mean, max | time per evaluation (all chains)")
    per = {}
    for key in ("fused", "generic"):
        sec, mean = statistics.median(times[key]), statistics.median(means[key])
        per[key] = sec / (K * mean)
        kern = pl.eslice_kernel(L.EY_FORCE_GENERIC if key == "generic" else 0)
        print(f"eslice_run {key} | {kern} | {C * K / sec:.4e} | {mean:.2f}, {max(maxes[key])} | {per[key] * 1e6:.2f} us   "
              f"({n[key]} launches a window; per launch: {', '.join(f'{t * 1e3:.3f}' for t in times[key])} ms)")
    per_mh = statistics.median(times["mh"]) / K
    print(f"mh_run | {pl.kernel} | {C * K / (per_mh * K):.4e} | 1 | {per_mh * 1e6:.2f} us per draw   "
          f"({n['mh']} launches a window; per launch: {', '.join(f'{t * 1e3:.3f}' for t in times['mh'])} ms)")
    print(f"fused / generic, per evaluation: {per['fused'] / per['generic']:.3f}   (generic / fused: {per['generic'] / per['fused']:.2f} x)")
    print(f"fused evaluation / mh_run draw: {per['fused'] / per_mh:.2f}")
    return 0 if per["fused"] < per["generic"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", action="store_true", help="the headline plan: fused, forced generic and ey_mh_run")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    a = ap.parse_args()
    if a.fused:
        sys.exit(fused(a))
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
