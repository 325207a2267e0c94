#!/usr/bin/env python3
"""Host time per call of plan.mh_step / ram_step / hmc_step (in-kernel Philox) on MLP(2-2-1) f32, 64 chains: a toy size on
purpose, so that what is timed is the path from Python to the launch.

    python tools/bench_entry_calls.py                          one line: mh ram hmc, microseconds per call, of this tree
    python tools/bench_entry_calls.py --against OTHER_TREE     OTHER_TREE (a built checkout, e.g. of the parent commit) and
                                                               this tree alternated, --repeats processes each, then the
                                                               medians and OTHER_TREE's own spread (max - min)

Each figure is --calls back-to-back calls ending in a device synchronise, after --warmup calls, in a process of its own."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(root, calls, warmup):
    sys.path.insert(0, root)
    import torch
    import eeyore_amd
    from eeyore_amd.plan import Plan
    assert os.path.abspath(eeyore_amd.__file__).startswith(os.path.abspath(root)), eeyore_amd.__file__
    dev = torch.device("cuda", 0)
    pl = Plan([2, 2, 1], [1, 1], [1, 1], 0, torch.float32, dev)
    x = torch.randn(4, 2, generator=torch.Generator().manual_seed(0))
    pl.set_data(x.to(dev), torch.tensor([[0.], [1.], [1.], [0.]], device=dev))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    C = 64
    th = 0.1 * pl.philox_normal(C, seed=1, it=0)
    t, gr = pl.log_target_grad(th)
    chol = torch.eye(pl.P, device=dev).repeat(C, 1, 1).contiguous()
    scale = torch.full((pl.P,), 0.1, device=dev)
    steps = (lambda i: pl.mh_step(th, t, scale, seed=2, it=i), lambda i: pl.ram_step(th, t, chol, i + 1, seed=3, it=i),
             lambda i: pl.hmc_step(th, t, gr, 0.05, 2, seed=4, it=i))
    out = []
    for f in steps:
        for i in range(warmup):
            f(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls):
            f(warmup + i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--against", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    a = ap.parse_args()
    if a.against is None:
        print(" ".join(f"{v:.3f}" for v in one(a.root, a.calls, a.warmup)), flush=True)
        sys.exit(0)
    rows = {"other": [], "this": []}
    print("repeat   tree     mh_step   ram_step   hmc_step")
    for r in range(a.repeats):
        for name, root in (("other", os.path.abspath(a.against)), ("this", HERE)):
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--calls", str(a.calls),
                                   "--warmup", str(a.warmup)], check=True, capture_output=True, text=True, timeout=300).stdout
            rows[name].append([float(v) for v in line.split()])
            print(f"{r + 1:<8} {name:<7} " + "  ".join(f"{v:9.3f}" for v in rows[name][-1]), flush=True)
    for j, step in enumerate(("mh_step", "ram_step", "hmc_step")):
        o, n = [r[j] for r in rows["other"]], [r[j] for r in rows["this"]]
        mo, mn, spread = statistics.median(o), statistics.median(n), max(o) - min(o)
        print(f"{step:<9} other median {mo:.3f} (min {min(o):.3f}, max {max(o):.3f}, spread {spread:.3f})   this median "
              f"{mn:.3f}   this - other {mn - mo:+.3f}: {'within' if mn - mo <= spread else 'BEYOND'} the other's spread")
