"""Gibbs on the device (ey_gibbs_step / ey_gibbs_run, k_gibbs in eeyore_amd/csrc/ey_generic.hip) against the numpy
restatement of the reference's Gibbs.draw (tests/gibbs_restatement.py), the reference's own traces
(g12_gibbs_traces.npz), k_mh, and itself."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mlp_oracle as orc
from tests.gibbs_restatement import gibbs_draw, table_of
from tests.helpers import load

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_DECISION_TOL = 2e-3  # as tests/test_ram_gpu.py:19 and tests/test_gpu_parity.py
TINY_OFF, TINY_DYN = 1 << 8, 1 << 9  # ey_debug_set_variant: the LDS tile loop / the register evaluation whenever it fits

# name: (dims, activations, likelihood, rows, sub-step blocks or None = one block per node, variant)
#   mlp433: a compile-time shape; mlp433-lds: the same on the LDS tile loop; mlp322-dyn: TinyDyn; mlp2321: sub-blocks;
#   mlp483: a fused16 model (Gibbs routes it to k_gibbs); lr5: a table the MLP numbering does not produce
CASES = {
    "mlp433": ([4, 3, 3], [1, 0], 1, 150, None, 0),
    "mlp433-lds": ([4, 3, 3], [1, 0], 1, 150, None, TINY_OFF),
    "mlp322-dyn": ([3, 2, 2], [2, 0], 1, 70, None, TINY_DYN),
    "mlp2321": ([2, 3, 2, 1], [1, 2, 1], 0, 64, [[0, 1, 6], [2, 3, 7], [4, 5, 8], [9, 10, 11, 15], [12, 13], [14, 16],
                                                 [17, 18, 19]], 0),
    "mlp483": ([4, 8, 3], [1, 0], 1, 150, None, 0),
    "lr5": ([4, 1], [1], 0, 40, [[4], [0, 2], [1, 3]], 0),
}


def _node_blocks(dims):
    """One block per non-input node: its incoming weights and its bias (every layer with bias)."""
    out, start = [], 0
    for l in range(len(dims) - 1):
        din, dout = dims[l], dims[l + 1]
        out += [[start + n * din + i for i in range(din)] + [start + din * dout + n] for n in range(dout)]
        start += (din + 1) * dout
    return out


def _case(name):
    dims, acts, lik, N, blocks, variant = CASES[name]
    blocks = blocks or _node_blocks(dims)
    rng = np.random.default_rng(len(blocks))
    scales = (0.15 + 0.3 * rng.random(len(blocks))).tolist()
    return dims, acts, lik, N, blocks, scales, variant


def _data(dims, lik, N, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, dims[0]))
    if lik == 0:
        y = (rng.random((N, dims[-1])) < 0.5).astype(np.float64)
    else:
        y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    return x, y


def _plan(dims, acts, lik, x, y, dtype, variant=0, bias=None):
    from eeyore_amd.plan import Plan
    pl = Plan(dims, bias or [1] * (len(dims) - 1), acts, lik, dtype, DEV)
    if variant:
        pl.set_variant(variant)
    pl.set_data(torch.tensor(x, dtype=dtype, device=DEV), torch.tensor(y, dtype=dtype, device=DEV))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    return pl


def _target_fn(dims, acts, lik, x, y, temperature=None, bias=None):
    spec = orc.Spec(dims, acts, lik, bias=bias, temperature=temperature)
    return lambda th: float(orc.log_target(spec, np.asarray(th, np.float64), x, y))


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _start(pl, C, dtype, seed=0, temp=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    th = (0.3 * torch.randn(C, pl.P, generator=g, dtype=torch.float64)).to(device=DEV, dtype=dtype)
    lik, prior = pl.log_target(th, temp=temp)
    return th, (lik + prior).contiguous()


def _g12():
    z = load("g12_gibbs_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abcd"}


@pytest.mark.parametrize("name", list("abcd"))
def test_fixture_replay(name):
    """The reference's traces through ey_gibbs_step in 'reference' mode with the recorded draws, f64: every flag equal
    (the generator asserted a margin >= 1e-6 on every sub-step), tolerances of test_ram_gpu.py::test_fixture_replay."""
    rec = _g12()[name]
    f64 = torch.float64
    pl = _plan(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], f64,
               bias=rec["bias"].tolist())
    tb = pl.gibbs_table(*table_of(rec))
    th = _t(rec["theta0"], f64)[None].clone()
    tv = _t([rec["init_target"]], f64)
    in_margin = 0
    for it in range(rec["z"].shape[0]):
        out = pl.gibbs_step(th, tv, tb, z=_t(rec["z"][it], f64)[None], u=_t(rec["u"][it], f64)[None], mode="reference")
        lr = out["log_rate"][0].cpu().numpy()
        in_margin += int((np.abs(np.log(rec["u"][it]) - lr) <= 1e-9).sum())
        assert np.array_equal(out["accepted"][0].cpu().numpy(), rec["accepted"][it]), it
        np.testing.assert_allclose(th[0].cpu().numpy(), rec["sample"][it], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(tv.item(), rec["target_val"][it], rtol=1e-9)
    assert in_margin == 0


def restated_draw(name, C, mode, f32, with_temps=False):
    """Inputs of one draw for C chains and what the f64 restatement makes of them (from values rounded to f32 when the
    device will hold f32); the seed is chosen by the restatement alone, see the loop.  Returns the inputs, the per-chain results and the fraction of sub-steps whose decision is
    within the f32 tolerance of the boundary or follows such a sub-step in its draw (they are left out of the f32
    comparison).  Needs no GPU."""
    dims, acts, lik, N, blocks, scales, _ = _case(name)
    x, y = _data(dims, lik, N)
    P = orc.Spec(dims, acts, lik).P
    rd = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, np.float64))
    for seed in range(1000 * C + P, 1000 * C + P + 50):  # a condition on the INPUTS: the first seed that leaves out <= 1 %
        r = _restated(seed, rd, dims, acts, lik, x, y, P, C, blocks, scales, mode, with_temps)
        if r["left_out"] <= 0.01:
            return r
    raise AssertionError("no seed in range keeps 99 % of the sub-steps clear of the f32 decision tolerance")


def _restated(seed, rd, dims, acts, lik, x, y, P, C, blocks, scales, mode, with_temps):
    rng = np.random.default_rng(seed)
    th0, z, u = rd(0.3 * rng.standard_normal((C, P))), rd(rng.standard_normal((C, P))), rd(rng.random((C, len(blocks))))
    temps = rd(0.3 + 0.7 * rng.random(C)) if with_temps else None
    xr, yr, sr = rd(x), rd(y), rd(scales)
    want, left_out = [], 0
    for c in range(C):
        tf = _target_fn(dims, acts, lik, xr, yr, None if temps is None else float(temps[c]))
        w = gibbs_draw(tf, th0[c], tf(th0[c]), blocks, sr, z[c], u[c], mode=mode)
        close = w[4] <= F32_DECISION_TOL * np.maximum(1.0, np.abs(w[3]))
        first = int(np.argmax(close)) if close.any() else len(blocks)
        left_out += len(blocks) - first
        want.append(w + (first,))
    return dict(dims=dims, acts=acts, lik=lik, x=x, y=y, blocks=blocks, scales=scales, th0=th0, z=z, u=u, temps=temps,
                want=want, left_out=left_out / (C * len(blocks)))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["intended", "reference"])
@pytest.mark.parametrize("C", [1, 3, 64])
def test_one_draw_against_the_restatement(name, dtype, mode, C):
    f64 = dtype == torch.float64
    r = restated_draw(name, C, mode, not f64, with_temps=name == "mlp433")
    pl = _plan(r["dims"], r["acts"], r["lik"], r["x"], r["y"], dtype, variant=CASES[name][5])
    tb = pl.gibbs_table(r["blocks"], r["scales"])
    S = len(r["blocks"])
    th, zt, ut = _t(r["th0"], dtype), _t(r["z"], dtype), _t(r["u"], dtype)
    tt = None if r["temps"] is None else _t(r["temps"], dtype)
    tv = pl.log_target(th, temp=tt)
    tv = (tv[0] + tv[1]).contiguous()
    tv0 = tv.double().cpu().numpy()
    out = pl.gibbs_step(th, tv, tb, z=zt, u=ut, mode=mode, temp=tt)
    acc, lr = out["accepted"].cpu().numpy(), out["log_rate"].double().cpu().numpy()
    th1, tv1 = th.double().cpu().numpy(), tv.double().cpu().numpy()
    left_out = 0
    for c in range(C):
        w_th, w_tv, w_acc, w_lr, w_margin, first = r["want"][c]
        assert np.isfinite(tv0[c])
        n = S if f64 else first  # f32: compare up to the first sub-step inside the decision tolerance
        left_out += S - n
        if f64:
            assert (w_margin > 1e-9).all(), "seed puts an f64 decision on the boundary"
        assert np.array_equal(acc[c, :n], w_acc[:n]), (c, acc[c], w_acc)
        np.testing.assert_allclose(lr[c, :n], w_lr[:n], rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
        if n == S:
            np.testing.assert_allclose(th1[c], w_th, rtol=1e-12 if f64 else 1e-5, atol=1e-12 if f64 else 1e-5)
            np.testing.assert_allclose(tv1[c], w_tv, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
    assert left_out <= 0.02 * C * S, (left_out, C * S)


def test_restated_seeds_leave_out_at_most_two_percent():
    # the f64 restatement alone (no device): the seeds of test_one_draw_against_the_restatement keep 98 % of the sub-steps
    for name in CASES:
        for mode in ("intended", "reference"):
            assert restated_draw(name, 64, mode, True, with_temps=name == "mlp433")["left_out"] <= 0.02, (name, mode)


@pytest.mark.parametrize("name", ["mlp433", "mlp433-lds", "mlp483", "lr5"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_block_of_all_parameters_is_mh(name, dtype):
    """One block holding all P indices with scale s against ey_mh_step with the scale vector s on the generic kernel: state,
    target and flag bit-identical, with recorded draws and on Philox (sub-step 0 draws MH's accept variate)."""
    from eeyore_amd import _lib as L
    dims, acts, lik, N, _, _, variant = _case(name)
    x, y = _data(dims, lik, N)
    pl = _plan(dims, acts, lik, x, y, dtype, variant=variant)
    C, P, s = 37, pl.P, 0.21
    tb = pl.gibbs_table([list(range(P))], [s])
    rng = np.random.default_rng(3)
    z, u = _t(rng.standard_normal((C, P)), dtype), _t(rng.random(C), dtype)
    for mode in ("intended", "reference"):
        for recorded in (True, False):
            th_a, tv_a = _start(pl, C, dtype, seed=4)
            th_b, tv_b = th_a.clone(), tv_a.clone()
            for it in range(6):
                kw = dict(z=z, u=u) if recorded else dict(seed=12, it=it)
                a = pl.gibbs_step(th_a, tv_a, tb, mode=mode, **{**kw, **({"u": u[:, None].contiguous()} if recorded else {})})
                b = pl.mh_step(th_b, tv_b, torch.full((P,), s, dtype=dtype), flags=L.EY_FORCE_GENERIC, **kw)
                assert torch.equal(a["accepted"][:, 0], b["accepted"]) and torch.equal(th_a, th_b), (mode, recorded, it)
                assert torch.equal(tv_a, tv_b) and torch.equal(a["log_rate"][:, 0], b["log_rate"])
            assert 0 < int(a["accepted"].sum()) + int((th_a != _start(pl, C, dtype, seed=4)[0]).any())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_philox_uniform_blocks(dtype):
    dims, acts, lik, N, _, _, _ = _case("lr5")
    pl = _plan(dims, acts, lik, *_data(dims, lik, N), dtype)
    u = pl.philox_uniform_blocks(9, 7, 5, 3, chain_offset=2)
    assert torch.equal(u[:, 0], pl.philox_uniform(9, 5, 3, chain_offset=2))
    assert ((u >= 0) & (u < 1)).all() and u.unique().numel() == 63


@pytest.mark.parametrize("name,dtype,mode", [("mlp433", torch.float32, "intended"), ("mlp2321", torch.float64, "reference"),
                                             ("mlp483", torch.float32, "reference"), ("mlp433-lds", torch.float64, "intended")])
def test_run_equals_steps_bit_for_bit(name, dtype, mode):
    dims, acts, lik, N, blocks, scales, variant = _case(name)
    pl = _plan(dims, acts, lik, *_data(dims, lik, N), dtype, variant=variant)
    tb = pl.gibbs_table(blocks, scales)
    C, K, S = 64, 25, len(blocks)
    th_a, tv_a = _start(pl, C, dtype)
    th_b, tv_b = th_a.clone(), tv_a.clone()
    rs = torch.empty(K, C, pl.P, dtype=dtype, device=DEV)
    rt = torch.empty(K, C, dtype=dtype, device=DEV)
    ra = torch.empty(K, C, S, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(C, S, dtype=torch.int32, device=DEV)
    pl.gibbs_run(th_a, tv_a, tb, K, mode=mode, seed=9, it=11, samples=rs, targets=rt, accepted_rec=ra, accept_count=cnt)
    for k in range(K):
        # the step reproduces the stream from the exposed entry points too
        out = pl.gibbs_step(th_b, tv_b, tb, mode=mode, seed=9, it=11 + k) if k % 2 else \
            pl.gibbs_step(th_b, tv_b, tb, mode=mode, z=pl.philox_normal(C, 9, 11 + k),
                          u=pl.philox_uniform_blocks(C, S, 9, 11 + k))
        assert torch.equal(rs[k], th_b) and torch.equal(rt[k], tv_b) and torch.equal(ra[k], out["accepted"]), k
    assert torch.equal(th_a, th_b) and torch.equal(tv_a, tv_b)
    assert torch.equal(cnt, ra.int().sum(0)) and 0 < int(cnt.sum()) < C * K * S


def _iris_sampler(C, dtype, fused_block, stats=False, epochs=40, burnin=10, mode="intended"):
    from torch.utils.data import DataLoader
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import synthetic
    from eeyore_amd.distributed import ChainStats
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import Gibbs
    data = synthetic.iris_shaped(dtype=dtype, device=DEV)
    loader = DataLoader(data, batch_size=len(data))
    model = mlp.MLP(loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[4, 3, 3], activations=[torch.sigmoid, None]), dtype=dtype, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(1)
    th0 = (0.1 * torch.randn(C, 27, generator=g, dtype=torch.float64)).to(device=DEV, dtype=dtype)
    if C == 1:
        th0 = th0[0]
    s = Gibbs(model, theta0=th0, dataloader=loader, seed=4, scales=0.4, node_subblock_size=[2, None, 3, None, 2, None],
              mode=mode)
    s.fused_block = fused_block
    st = None
    if stats:
        st = ChainStats(C, 27, DEV)
        st.attach(model._plan(*next(iter(loader))))
    s.run(num_epochs=epochs, num_burnin_epochs=burnin)
    if stats:
        model._plan(*next(iter(loader))).detach_moments()
    return s, st


@pytest.mark.parametrize("stats", [False, True])
def test_sampler_run_in_blocks_equals_draws(stats):
    a, sa = _iris_sampler(32, torch.float32, 256, stats)
    b, sb = _iris_sampler(32, torch.float32, 0, stats)
    assert torch.equal(a._theta, b._theta) and torch.equal(a._target, b._target)
    ca, cb = a.get_chain(), b.get_chain()
    assert torch.equal(ca.get_samples(), cb.get_samples()) and torch.equal(ca.get_target_vals(), cb.get_target_vals())
    assert torch.equal(ca.get_accepted(), cb.get_accepted())
    S = a.num_substeps
    assert S == 8 and ca.get_samples().shape[0] == 30 and ca.get_accepted().shape == (30, 32, S)
    assert ca.acceptance_rate().shape == (32, S) and a.current['accepted'].shape == (32, S)
    if stats:
        torch.testing.assert_close(sa.s1, sb.s1, rtol=1e-12, atol=0)
        torch.testing.assert_close(sa.s2, sb.s2, rtol=1e-12, atol=0)
        assert torch.equal(sa.acc, sb.acc) and sa.n == sb.n == 40
        assert 0 < sa.acc.min().item() and sa.acc.max().item() < 40  # the accepted fraction of every draw's sub-steps


def test_single_chain_view():
    s, _ = _iris_sampler(1, torch.float64, 256, mode="reference")
    assert s.rng == 'torch' and s.current['sample'].shape == (27,) and s.current['accepted'].shape == (8,)
    chain = s.get_chain()
    assert len(chain) == 30 and chain.acceptance_rate().shape == (8,)
    s.reset(torch.zeros(27, dtype=torch.float64, device=DEV))
    assert s.current['accepted'] is None and len(s.get_chain()) == 0


@pytest.mark.parametrize("name,dtype", [("mlp433", torch.float32), ("mlp2321", torch.float64), ("mlp433-lds", torch.float32)])
def test_intended_mode_keeps_the_target_of_the_state(name, dtype):
    """After 200 Philox draws target[c] is the log-target of theta[c].  k_gibbs and the log-target kernel call the same
    evaluation form (eval_target of the same instantiation, one wave, the same LDS vector layout), so: bit-equal."""
    dims, acts, lik, N, blocks, scales, variant = _case(name)
    pl = _plan(dims, acts, lik, *_data(dims, lik, N), dtype, variant=variant)
    tb = pl.gibbs_table(blocks, scales)
    th, tv = _start(pl, 256, dtype, seed=6)
    pl.gibbs_run(th, tv, tb, 200, seed=3)
    lik_, prior = pl.log_target(th)
    assert torch.equal(tv, lik_ + prior)
    th2, tv2 = _start(pl, 256, dtype, seed=6)
    pl.gibbs_run(th2, tv2, tb, 200, seed=3, mode="reference")
    lik2, prior2 = pl.log_target(th2)
    assert not torch.equal(tv2, lik2 + prior2)  # the carried rejections show


def test_chain_independence_and_temperature():
    dims, acts, lik, N, blocks, scales, _ = _case("mlp433")
    pl = _plan(dims, acts, lik, *_data(dims, lik, N), torch.float32)
    tb = pl.gibbs_table(blocks, scales)
    th, tv = _start(pl, 1024, torch.float32, seed=2)
    one = [t[:1].clone() for t in (th, tv)]
    halves = [[t[:512].clone() for t in (th, tv)], [t[512:].clone() for t in (th, tv)]]
    pl.gibbs_run(th, tv, tb, 20, seed=5)
    pl.gibbs_run(*one, tb, 20, seed=5)
    pl.gibbs_run(*halves[0], tb, 20, seed=5)
    pl.gibbs_run(*halves[1], tb, 20, seed=5, chain_offset=512)
    for full, part in zip((th, tv), one):
        assert torch.equal(full[:1], part)
    for i, full in enumerate((th, tv)):
        assert torch.equal(full, torch.cat([halves[0][i], halves[1][i]]))
    # per-chain temperature: a chain at temperature t equals a launch that has only that chain at t
    temps = torch.linspace(0.2, 1.0, 8, device=DEV)
    th8, tv8 = _start(pl, 8, torch.float32, seed=3, temp=temps)
    solo = [(th8[c:c + 1].clone(), tv8[c:c + 1].clone()) for c in range(8)]
    pl.gibbs_run(th8, tv8, tb, 10, seed=7, temp=temps)
    for c, (a, b) in enumerate(solo):
        pl.gibbs_run(a, b, tb, 10, seed=7, temp=temps[c:c + 1], chain_offset=c)
        assert torch.equal(a[0], th8[c]) and torch.equal(b[0], tv8[c]), c
    assert not torch.equal(th8[0], _start(pl, 8, torch.float32, seed=3, temp=temps)[0][0])


def _padded(shape, dtype, fill, pad=64):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n].view(*shape)


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 5, 33])
@pytest.mark.parametrize("name", ["mlp2321", "mlp433-lds"])
def test_buffer_safety_on_a_fresh_plan(name, C, N):
    """Canaries around every buffer, read-only inputs keep their bits, small C and N on a plan whose first call this is."""
    dims, acts, lik, _, blocks, scales, variant = _case(name)
    x, y = _data(dims, lik, N)
    for dtype in (torch.float64, torch.float32):
        pl = _plan(dims, acts, lik, x, y, dtype, variant=variant)
        tb = pl.gibbs_table(blocks, scales)
        P, S, K = pl.P, len(blocks), 3
        g = torch.Generator(device="cpu").manual_seed(C)
        th0 = (0.3 * torch.randn(C, P, generator=g, dtype=torch.float64)).to(device=DEV, dtype=dtype)
        bufs = {}
        for key, shape, dt in (("th", (C, P), dtype), ("tv", (C,), dtype), ("z", (C, P), dtype), ("u", (C, S), dtype),
                               ("temp", (C,), dtype), ("acc", (C, S), torch.uint8), ("lr", (C, S), dtype),
                               ("rs", (K, C, P), dtype), ("rt", (K, C), dtype), ("ra", (K, C, S), torch.uint8),
                               ("cnt", (C, S), torch.int32)):
            bufs[key] = _padded(shape, dt, 77 if dt in (torch.uint8, torch.int32) else float("nan"))
        bufs["th"][1].copy_(th0)
        bufs["tv"][1].fill_(-1e30)  # every first sub-step accepts: the state moves
        bufs["z"][1].copy_(torch.randn(C, P, generator=g, dtype=torch.float64))
        bufs["u"][1].copy_(torch.rand(C, S, generator=g, dtype=torch.float64))
        bufs["temp"][1].fill_(0.7)
        bufs["cnt"][1].zero_()
        snap = {k: b.clone() for k, (b, _) in bufs.items()}
        v = {k: view for k, (_, view) in bufs.items()}
        pl.gibbs_step(v["th"], v["tv"], tb, z=v["z"], u=v["u"], temp=v["temp"], out=dict(accepted=v["acc"], log_rate=v["lr"]))
        pl.gibbs_run(v["th"], v["tv"], tb, K, temp=v["temp"], samples=v["rs"], targets=v["rt"], accepted_rec=v["ra"],
                     accept_count=v["cnt"], out=dict(accepted=v["acc"]))
        torch.cuda.synchronize()
        for k, (b, _) in bufs.items():
            same = (lambda p, q: torch.equal(p.view(torch.uint8), q.view(torch.uint8)))
            assert same(b[:64], snap[k][:64]) and same(b[-64:], snap[k][-64:]), k
        for k in ("z", "u", "temp"):
            assert torch.equal(bufs[k][0].view(torch.uint8), snap[k].view(torch.uint8)), k
        assert torch.isfinite(v["th"]).all() and torch.isfinite(v["rs"]).all() and torch.isfinite(v["rt"]).all()
        assert (v["acc"] <= 1).all() and (v["ra"] <= 1).all() and torch.equal(v["rs"][-1], v["th"])
        assert not torch.equal(v["th"], th0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["intended", "reference"])
def test_nan_proposal_rejects_its_substep(dtype, mode):
    # every row has y = 1 and a large first feature: a large first weight saturates the sigmoid to exactly 1 and the naive
    # BCE term log(1 - o) * (1 - y) = -inf * 0 is NaN (eeyore/stats/loss.py:2)
    N, P = 16, 5
    x = np.ones((N, 4)) * np.array([10.0, 0.1, 0.1, 0.1])
    pl = _plan([4, 1], [1], 0, x, np.ones((N, 1)), dtype)
    tb = pl.gibbs_table([[1, 2], [0], [3, 4]], [1.0, 1.0, 1.0])
    th = torch.zeros(1, P, dtype=dtype, device=DEV)
    lik, prior = pl.log_target(th)
    tv = (lik + prior).contiguous()
    z = _t([[500.0, 0.01, -0.01, 0.01, 0.0]], dtype)
    out = pl.gibbs_step(th, tv, tb, z=z, u=_t([[1e-30, 0.5, 1e-30]], dtype), mode=mode)
    acc, lr = out["accepted"][0].tolist(), out["log_rate"][0]
    assert acc[0] == 1 and acc[1] == 0 and torch.isnan(lr[1]) and torch.isfinite(th).all() and th[0, 0] == 0
    if mode == "intended":  # the NaN is gone with the restored block
        assert acc[2] == 1 and torch.isfinite(lr[2]) and th[0, 3] != 0
    else:  # carried: every later sub-step of the draw sees it
        assert acc[2] == 0 and torch.isnan(lr[2]) and th[0, 3] == 0
    lik2, prior2 = pl.log_target(th)
    assert torch.isfinite(tv).all() and (mode == "reference" or torch.equal(tv, lik2 + prior2))


def test_unsupported_and_invalid_inputs_fail_before_any_launch():
    dims, acts, lik, N, blocks, scales, _ = _case("mlp433")
    pl = _plan(dims, acts, lik, *_data(dims, lik, N), torch.float32)
    tb = pl.gibbs_table(blocks, scales)
    th, tv = _start(pl, 3, torch.float32)
    before = (th.clone(), tv.clone())
    acc = torch.full((3, len(blocks)), 9, dtype=torch.uint8, device=DEV)
    for bad_blocks, bad_scales in (([[0, 1], [1, 2]], [1.0, 1.0]), ([[0, 27]], [1.0]), ([[0], []], [1.0, 1.0]),
                                   ([], []), ([[0]], [float("nan")]), ([[0]], [0.0])):
        with pytest.raises(ValueError):
            pl.gibbs_table(bad_blocks, bad_scales)
    other = _plan([2, 2, 1], [1, 1], 0, *_data([2, 2, 1], 0, 8), torch.float32)
    with pytest.raises(ValueError, match="another model size"):  # a table built for another P
        pl.gibbs_step(th, tv, other.gibbs_table([[0, 1]], [1.0]), out=dict(accepted=acc, log_rate=None))
    with pytest.raises(ValueError, match="mode"):
        pl.gibbs_step(th, tv, tb, mode="carry")
    with pytest.raises(ValueError, match="n_iters"):
        pl.gibbs_run(th, tv, tb, 0, out=dict(accepted=acc))
    # a model beyond the 160 KiB LDS of a CU: EY_ERR_UNSUPPORTED
    big_dims = [4, 300, 3]
    big = _plan(big_dims, [1, 0], 1, *_data(big_dims, 1, 8), torch.float64)
    tb_big = big.gibbs_table([list(range(big.P))], [0.1])
    thb = torch.zeros(2, big.P, dtype=torch.float64, device=DEV)
    tvb = torch.zeros(2, dtype=torch.float64, device=DEV)
    accb = torch.full((2, 1), 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="status -2"):
        big.gibbs_step(thb, tvb, tb_big, out=dict(accepted=accb, log_rate=None))
    torch.cuda.synchronize()
    assert (acc == 9).all() and (accb == 9).all() and (thb == 0).all()
    assert torch.equal(th, before[0]) and torch.equal(tv, before[1])


def test_posterior_means_agree_with_hmc():
    """'intended' Gibbs against HMC of this package on the same plan, 4096 chains, logistic regression (4 features and a
    bias, 200 rows: a unimodal posterior): the per-parameter posterior means, pooled over the chains, agree within a
    multiple of the pooled Monte-Carlo standard error from chain.mc_se().  The multiple is measured here: twice the largest
    standardised difference between two HMC runs with different seeds, and never below 4 (the expected maximum of five
    standard normal differences is about 2.3).  It cannot pass by accident: the means lie many standard errors from the
    start of the chains, and 'reference' mode or a kernel that forgot a block would move them."""
    from eeyore_amd.chains import ChainBuffer
    dims, acts, lik = [4, 1], [1], 0
    x, y = _data(dims, lik, 200, seed=5)
    w = np.array([1.0, -0.5, 0.25, 0.8])
    y = (np.random.default_rng(6).random(200) < 1 / (1 + np.exp(-(x @ w + 0.3)))).astype(np.float64)[:, None]
    dtype = torch.float64
    pl = _plan(dims, acts, lik, x, y, dtype)
    C, P = 4096, pl.P

    def pooled(run, burn, keep, seed):
        th, tv = _start(pl, C, dtype, seed=seed)
        buf = ChainBuffer(keys=['sample'])
        run(th, tv, burn, None, seed, 0)
        views = buf.block(keep, dict(sample=th))
        run(th, tv, keep, views['sample'], seed, burn)
        buf.commit(keep)
        se = buf.mc_se() / keep ** 0.5  # [C, P]: mc_se() is the root of the asymptotic variance, as the reference's
        assert torch.isfinite(se).all()
        return buf.mean().mean(0).cpu().numpy(), (se.pow(2).sum(0).sqrt() / C).cpu().numpy()

    def hmc(th, tv, n, samples, seed, it):
        _, g = pl.log_target_grad(th)
        pl.hmc_run(th, tv, g.contiguous(), 0.08, 8, n, seed=seed, it=it, samples=samples)

    tb = pl.gibbs_table([[0, 1], [2, 3], [4]], [0.3, 0.3, 0.3])

    def gibbs(th, tv, n, samples, seed, it):
        pl.gibbs_run(th, tv, tb, n, seed=seed, it=it, samples=samples)

    m1, s1 = pooled(hmc, 200, 400, 11)
    m2, s2 = pooled(hmc, 200, 400, 12)
    mg, sg = pooled(gibbs, 400, 800, 13)
    r_hh = float(np.max(np.abs(m1 - m2) / np.sqrt(s1 ** 2 + s2 ** 2)))
    multiple = max(4.0, 2.0 * r_hh)
    r_g1 = float(np.max(np.abs(mg - m1) / np.sqrt(sg ** 2 + s1 ** 2)))
    r_g2 = float(np.max(np.abs(mg - m2) / np.sqrt(sg ** 2 + s2 ** 2)))
    print(f"HMC-HMC {r_hh:.2f}, Gibbs-HMC {r_g1:.2f} / {r_g2:.2f}, multiple {multiple:.2f}, means {m1}, se {sg}")
    assert np.max(np.abs(m1) / s1) > 50  # far from the chains' start: agreement is not the absence of movement
    assert r_g1 <= multiple and r_g2 <= multiple, (r_hh, r_g1, r_g2)


def test_example_runs():
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="33", EEYORE_EXAMPLE_CHAINS="96", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gibbs_mlp_iris.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "cceptance rate" in out.stdout and "sub-steps per draw: 9" in out.stdout
