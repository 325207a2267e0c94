"""AM on the device (ey_am_step / ey_am_run, k_am in eeyore_amd/csrc/ey_generic.hip) against the numpy restatement of the
reference's AM.draw (tests/am_restatement.py), the reference's own traces (g13_am_traces.npz), k_mh, and itself."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mlp_oracle as orc
from tests.am_restatement import am_draw
from tests.helpers import load

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_DECISION_TOL = 2e-3  # as tests/test_ram_gpu.py

# (dims, activations, likelihood, rows): LR(4+bias); the register-evaluated tiny MLP(2-3-2-1); MLP(4-3-3) CE;
# LR(64+bias), P = 65, the first size that needs row lane + 64; MLP(6-14-2) CE, P = 128, the limit
CASES = {
    "lr5": ([4, 1], [1], 0, 40),
    "mlp2321": ([2, 3, 2, 1], [1, 2, 1], 0, 64),
    "mlp433": ([4, 3, 3], [1, 0], 1, 150),
    "lr65": ([64, 1], [1], 0, 16),
    "mlp6142": ([6, 14, 2], [2, 0], 1, 100),
}


def _data(dims, lik, N, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, dims[0]))
    if dims[0] > 16:
        x /= np.sqrt(dims[0])  # logits of order one whatever the width
    if lik == 0:
        y = (rng.random((N, dims[-1])) < 0.5).astype(np.float64)
    else:
        y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    return x, y


def _plan(dims, acts, lik, x, y, dtype):
    from eeyore_amd.plan import Plan
    pl = Plan(dims, [1] * (len(dims) - 1), acts, lik, dtype, DEV)
    pl.set_data(torch.tensor(x, dtype=dtype, device=DEV), torch.tensor(y, dtype=dtype, device=DEV))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    return pl


def _case_plan(name, dtype):
    dims, acts, lik, N = CASES[name]
    x, y = _data(dims, lik, N)
    return _plan(dims, acts, lik, x, y, dtype), (dims, acts, lik, x, y)


def _target_fn(dims, acts, lik, x, y):
    spec = orc.Spec(dims, acts, lik)
    return lambda th: float(orc.log_target(spec, np.asarray(th, np.float64), x, y))


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.double().cpu().numpy()


def _spd(C, P, rng, scale):
    out = np.empty((C, P, P))
    for c in range(C):
        A = rng.standard_normal((P, P)) / np.sqrt(P)
        out[c] = scale * (A @ A.T + 0.5 * np.eye(P))
    return out


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)


def _lower(a):
    return np.tril(a)


# the scenarios of one step: (name, idx, offset, t0, num_accepted before, what u_mix does, force an accept)
T0, OFF, LMIX = 6, 2, 0.25
SCENARIOS = [
    ("n<t0", 4, OFF, T0, 2, None, False),
    ("n=t0,none accepted", T0 - 1 + OFF, OFF, T0, 0, None, False),
    ("n=t0,some accepted", T0 - 1 + OFF, OFF, T0, 3, None, False),
    ("n>t0,u_mix around l", 20, OFF, T0, 4, "straddle", False),
    ("n>t0,none accepted", 20, OFF, T0, 0, "straddle", False),
    ("idx=0,accept", 0, 0, T0, 0, None, True),
]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("C", [1, 3, 65])
def test_one_step_against_the_restatement(name, dtype, C):
    pl, (dims, acts, lik, x, y) = _case_plan(name, dtype)
    tf = _target_fn(dims, acts, lik, x, y)
    P = pl.P
    f64 = dtype == torch.float64
    eps, b, c = 1e-3, 2.38 / np.sqrt(P), 0.05
    sc = 0.02 if P > 60 else 0.1
    below, above = np.nextafter(np.float32(LMIX), np.float32(0)), np.nextafter(np.float32(LMIX), np.float32(1))
    decided = factored = 0
    for si, (label, idx, offset, t0, nacc0, mix, force) in enumerate(SCENARIOS):
        rng = np.random.default_rng(1000 * si + C + P)
        n = idx + 1 - offset
        hist = sc * rng.standard_normal((max(n - 1, 1), C, P))  # the states the sums were built from
        th0 = hist[-1].copy()
        mean0 = hist.mean(0) if n > 1 else np.zeros((C, P))
        cs0 = np.einsum("kci,kcj->cij", hist, hist) if n > 1 else np.zeros((C, P, P))
        cov_init, cov0 = _spd(C, P, rng, sc * sc), _spd(C, P, rng, sc * sc)
        z = rng.standard_normal((C, P))
        u = np.full(C, 1e-30) if force else rng.random(C)
        um = np.where(np.arange(C) % 2 == 0, above, below).astype(np.float64) if mix else rng.random(C)
        th, mean, cs, cov = _t(th0, dtype), _t(mean0, dtype), _t(cs0, dtype), _t(cov_init, dtype)
        c0, zt, ut, umt = _t(cov0, dtype), _t(z, dtype), _t(u, dtype), _t(um, dtype)
        nacc, bd = _i32(np.full(C, nacc0)), _i32(np.zeros(C))
        # the restatement starts from the values the device holds (f32: rounded)
        th0, mean0, cs0, cov_init, cov0, z, u, um = (_np(v) for v in (th, mean, cs, cov, c0, zt, ut, umt))
        tv = pl.log_target(th)
        tv = (tv[0] + tv[1]).contiguous()
        tv0 = _np(tv)
        out = pl.am_step(th, tv, mean, cs, cov, nacc, c0, idx, l=LMIX, b=b, c=c, eps=eps, t0=t0, offset=offset, z=zt,
                         u_mix=umt, u=ut, breakdowns=bd)
        acc, br, lr_dev = out["accepted"].cpu().numpy(), out["branch"].cpu().numpy(), _np(out["log_rate"])
        th1, tv1, mean1, cs1, cov1 = (_np(v) for v in (th, tv, mean, cs, cov))
        assert (bd == 0).all(), label
        for ch in range(C):
            want = am_draw(tf, th0[ch], float(tv0[ch]), mean0[ch], cs0[ch], cov_init[ch], nacc0, cov0[ch], z[ch], um[ch],
                           u[ch], idx, offset, LMIX, b, c, t0, eps)
            assert br[ch] == want["branch"], (label, ch)
            if mix:
                assert br[ch] == (1 if ch % 2 == 0 else 0), (label, ch)
            factored += int(br[ch] == 1)
            lr_ref = want["log_rate"]
            np.testing.assert_allclose(lr_dev[ch], lr_ref, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
            tol = 1e-9 if f64 else F32_DECISION_TOL * max(1.0, abs(lr_ref))
            if not abs(np.log(u[ch]) - lr_ref) > tol:
                continue  # a margin case: the two may decide differently
            decided += 1
            assert bool(acc[ch]) == want["accepted"], (label, ch, lr_ref, np.log(u[ch]))
            if force:
                assert acc[ch] == 1 and int(nacc[ch]) == 0, label  # idx = 0: accepted, not counted (am.py:85)
            assert int(nacc[ch]) == want["num_accepted"], (label, ch)
            kw = dict(rtol=1e-12, atol=1e-12) if f64 else dict(rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(th1[ch], want["theta"], **kw)
            np.testing.assert_allclose(tv1[ch], want["target"], rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
            np.testing.assert_allclose(mean1[ch], want["mean"], **kw)
            # sums of products of O(sc) states: a few roundings of the largest entry
            big = max(np.abs(want["cov_sum"]).max(), 1e-30)
            np.testing.assert_allclose(_lower(cs1[ch]), _lower(want["cov_sum"]), rtol=0, atol=(1e-14 if f64 else 1e-6) * big)
            # (cov_sum - n m m^T) / (n - 1): four roundings of entries of the size of cov_sum, divided by n - 1; 1e-6
            # (f32, 2^-24 = 6e-8 each) and 1e-14 (f64) of its largest entry bound them
            np.testing.assert_allclose(_lower(cov1[ch]), _lower(want["cov"]), rtol=1e-12 if f64 else 1e-5,
                                       atol=(1e-14 if f64 else 1e-6) * big)
            if n >= t0 and nacc0 == 0 and want["num_accepted"] == 0:
                assert (np.tril(cov1[ch]) == np.tril(cov0[ch])).all(), label  # cov0' as it is, not transformed again
            if n < t0:
                assert (cov1[ch] == cov_init[ch]).all(), label
    assert decided >= len(SCENARIOS) * max(1, C - 3)
    assert factored >= 2 * ((C + 1) // 2)


def _g13():
    z = load("g13_am_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abcd"}


@pytest.mark.parametrize("name", list("abcd"))
def test_fixture_replay(name):
    rec = _g13()[name]
    f64 = torch.float64
    pl = _plan(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], f64)
    P = pl.P
    th = _t(rec["theta0"], f64)[None].clone()
    tv = _t([rec["init_target"]], f64)
    mean, cs = torch.zeros(1, P, dtype=f64, device=DEV), torch.zeros(1, P, P, dtype=f64, device=DEV)
    c0 = _t(rec["cov0"], f64)
    cov = c0[None].clone()
    nacc, bd = _i32([0]), _i32([0])
    par = dict(l=float(rec["l"]), b=float(rec["b"]), c=float(rec["c"]), eps=float(rec["eps"]), t0=int(rec["t0"]),
               offset=int(rec["offset"]))
    in_margin, k, factored = 0, 0, 0
    for it in range(rec["z"].shape[0]):
        out = pl.am_step(th, tv, mean, cs, cov, nacc, c0, int(rec["idx"][it]), z=_t(rec["z"][it], f64)[None],
                         u_mix=_t([rec["u_mix"][it]], f64), u=_t([rec["u"][it]], f64), breakdowns=bd, **par)
        if abs(np.log(float(rec["u"][it])) - out["log_rate"].item()) <= 1e-9:
            in_margin += 1
        factored += int(out["branch"].item() == 1)
        assert int(out["accepted"].item()) == int(rec["accepted"][it]), it
        np.testing.assert_allclose(th[0].cpu().numpy(), rec["sample"][it], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(tv.item(), rec["target_val"][it], rtol=1e-9)
        if k < len(rec["state_it"]) and rec["state_it"][k] == it:
            want = rec["cov"][k]
            got = np.tril(cov[0].cpu().numpy())
            assert np.linalg.norm(got - want) <= 1e-8 * np.linalg.norm(want), it
            np.testing.assert_allclose(mean[0].cpu().numpy(), rec["running_mean"][k], rtol=1e-8, atol=1e-9)
            assert int(nacc.item()) == int(rec["num_accepted"][k])
            k += 1
    assert in_margin == 0 and k == len(rec["state_it"]) and int(bd.item()) == 0
    after = rec["n"] > int(rec["t0"])
    assert factored == int((~(rec["u_mix"][after] < float(rec["l"]))).sum())


class _Replay:
    """torch.randn / torch.rand hand out the recorded draws in the recorded order; a call of the wrong kind, shape or at
    the wrong place fails."""

    def __init__(self, rec):
        self.items = []
        for it in range(rec["z"].shape[0]):
            self.items.append(("z", rec["z"][it]))
            if not np.isnan(rec["u_mix"][it]):
                self.items.append(("u", rec["u_mix"][it]))
            self.items.append(("u", rec["u"][it]))
        self.pos = 0

    def _next(self, kind, shape, kw):
        assert self.pos < len(self.items), "more random draws than the reference made"
        k, v = self.items[self.pos]
        assert k == kind, f"draw {self.pos}: the reference drew {k}, the sampler asks for {kind}"
        self.pos += 1
        return torch.tensor(np.asarray(v), dtype=kw.get("dtype"), device=kw.get("device")).reshape(shape)

    def __enter__(self):
        self._randn, self._rand = torch.randn, torch.rand
        torch.randn = lambda *shape, **kw: self._next("z", shape, kw)
        torch.rand = lambda *shape, **kw: self._next("u", shape, kw)
        return self

    def __exit__(self, *exc):
        torch.randn, torch.rand = self._randn, self._rand


def _lr_model(dtype):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import logistic_regression as lr
    return lr.LogisticRegression(loss_functions['binary_classification'], hparams=lr.Hyperparameters(input_size=4),
                                 dtype=dtype, device=DEV)


def _loader(x, y, dtype):
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import XYDataset
    data = XYDataset(torch.tensor(x, dtype=dtype, device=DEV), torch.tensor(y, dtype=dtype, device=DEV))
    return DataLoader(data, batch_size=len(x))


def test_single_chain_sampler_on_torch_draws_reproduces_group_a():
    from eeyore_amd.samplers import AM, Ridge
    rec = _g13()["a"]
    n_it = rec["z"].shape[0]
    s = AM(_lr_model(torch.float64), theta0=torch.tensor(rec["theta0"], device=DEV),
           dataloader=_loader(rec["x"], rec["y"], torch.float64), l=float(rec["l"]), b=float(rec["b"]),
           c=float(rec["c"]), t0=int(rec["t0"]), transform=Ridge(float(rec["eps"])))
    assert s.rng == 'torch' and s.cov.shape == (5, 5) and s.running_mean.shape == (5,)
    assert abs(float(s.current['target_val']) - float(rec["init_target"])) <= 1e-9 * abs(float(rec["init_target"]))
    with _Replay(rec) as rp:
        s.run(num_epochs=n_it, num_burnin_epochs=0)
    assert rp.pos == len(rp.items)  # every recorded draw was consumed: two uniforms past t0, one before
    got = torch.stack(list(s.get_chain().vals['sample'])).cpu().numpy()
    np.testing.assert_allclose(got, rec["sample"], rtol=1e-8, atol=1e-9)
    assert [int(a) for a in s.get_chain().vals['accepted']] == rec["accepted"].tolist()
    assert s.num_accepted == int(rec["num_accepted"][-1]) and s.breakdowns == 0
    want = rec["cov"][-1]
    assert np.linalg.norm(np.tril(s.cov.cpu().numpy()) - want) <= 1e-8 * np.linalg.norm(want)
    assert torch.equal(s.cov, s.cov.T) and torch.equal(s.cov_sum, s.cov_sum.T)


def _start(pl, C, dtype, seed=0, scale=0.1, cov_scale=0.01):
    g = torch.Generator(device="cpu").manual_seed(seed)
    th = (scale * torch.randn(C, pl.P, generator=g, dtype=torch.float64)).to(device=DEV, dtype=dtype)
    lik, prior = pl.log_target(th)
    P = pl.P
    c0 = (cov_scale * torch.eye(P, dtype=dtype, device=DEV)).contiguous()
    return dict(theta=th, target=(lik + prior).contiguous(), mean=torch.zeros(C, P, dtype=dtype, device=DEV),
                cov_sum=torch.zeros(C, P, P, dtype=dtype, device=DEV), cov=c0.expand(C, P, P).contiguous(),
                nacc=torch.zeros(C, dtype=torch.int32, device=DEV), cov0=c0,
                bd=torch.zeros(C, dtype=torch.int32, device=DEV))


def _args(st):
    return st["theta"], st["target"], st["mean"], st["cov_sum"], st["cov"], st["nacc"], st["cov0"]


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _same(a, b, keys=("theta", "target", "mean", "cov_sum", "cov", "nacc", "bd")):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("name", ["lr5", "mlp2321", "lr65"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("how", ["t0 beyond the run", "l = 1"])
def test_isotropic_cases_are_k_mh_bit_for_bit(name, dtype, how):
    from eeyore_amd import _lib as L
    pl, _ = _case_plan(name, dtype)
    C, P, K, c = 65, pl.P, 12, 0.07
    par = dict(l=0.05, t0=10 ** 6, c=c) if how.startswith("t0") else dict(l=1.0, t0=2, c=c)
    scale = torch.full((P,), c, dtype=dtype)
    a = _start(pl, C, dtype, seed=4)
    th_b, tv_b = a["theta"].clone(), a["target"].clone()
    rec = [(torch.empty(K, C, P, dtype=dtype, device=DEV), torch.empty(K, C, dtype=dtype, device=DEV),
            torch.empty(K, C, dtype=torch.uint8, device=DEV)) for _ in range(2)]
    pl.am_run(*_args(a), 0, K, seed=12, it=3, breakdowns=a["bd"], samples=rec[0][0], targets=rec[0][1],
              accepted_rec=rec[0][2], **par)
    pl.mh_run(th_b, tv_b, scale, K, seed=12, it=3, flags=L.EY_FORCE_GENERIC, samples=rec[1][0], targets=rec[1][1],
              accepted_rec=rec[1][2])
    assert all(torch.equal(x, y) for x, y in zip(*rec))
    assert torch.equal(a["theta"], th_b) and torch.equal(a["target"], tv_b)
    assert 0 < int(rec[0][2].sum()) < K * C and int(a["bd"].sum()) == 0
    # recorded draws, continuing from the state the run left (idx = K: past t0 = 2 in the l = 1 case)
    rng = np.random.default_rng(3)
    for it in range(3):
        z, u = _t(rng.standard_normal((C, P)), dtype), _t(rng.random(C), dtype)
        oa = pl.am_step(*_args(a), K + it, z=z, u_mix=_t(rng.random(C), dtype), u=u, breakdowns=a["bd"], **par)
        ob = pl.mh_step(th_b, tv_b, scale, z=z, u=u, flags=L.EY_FORCE_GENERIC)
        assert torch.equal(oa["accepted"], ob["accepted"]) and torch.equal(oa["log_rate"], ob["log_rate"])
        assert torch.equal(a["theta"], th_b) and torch.equal(a["target"], tv_b) and (oa["branch"] == 0).all()


PAR = dict(l=0.3, b=0.8, c=0.05, t0=5)


@pytest.mark.parametrize("name,dtype", [("mlp433", torch.float32), ("lr5", torch.float64), ("mlp6142", torch.float32),
                                        ("lr65", torch.float64)])
def test_run_equals_steps_bit_for_bit(name, dtype):
    pl, _ = _case_plan(name, dtype)
    C, P = 33, pl.P
    eps = 1e-3 if dtype == torch.float32 else 1e-6
    a = _start(pl, C, dtype, scale=0.05, cov_scale=0.0025)
    b = _clone(a)
    chunks = (2, 3, 4, 5)  # launches end at n = 2 (before t0 = 5), n = 5 (at t0) and n = 9 (after): the state written
    K = sum(chunks)        # back and read again crosses every regime
    rs = torch.empty(K, C, P, dtype=dtype, device=DEV)
    rt = torch.empty(K, C, dtype=dtype, device=DEV)
    ra = torch.empty(K, C, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(C, dtype=torch.int32, device=DEV)
    k0 = 0
    for k in chunks:
        pl.am_run(*_args(a), k0, k, eps=eps, seed=9, it=11 + k0, breakdowns=a["bd"], samples=rs[k0:k0 + k],
                  targets=rt[k0:k0 + k], accepted_rec=ra[k0:k0 + k], accept_count=cnt, **PAR)
        k0 += k
    branches = []
    for k in range(K):
        out = pl.am_step(*_args(b), k, eps=eps, seed=9, it=11 + k, breakdowns=b["bd"], **PAR)
        branches.append(out["branch"].clone())
        assert torch.equal(rs[k], b["theta"]) and torch.equal(rt[k], b["target"]), k
        assert torch.equal(ra[k], out["accepted"]), k
    assert _same(a, b)
    assert torch.equal(cnt, ra.int().sum(0)) and 0 < int(cnt.sum()) < C * K
    assert torch.equal(a["nacc"], ra[1:].int().sum(0).int())  # the accept of idx = 0 is not counted
    br = torch.stack(branches)
    assert (br[:PAR["t0"]] == 0).all() and (br[PAR["t0"]:] == 1).any() and (br[PAR["t0"]:] == 0).any()
    assert int(a["bd"].sum()) == 0 and (br != 2).all()


def _lr_sampler(C, dtype, fused_block, stats=False, epochs=40, burnin=10, N=200, transform="ridge", seed=4, **kw):
    from eeyore_amd.distributed import ChainStats
    from eeyore_amd.samplers import AM, Ridge
    x, y = _data([4, 1], 0, N, seed=5)
    loader = _loader(x, y, dtype)
    model = _lr_model(dtype)
    g = torch.Generator(device="cpu").manual_seed(1)
    th0 = (0.1 * torch.randn(C, 5, generator=g, dtype=torch.float64)).to(device=DEV, dtype=dtype)
    eps = 1e-4
    if transform == "ridge":
        transform = Ridge(eps)
    elif transform == "callable":
        eye = torch.eye(5, dtype=dtype, device=DEV)
        transform = lambda cov: cov + eps * eye  # noqa: E731
    par = dict(l=0.1, b=2.38 / np.sqrt(5), c=0.1, t0=5)
    par.update(kw)
    s = AM(model, theta0=th0, dataloader=loader, seed=seed, transform=transform, **par)
    s.fused_block = fused_block
    st = None
    if stats:
        st = ChainStats(C, 5, DEV)
        st.attach(model._plan(*next(iter(loader))))
    s.run(num_epochs=epochs, num_burnin_epochs=burnin)
    if stats:
        model._plan(*next(iter(loader))).detach_moments()
    return s, st


@pytest.mark.parametrize("stats", [False, True])
def test_sampler_run_in_blocks_equals_draws(stats):
    a, sa = _lr_sampler(32, torch.float32, 256, stats)
    b, sb = _lr_sampler(32, torch.float32, 0, stats)
    assert a._can_fuse(False) and not b._can_fuse(False)
    for key in ("cov", "cov_sum", "running_mean", "num_accepted", "breakdowns", "_theta"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    ca, cb = a.get_chain(), b.get_chain()
    assert torch.equal(ca.get_samples(), cb.get_samples()) and torch.equal(ca.get_target_vals(), cb.get_target_vals())
    assert ca.get_samples().shape[0] == 30 and int(a.num_accepted.sum()) > 0
    if stats:
        torch.testing.assert_close(sa.s1, sb.s1, rtol=1e-12, atol=0)
        torch.testing.assert_close(sa.s2, sb.s2, rtol=1e-12, atol=0)
        assert torch.equal(sa.acc, sb.acc) and sa.n == sb.n == 40


def test_whole_run_covariance_identity():
    """f64, 200 Philox draws recorded from the first: cov is the sample covariance of the recorded states plus eps I,
    running_mean their mean (am.py:57-59 is the textbook estimator written with sums)."""
    s, _ = _lr_sampler(16, torch.float64, 256, epochs=200, burnin=0)
    states = s.get_chain().get_samples()  # [200, C, P]
    assert states.shape == (200, 16, 5)
    moved = (s.num_accepted > 0).nonzero().flatten().tolist()
    assert len(moved) >= 12
    eye = torch.eye(5, dtype=torch.float64, device=DEV)
    for ch in moved:
        want = torch.cov(states[:, ch].T) + 1e-4 * eye
        assert (s.cov[ch] - want).abs().max() <= 1e-9 * want.abs().max(), ch
        torch.testing.assert_close(s.running_mean[ch], states[:, ch].mean(0), rtol=1e-9, atol=1e-12)
    assert int(s.breakdowns.sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_deterministic_breakdown(dtype):
    pl, _ = _case_plan("lr5", dtype)
    C, P, c = 5, pl.P, 0.05
    st = _start(pl, C, dtype, seed=6)
    bad = torch.diag(torch.tensor([1.0, -1.0, 1.0, 1.0, 1.0], dtype=dtype, device=DEV))
    st["cov"][1] = bad
    st["cov"][3] = torch.eye(P, dtype=dtype, device=DEV)
    st["cov"][3][2, 0] = float("nan")
    st["nacc"].fill_(1)
    th0 = st["theta"].clone()
    rng = np.random.default_rng(0)
    z = _t(rng.standard_normal((C, P)), dtype)
    out = pl.am_step(*_args(st), 20, l=0.25, b=1.0, c=c, t0=4, z=z, u_mix=_t(np.full(C, 0.9), dtype),
                     u=_t(np.full(C, 1e-30), dtype), breakdowns=st["bd"])
    assert out["branch"].tolist() == [1, 2, 1, 2, 1] and st["bd"].tolist() == [0, 1, 0, 1, 0]
    assert out["accepted"].tolist() == [1] * C
    for ch in (1, 3):  # the proposal was theta + c z
        want = th0[ch] + torch.tensor(c, dtype=dtype, device=DEV) * z[ch]
        torch.testing.assert_close(st["theta"][ch], want, rtol=1e-15 if dtype == torch.float64 else 1e-6, atol=0)
    assert torch.isfinite(torch.tril(st["cov"])).all()  # the adaptation rebuilt the covariance


def test_on_breakdown_raises_or_continues():
    for mode in ("raise", "isotropic"):
        s, _ = _lr_sampler(6, torch.float64, 0, epochs=10, burnin=0, l=0.0, on_breakdown=mode)
        assert int(s.breakdowns.sum()) == 0
        cov = s.cov.clone()
        cov[2] = torch.diag(torch.tensor([1.0, -1.0, 1.0, 1.0, 1.0], dtype=torch.float64, device=DEV))
        cov[4][0, 0] = float("nan")
        th = s._theta.clone()
        s.set_all(th, cov=cov)
        assert (s.running_mean == 0).all() and (s.cov_sum == 0).all()
        x, y = next(iter(s.dataloader))
        if mode == "raise":
            with pytest.raises(RuntimeError, match=r"chain\(s\) \[2, 4\]"):
                s.draw(x, y)
            s.draw(x, y)  # the adaptation repaired the covariance: the next draw factorises
        else:
            s.draw(x, y)
            s.draw(x, y)
        assert s.breakdowns.tolist() == [0, 0, 1, 0, 1, 0]
    s.reset(th)
    assert int(s.num_accepted.sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_callable_transform_equals_ridge_bit_for_bit(dtype):
    a, _ = _lr_sampler(8, dtype, 256, epochs=30, burnin=0, transform="ridge")
    b, _ = _lr_sampler(8, dtype, 256, epochs=30, burnin=0, transform="callable")
    assert a._can_fuse(False) and not b._can_fuse(False)
    assert torch.equal(a.get_chain().get_samples(), b.get_chain().get_samples())
    for key in ("cov", "cov_sum", "running_mean", "num_accepted"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert int(a.num_accepted.sum()) > 0


def test_chain_independence():
    pl, _ = _case_plan("mlp433", torch.float32)
    full = _start(pl, 1024, torch.float32, seed=2)
    par = dict(eps=1e-3, seed=5, **PAR)
    pick = 777
    one = {k: (v[pick:pick + 1].clone() if k != "cov0" else v) for k, v in full.items()}
    halves = [{k: (v[:512].clone() if k != "cov0" else v) for k, v in full.items()},
              {k: (v[512:].clone() if k != "cov0" else v) for k, v in full.items()}]
    pl.am_run(*_args(full), 0, 20, breakdowns=full["bd"], **par)
    pl.am_run(*_args(one), 0, 20, breakdowns=one["bd"], chain_offset=pick, **par)
    pl.am_run(*_args(halves[0]), 0, 20, breakdowns=halves[0]["bd"], **par)
    pl.am_run(*_args(halves[1]), 0, 20, breakdowns=halves[1]["bd"], chain_offset=512, **par)
    for k in ("theta", "target", "mean", "cov_sum", "cov", "nacc", "bd"):
        assert torch.equal(full[k][pick:pick + 1], one[k]), k
        assert torch.equal(full[k], torch.cat([halves[0][k], halves[1][k]])), k
    assert int(full["nacc"].sum()) > 0


def _padded(shape, dtype, fill, pad=64):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n].view(*shape)


def _am_lds_bytes(dims, esz):
    """The kernel's LDS of one chain (ey_generic_am_lds): the MH image, two packed triangles, mean, z, a slot per lane."""
    P = sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1))
    ppad = (P + 3) & ~3
    packed = (P * (P + 1) // 2 + 3) & ~3
    return esz * (2 * ppad + sum(dims) * 65 + 2 * max(dims) * 65 + 2 * packed + 2 * ppad + 64)


def test_buffer_safety():
    dims, acts, lik, N = CASES["mlp433"]
    x, y = _data(dims, lik, N)
    for dtype in (torch.float64, torch.float32):
        pl = _plan(dims, acts, lik, x, y, dtype)
        C, P, K = 5, pl.P, 9
        st = _start(pl, C, dtype)
        g = torch.Generator(device="cpu").manual_seed(0)
        src = dict(th=st["theta"], tv=st["target"], mean=st["mean"], cs=st["cov_sum"], cov=st["cov"],
                   c0=st["cov"].clone(), z=torch.randn(C, P, generator=g).to(DEV, dtype),
                   um=torch.rand(C, generator=g).to(DEV, dtype), u=torch.rand(C, generator=g).to(DEV, dtype))
        specs = [("th", (C, P), dtype), ("tv", (C,), dtype), ("mean", (C, P), dtype), ("cs", (C, P, P), dtype),
                 ("cov", (C, P, P), dtype), ("c0", (C, P, P), dtype), ("z", (C, P), dtype), ("um", (C,), dtype),
                 ("u", (C,), dtype), ("nacc", (C,), torch.int32), ("bd", (C,), torch.int32), ("acc", (C,), torch.uint8),
                 ("br", (C,), torch.uint8), ("lr", (C,), dtype), ("rs", (K, C, P), dtype), ("rt", (K, C), dtype),
                 ("ra", (K, C), torch.uint8), ("cnt", (C,), torch.int32)]
        bufs = {}
        for key, shape, dt in specs:
            buf, view = _padded(shape, dt, 77 if dt in (torch.uint8, torch.int32) else -12345.0)
            if key in src:
                view.copy_(src[key])
            if key in ("cnt", "nacc", "bd"):
                view.zero_()
            bufs[key] = (buf, view)
        v = {k: b[1] for k, b in bufs.items()}
        upper = torch.triu(torch.ones(P, P, dtype=torch.bool, device=DEV), 1).expand(C, P, P)
        v["cov"][upper] = float("nan")
        v["cs"][upper] = float("nan")
        snap = {k: b.clone() for k, (b, _) in bufs.items()}
        par = dict(eps=1e-3, breakdowns=v["bd"], **PAR)
        pl.am_run(v["th"], v["tv"], v["mean"], v["cs"], v["cov"], v["nacc"], v["c0"], 0, K, samples=v["rs"],
                  targets=v["rt"], accepted_rec=v["ra"], accept_count=v["cnt"], out=dict(accepted=v["acc"]), **par)
        pl.am_step(v["th"], v["tv"], v["mean"], v["cs"], v["cov"], v["nacc"], v["c0"], K, z=v["z"], u_mix=v["um"],
                   u=v["u"], out=dict(accepted=v["acc"], log_rate=v["lr"], branch=v["br"]), **par)
        torch.cuda.synchronize()
        for k, (b, _) in bufs.items():
            assert torch.equal(b[:64], snap[k][:64]) and torch.equal(b[-64:], snap[k][-64:]), k
        for k in ("c0", "z", "um", "u"):  # read-only inputs keep their bits
            assert torch.equal(bufs[k][0], snap[k]), k
        for k in ("cov", "cs"):
            assert torch.isnan(v[k][upper]).all() and torch.isfinite(v[k][~upper]).all(), k
        assert torch.isfinite(v["rs"]).all() and (v["br"] <= 1).all() and (v["bd"] == 0).all()
        assert 0 < int(v["cnt"].sum()) and torch.isfinite(v["lr"]).all()


def test_lds_limit():
    limit = 160 * 1024
    assert _am_lds_bytes([73, 1], 8) <= limit < _am_lds_bytes([74, 1], 8)
    assert _am_lds_bytes([6, 14, 2], 8) <= limit  # P = 128 in f64 fits
    for d0, dtype, ok in ((74, torch.float64, False), (73, torch.float64, True), (128, torch.float32, False)):
        x, y = _data([d0, 1], 0, 16)
        pl = _plan([d0, 1], [1], 0, x, y, dtype)
        st = _start(pl, 3, dtype)
        before = _clone(st)
        acc = torch.full((3,), 9, dtype=torch.uint8, device=DEV)
        if ok:
            pl.am_run(*_args(st), 0, 8, breakdowns=st["bd"], eps=1e-6, out=dict(accepted=acc), **PAR)
            torch.cuda.synchronize()
            assert (acc <= 1).all() and torch.isfinite(torch.tril(st["cov"])).all() and int(st["bd"].sum()) == 0
            continue
        with pytest.raises(RuntimeError, match="status -2"):
            pl.am_step(*_args(st), 0, breakdowns=st["bd"], out=dict(accepted=acc), **PAR)
        torch.cuda.synchronize()
        assert (acc == 9).all() and _same(st, before)


def test_invalid_arguments_return_before_any_launch():
    pl, _ = _case_plan("lr5", torch.float64)
    st = _start(pl, 2, torch.float64)
    before = _clone(st)
    for kw in (dict(t0=1), dict(l=1.5), dict(l=-0.1), dict(b=float("inf")), dict(c=float("nan")), dict(eps=-1e-9),
               dict(eps=float("inf")), dict(offset=3)):
        with pytest.raises(ValueError):
            pl.am_step(*_args(st), 0, breakdowns=st["bd"], **kw)
    with pytest.raises(ValueError):
        pl.am_run(*_args(st), 0, 0, breakdowns=st["bd"])
    torch.cuda.synchronize()
    assert _same(st, before)


def test_example_runs():
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="60", EEYORE_EXAMPLE_CHAINS="16", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "am_logistic_regression.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "cceptance rate" in out.stdout and "sample covariance" in out.stdout
