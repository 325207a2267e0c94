"""softabs on the device: ``ey_softabs`` against the eigh form, AM with the fused transform (ey_am_softabs_step /
ey_am_softabs_run, k_am's softabs instantiation in eeyore_amd/csrc/ey_generic.hip) against the numpy restatement
(tests/softabs_restatement.py), the reference's traces (g22_am_softabs_traces.npz) and itself."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import load
from tests.softabs_cases import (FACTOR, LIMIT, ONE_STEP, ONE_STEP_MODELS, largest_lr, matrices, one_step_inputs,
                                 one_step_model, softabs_lds_bytes, yardstick)
from tests.softabs_restatement import MAX_SWEEPS, am_draw_softabs, recorded_state, softabs_jacobi, softabs_ref
from tests.test_am_gpu import (CASES, DEV, F32_DECISION_TOL, LMIX, PAR, ROOT, _args, _clone, _data, _i32, _lower,
                               _lr_sampler, _np, _padded, _plan, _same, _start, _t, _target_fn)

pytestmark = pytest.mark.gpu

A = 1000.0


def _model_plan(name, dtype):
    dims, acts, lik, N = one_step_model(name, dtype == torch.float64)
    x, y = _data(dims, lik, N)
    return _plan(dims, acts, lik, x, y, dtype), (dims, acts, lik, x, y)


# ----------------------------------------------------------------------------------------------------------- ey_softabs
@functools.lru_cache(maxsize=None)
def _cases(P, f32):
    """[(name, the matrix as the device holds it, its eigh-form softabs, its yardstick)], computed once."""
    out = []
    for name, M in matrices(P).items():
        if f32:
            M = M.astype(np.float32).astype(np.float64)
            M = np.tril(M) + np.tril(M, -1).T
        out.append((name, M, softabs_ref(M, A), yardstick(M, A)))
    return out


@pytest.mark.parametrize("P", [1, 2, 3, 5, 27, 64, 65, 128])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ey_softabs_against_eigh(P, dtype):
    from eeyore_amd.stats import batched
    f32 = dtype == torch.float32
    cases = _cases(P, f32)
    for B in (1, 3, 65):
        pick = [cases[(k + B) % len(cases)] for k in range(B)]
        mats = _t(np.stack([np.tril(c[1]) for c in pick]), dtype)
        mats += torch.triu(torch.full((P, P), float("nan"), dtype=dtype, device=DEV), 1)  # the upper triangle is not read
        sweeps = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        got = batched.softabs(mats, A, sweeps=sweeps)
        assert got.shape == mats.shape and got.dtype == dtype and torch.equal(got, got.mT)
        S = _np(got)
        for k, (name, M, ref, unit) in enumerate(pick):
            err = np.linalg.norm(S[k] - ref)
            bound = FACTOR * unit + (2.0 ** -24 * np.linalg.norm(S[k]) if f32 else 0.0)  # f32: rounded once
            print(f"P={P} B={B} {name}: sweeps {int(sweeps[k])} error / bound {err / bound:.3f}")
            assert err <= bound, (B, k, name, err, bound)
            assert (0 if P == 1 else 1) <= int(sweeps[k]) < MAX_SWEEPS, (name, int(sweeps[k]))
    one = batched.softabs(mats[0], A)  # [P, P]: the same function
    assert one.shape == (P, P) and torch.equal(one, got[0])
    if P <= 27 and not f32:  # the restatement restates: the same sweeps, the same numbers to a few roundings (tanh is libm's)
        for k, (name, M, ref, unit) in enumerate(pick[:6]):
            want, sw = softabs_jacobi(M, A)
            assert int(sweeps[k]) == sw, name
            np.testing.assert_allclose(S[k], want, rtol=1e-13, atol=1e-13 * np.abs(want).max())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ey_softabs_leaves_a_non_finite_matrix_and_serves_its_neighbours(dtype):
    from eeyore_amd.stats import batched
    P = 5
    cases = _cases(P, dtype == torch.float32)
    mats = _t(np.stack([cases[0][1], cases[5][1], cases[4][1]]), dtype)
    mats[1][3, 1] = float("nan")
    mats[1][1, 3] = 7.0  # the upper triangle is not read: the mirrored lower triangle comes back
    sweeps = torch.zeros(3, dtype=torch.int32, device=DEV)
    got = batched.softabs(mats, A, sweeps=sweeps)
    lo = torch.tril(mats[1])
    want = lo + torch.tril(mats[1], -1).mT
    assert torch.equal(torch.nan_to_num(got[1], nan=-99.0), torch.nan_to_num(want, nan=-99.0)) and int(sweeps[1]) == -1
    for k, c in ((0, cases[0]), (2, cases[4])):
        bound = FACTOR * c[3] + 2.0 ** -24 * np.linalg.norm(c[2]) * (dtype == torch.float32)
        assert np.linalg.norm(_np(got[k]) - c[2]) <= bound and int(sweeps[k]) >= 1
    inf = mats.clone()
    inf[1][3, 1] = float("-inf")
    assert int(batched.softabs(inf, A)[1][3, 1] == float("-inf")) == 1
    with pytest.raises(RuntimeError, match="status -2"):
        batched.softabs(torch.zeros(129, 129, dtype=dtype, device=DEV))
    with pytest.raises(ValueError):
        batched.softabs(mats, 0.0)


@pytest.mark.parametrize("P", [2, 5])
def test_sweeps_stay_below_the_cap_on_many_matrices(P):
    """4096 covariances of three states, and their transforms once more (eigenvalue 1 / a repeated P - 2 times, or a pair
    that rounding alone separates): every one converges, none runs into the cap.  (With the pair test at 2^-52, below what
    rounding leaves of an inner product, about one f64 matrix in 4096 rotated until the cap.)"""
    from eeyore_amd.stats import batched
    rng = np.random.default_rng(P)
    states = 0.1 * rng.standard_normal((4096, 3, P))
    d = states - states.mean(1, keepdims=True)
    mats = _t(np.einsum("bki,bkj->bij", d, d) / 2, torch.float64)
    sweeps = torch.zeros(4096, dtype=torch.int32, device=DEV)
    once = batched.softabs(mats, A, sweeps=sweeps)
    assert 1 <= int(sweeps.min()) and int(sweeps.max()) < MAX_SWEEPS // 2
    twice = batched.softabs(once, A, sweeps=sweeps)
    assert 1 <= int(sweeps.min()) and int(sweeps.max()) < MAX_SWEEPS // 2
    lam = torch.linalg.eigvalsh(twice)
    assert float(lam.min()) > 0.99 / A and torch.isfinite(twice).all()


# ---------------------------------------------------------------------------------- one step against am_draw_softabs
@pytest.mark.parametrize("name", ONE_STEP_MODELS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("C", [1, 3, 65])
def test_one_step_against_the_restatement(name, dtype, C):
    pl, (dims, acts, lik, x, y) = _model_plan(name, dtype)
    assert pl.am_softabs_fits()
    tf = _target_fn(dims, acts, lik, x, y)
    P = pl.P
    f64 = dtype == torch.float64
    b, c = 2.38 / np.sqrt(P), 0.05
    transformed = factored = skipped = 0
    for si, (label, idx, offset, t0, nacc0, mix, force) in enumerate(ONE_STEP):
        n = idx + 1 - offset
        inp = one_step_inputs(P, C, si)
        dev = {k: _t(v, dtype) for k, v in inp.items()}
        nacc, bd = _i32(np.full(C, nacc0)), _i32(np.zeros(C))
        h = {k: _np(v) for k, v in dev.items()}  # the restatement starts from the values the device holds (f32: rounded)
        th, mean, cs, cov = (dev[k].clone() for k in ("th", "mean", "cs", "cov"))
        tv = pl.log_target(th)
        tv = (tv[0] + tv[1]).contiguous()
        tv0 = _np(tv)
        out = pl.am_step(th, tv, mean, cs, cov, nacc, dev["cov0"], idx, l=LMIX, b=b, c=c, t0=t0, offset=offset,
                         z=dev["z"], u_mix=dev["um"], u=dev["u"], breakdowns=bd, softabs_a=A)
        acc, br, lr_dev = out["accepted"].cpu().numpy(), out["branch"].cpu().numpy(), _np(out["log_rate"])
        th1, tv1, mean1, cs1, cov1 = (_np(v) for v in (th, tv, mean, cs, cov))
        assert (bd == 0).all(), label
        for ch in range(C):
            want = am_draw_softabs(tf, h["th"][ch], float(tv0[ch]), h["mean"][ch], h["cs"][ch], h["cov"][ch], nacc0,
                                   h["cov0"][ch], h["z"][ch], h["um"][ch], h["u"][ch], idx, offset, LMIX, b, c, t0, A,
                                   transform=softabs_ref)
            assert br[ch] == want["branch"], (label, ch)
            factored += int(br[ch] == 1)
            lr_ref = want["log_rate"]
            np.testing.assert_allclose(lr_dev[ch], lr_ref, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
            tol = 1e-9 if f64 else F32_DECISION_TOL * max(1.0, abs(lr_ref))
            if not abs(np.log(h["u"][ch]) - lr_ref) > tol:
                skipped += 1
                continue
            assert bool(acc[ch]) == want["accepted"], (label, ch, lr_ref, np.log(h["u"][ch]))
            assert int(nacc[ch]) == want["num_accepted"], (label, ch)
            kw = dict(rtol=1e-12, atol=1e-12) if f64 else dict(rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(th1[ch], want["theta"], **kw)
            np.testing.assert_allclose(tv1[ch], want["target"], rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3)
            np.testing.assert_allclose(mean1[ch], want["mean"], **kw)
            big = max(np.abs(want["cov_sum"]).max(), 1e-30)
            np.testing.assert_allclose(_lower(cs1[ch]), _lower(want["cov_sum"]), rtol=0, atol=(1e-14 if f64 else 1e-6) * big)
            if not want["transformed"]:
                src = h["cov0"][ch] if n >= t0 else h["cov"][ch]  # cov0' as it is, or nothing rebuilt
                assert (np.tril(cov1[ch]) == np.tril(src)).all(), label
                continue
            transformed += 1
            # the raw covariance as tests/test_am_gpu.py bounds it (four roundings of entries of the size of cov_sum),
            # through the Lipschitz-1 transform, then the yardstick; f32 adds the one rounding of the result
            raw_err = P * (1e-14 if f64 else 1e-6) * big + (1e-12 if f64 else 1e-5) * np.linalg.norm(want["raw_cov"])
            got = np.tril(cov1[ch]) + np.tril(cov1[ch], -1).T
            bound = FACTOR * yardstick(want["raw_cov"], A) + raw_err + (0.0 if f64 else 2.0 ** -24 * np.linalg.norm(got))
            assert np.linalg.norm(got - want["cov"]) <= bound, (label, ch)
            assert np.linalg.eigvalsh(got).min() > 0.5 / A, (label, ch)  # positive definite, rank deficient or not
    assert skipped == 0
    assert transformed >= 3 * max(1, C - 3) and factored >= 2 * ((C + 1) // 2)


# --------------------------------------------------------------------------------------------------------- the fixture
def _g22():
    z = load("g22_am_softabs_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in "abc"}


def _fixture_plan(rec):
    f64 = torch.float64
    if "weights" in rec:
        from eeyore_amd.models import DistributionModel, NormalMixture
        from eeyore_amd.datasets import EmptyXYDataset
        target = NormalMixture(rec["weights"].tolist(), torch.tensor(rec["means"]), torch.tensor(rec["covs"]),
                               normalized=bool(rec["normalized"]))
        model = DistributionModel(target, rec["means"].shape[1], dtype=f64, device=DEV)
        return model._plan(*next(iter(torch.utils.data.DataLoader(EmptyXYDataset()))))
    return _plan(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], f64)


@pytest.mark.parametrize("name", list("abc"))
def test_fixture_replay(name):
    """Every recorded draw through ey_am_softabs_step from the recorded state before it, f64: the bounds of
    tests/test_softabs_host.py::test_fixture_replay."""
    rec = _g22()[name]
    f64 = torch.float64
    pl = _fixture_plan(rec)
    P = pl.P
    c0 = _t(rec["cov0"], f64)
    par = dict(l=float(rec["l"]), b=float(rec["b"]), c=float(rec["c"]), t0=int(rec["t0"]), offset=int(rec["offset"]),
               softabs_a=float(rec["a"]))
    bd = _i32([0])
    transformed = factored = 0
    for it in range(rec["z"].shape[0]):
        st, want = recorded_state(rec, it - 1), recorded_state(rec, it)
        th, tv = _t(st["theta"], f64)[None].clone(), _t([st["target"]], f64)
        mean, cs, cov = _t(st["mean"], f64)[None].clone(), _t(st["cov_sum"], f64)[None].clone(), _t(st["cov"], f64)[None].clone()
        nacc = _i32([st["num_accepted"]])
        out = pl.am_step(th, tv, mean, cs, cov, nacc, c0, int(rec["idx"][it]), z=_t(rec["z"][it], f64)[None],
                         u_mix=_t([rec["u_mix"][it]], f64), u=_t([rec["u"][it]], f64), breakdowns=bd, **par)
        assert abs(np.log(float(rec["u"][it])) - out["log_rate"].item()) >= 1e-6, it
        assert int(out["accepted"].item()) == int(rec["accepted"][it]), it
        factored += int(out["branch"].item() == 1)
        np.testing.assert_allclose(_np(th[0]), want["theta"], rtol=1e-10, atol=1e-10 * np.abs(want["theta"]).max())
        np.testing.assert_allclose(tv.item(), want["target"], rtol=1e-9)
        assert int(nacc.item()) == want["num_accepted"]
        np.testing.assert_allclose(_np(mean[0]), want["mean"], rtol=1e-12, atol=1e-14)
        got = np.tril(_np(cov[0])) + np.tril(_np(cov[0]), -1).T
        n = int(rec["n"][it])
        if not (n >= par["t0"] and want["num_accepted"] > 0):
            assert np.array_equal(got, want["cov"]), it
            continue
        transformed += 1
        m, csum = want["mean"], want["cov_sum"]
        raw = (csum - n * np.outer(m, m)) / (n - 1)
        carried = 8 * 2.0 ** -52 * (np.linalg.norm(csum) + n * m @ m) / (n - 1)
        assert np.linalg.norm(got - want["cov"]) <= FACTOR * yardstick(raw, A) + carried, it
    assert int(bd.item()) == 0 and transformed >= rec["z"].shape[0] // 2 and factored >= 3


# ------------------------------------------------------------------------------------------------- against itself
@pytest.mark.parametrize("name,dtype", [("mlp433", torch.float32), ("lr5", torch.float64), ("lr65", torch.float32),
                                        ("lr65", torch.float64)])
def test_run_equals_steps_bit_for_bit(name, dtype):
    pl, _ = _model_plan(name, dtype)
    C, P = 33, pl.P
    a = _start(pl, C, dtype, scale=0.05, cov_scale=0.0025)
    b = _clone(a)
    chunks = (2, 3, 4, 5)  # launches end before t0 = 5, at it and after it, as in tests/test_am_gpu.py
    K = sum(chunks)
    rs = torch.empty(K, C, P, dtype=dtype, device=DEV)
    rt = torch.empty(K, C, dtype=dtype, device=DEV)
    ra = torch.empty(K, C, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(C, dtype=torch.int32, device=DEV)
    k0 = 0
    for k in chunks:
        pl.am_run(*_args(a), k0, k, softabs_a=A, seed=9, it=11 + k0, breakdowns=a["bd"], samples=rs[k0:k0 + k],
                  targets=rt[k0:k0 + k], accepted_rec=ra[k0:k0 + k], accept_count=cnt, **PAR)
        k0 += k
    branches = []
    for k in range(K):
        out = pl.am_step(*_args(b), k, softabs_a=A, seed=9, it=11 + k, breakdowns=b["bd"], **PAR)
        branches.append(out["branch"].clone())
        assert torch.equal(rs[k], b["theta"]) and torch.equal(rt[k], b["target"]), k
        assert torch.equal(ra[k], out["accepted"]), k
    assert _same(a, b)
    assert torch.equal(cnt, ra.int().sum(0)) and 0 < int(cnt.sum()) < C * K
    br = torch.stack(branches)
    assert (br[:PAR["t0"]] == 0).all() and (br[PAR["t0"]:] == 1).any() and (br != 2).all() and int(a["bd"].sum()) == 0
    # the covariance of every chain that moved was transformed: positive definite, no eigenvalue below 1 / a
    moved = (a["nacc"] > 0).nonzero().flatten().tolist()
    assert len(moved) >= C // 2
    lam = torch.linalg.eigvalsh(torch.tril(a["cov"][moved]).double(), UPLO="L")
    assert float(lam.min()) > 0.9 / A


def _softabs_sampler(C, dtype, fused_block, transform, **kw):
    return _lr_sampler(C, dtype, fused_block, transform=transform, **kw)[0]


def test_sampler_run_in_blocks_equals_draws():
    from eeyore_amd.samplers import SoftAbs
    a = _softabs_sampler(32, torch.float32, 256, SoftAbs(A))
    b = _softabs_sampler(32, torch.float32, 0, SoftAbs(A))
    assert a._can_fuse(False) and not b._can_fuse(False) and not a._generic and not b._generic
    for key in ("cov", "cov_sum", "running_mean", "num_accepted", "breakdowns", "_theta"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    ca, cb = a.get_chain(), b.get_chain()
    assert torch.equal(ca.get_samples(), cb.get_samples()) and torch.equal(ca.get_target_vals(), cb.get_target_vals())
    assert ca.get_samples().shape[0] == 30 and int(a.num_accepted.sum()) > 0 and int(a.breakdowns.sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fused_transform_equals_the_callable_path_bit_for_bit(dtype):
    from eeyore_amd.samplers import SoftAbs
    from eeyore_amd.stats import batched
    a = _softabs_sampler(8, dtype, 256, SoftAbs(A), epochs=30, burnin=0)
    b = _softabs_sampler(8, dtype, 256, lambda m: batched.softabs(m, A), epochs=30, burnin=0)
    assert a._can_fuse(False) and not b._can_fuse(False) and b._generic
    assert torch.equal(a.get_chain().get_samples(), b.get_chain().get_samples())
    for key in ("cov", "cov_sum", "running_mean", "num_accepted"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert int(a.num_accepted.sum()) > 0 and int(a.breakdowns.sum()) == 0


def test_chain_independence():
    pl, _ = _model_plan("mlp433", torch.float32)
    full = _start(pl, 256, torch.float32, seed=2)
    par = dict(softabs_a=A, seed=5, **PAR)
    pick = 177
    one = {k: (v[pick:pick + 1].clone() if k != "cov0" else v) for k, v in full.items()}
    halves = [{k: (v[:128].clone() if k != "cov0" else v) for k, v in full.items()},
              {k: (v[128:].clone() if k != "cov0" else v) for k, v in full.items()}]
    pl.am_run(*_args(full), 0, 12, breakdowns=full["bd"], **par)
    pl.am_run(*_args(one), 0, 12, breakdowns=one["bd"], chain_offset=pick, **par)
    pl.am_run(*_args(halves[0]), 0, 12, breakdowns=halves[0]["bd"], **par)
    pl.am_run(*_args(halves[1]), 0, 12, breakdowns=halves[1]["bd"], chain_offset=128, **par)
    for k in ("theta", "target", "mean", "cov_sum", "cov", "nacc", "bd"):
        assert torch.equal(full[k][pick:pick + 1], one[k]), k
        assert torch.equal(full[k], torch.cat([halves[0][k], halves[1][k]])), k
    assert int(full["nacc"].sum()) > 0


# ------------------------------------------------------------------------------------------------------------ buffers
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
                 ("ra", (K, C), torch.uint8), ("cnt", (C,), torch.int32), ("sin", (C, P, P), dtype),
                 ("sout", (C, P, P), dtype), ("sw", (C,), torch.int32)]
        bufs = {}
        for key, shape, dt in specs:
            buf, view = _padded(shape, dt, 77 if dt in (torch.uint8, torch.int32) else -12345.0)
            if key in src:
                view.copy_(src[key])
            if key in ("cnt", "nacc", "bd"):
                view.zero_()
            bufs[key] = (buf, view)
        v = {k: b[1] for k, b in bufs.items()}
        v["sin"].copy_(st["cov"])
        upper = torch.triu(torch.ones(P, P, dtype=torch.bool, device=DEV), 1).expand(C, P, P)
        v["cov"][upper] = float("nan")
        v["cs"][upper] = float("nan")
        snap = {k: b.clone() for k, (b, _) in bufs.items()}
        par = dict(softabs_a=A, breakdowns=v["bd"], **PAR)
        pl.am_run(v["th"], v["tv"], v["mean"], v["cs"], v["cov"], v["nacc"], v["c0"], 0, K, samples=v["rs"],
                  targets=v["rt"], accepted_rec=v["ra"], accept_count=v["cnt"], out=dict(accepted=v["acc"]), **par)
        pl.am_step(v["th"], v["tv"], v["mean"], v["cs"], v["cov"], v["nacc"], v["c0"], K, z=v["z"], u_mix=v["um"],
                   u=v["u"], out=dict(accepted=v["acc"], log_rate=v["lr"], branch=v["br"]), **par)
        from eeyore_amd import _lib as L
        L.check(L.lib().ey_softabs(L.ptr(v["sin"]), C, P, L.EY_F32 if dtype == torch.float32 else L.EY_F64, A,
                                   L.ptr(v["sout"]), L.ptr(v["sw"]), None), "ey_softabs")
        torch.cuda.synchronize()
        for k, (b, _) in bufs.items():
            assert torch.equal(b[:64], snap[k][:64]) and torch.equal(b[-64:], snap[k][-64:]), k
        for k in ("c0", "z", "um", "u", "sin"):  # read-only inputs keep their bits
            assert torch.equal(bufs[k][0], snap[k]), k
        for k in ("cov", "cs"):
            assert torch.isnan(v[k][upper]).all() and torch.isfinite(v[k][~upper]).all(), k
        assert torch.isfinite(v["rs"]).all() and (v["br"] <= 1).all() and (v["bd"] == 0).all()
        assert 0 < int(v["cnt"].sum()) and torch.isfinite(v["lr"]).all()
        assert torch.isfinite(v["sout"]).all() and (v["sw"] >= 1).all()


# ----------------------------------------------------------------------------------------------- limits and refusals
def test_lds_limit_and_fallback():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import logistic_regression as lr
    from eeyore_amd.samplers import AM, SoftAbs
    for dtype, esz in ((torch.float64, 8), (torch.float32, 4)):
        d = largest_lr(esz)
        assert softabs_lds_bytes([d, 1], esz) <= LIMIT < softabs_lds_bytes([d + 1, 1], esz) and d + 2 <= 128
        for d0, ok in ((d, True), (d + 1, False)):
            x, y = _data([d0, 1], 0, 16)
            pl = _plan([d0, 1], [1], 0, x, y, dtype)
            assert pl.am_softabs_fits() == ok
            if ok:
                continue  # the one-step test runs it
            st = _start(pl, 3, dtype)
            before = _clone(st)
            acc = torch.full((3,), 9, dtype=torch.uint8, device=DEV)
            with pytest.raises(RuntimeError, match="status -2"):
                pl.am_step(*_args(st), 0, breakdowns=st["bd"], out=dict(accepted=acc), softabs_a=A, **PAR)
            with pytest.raises(RuntimeError, match="status -2"):
                pl.am_run(*_args(st), 0, 4, breakdowns=st["bd"], out=dict(accepted=acc), softabs_a=A, **PAR)
            torch.cuda.synchronize()
            assert (acc == 9).all() and _same(st, before)
    # AM on the f32 model one past the limit (the kernel without the work matrix has room for it): the callable path with
    # the same object, said once
    d0 = largest_lr(4) + 1
    x, y = _data([d0, 1], 0, 16)
    model = lr.LogisticRegression(loss_functions['binary_classification'], hparams=lr.Hyperparameters(input_size=d0),
                                  dtype=torch.float32, device=DEV)
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import XYDataset
    loader = DataLoader(XYDataset(_t(x, torch.float32), _t(y, torch.float32)), batch_size=len(x))
    g = torch.Generator(device="cpu").manual_seed(1)
    th0 = (0.02 * torch.randn(4, d0 + 1, generator=g, dtype=torch.float64)).to(DEV, torch.float32)
    tr = SoftAbs(A)
    s = AM(model, theta0=th0, dataloader=loader, seed=3, transform=tr, l=0.1, b=2.38 / np.sqrt(d0 + 1), c=0.02, t0=3)
    with pytest.warns(RuntimeWarning, match="does not fit in LDS"):
        s.run(num_epochs=8, num_burnin_epochs=0)
    assert s._generic and s.transform is tr and int(s.breakdowns.sum()) == 0 and int(s.num_accepted.sum()) > 0
    moved = (s.num_accepted > 0).nonzero().flatten().tolist()
    assert float(torch.linalg.eigvalsh(s.cov[moved].double()).min()) > 0.9 / A  # the callable transformed what the kernel left
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.run(num_epochs=2, num_burnin_epochs=0)  # said once


def test_invalid_a_returns_before_any_launch():
    pl, _ = _model_plan("lr5", torch.float64)
    st = _start(pl, 2, torch.float64)
    before = _clone(st)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="a must be"):
            pl.am_step(*_args(st), 0, breakdowns=st["bd"], softabs_a=bad)
        with pytest.raises(ValueError, match="a must be"):
            pl.am_run(*_args(st), 0, 3, breakdowns=st["bd"], softabs_a=bad)
    for kw in (dict(t0=1), dict(l=1.5), dict(b=float("inf")), dict(offset=3)):
        with pytest.raises(ValueError):
            pl.am_step(*_args(st), 0, breakdowns=st["bd"], softabs_a=A, **kw)
    torch.cuda.synchronize()
    assert _same(st, before)


# --------------------------------------------------------------------------------------------------------- end to end
def test_example_runs():
    env = dict(os.environ, EEYORE_EXAMPLE_EPOCHS="110", EEYORE_EXAMPLE_CHAINS="16", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bivariate_normal_mixture_am.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "One chain" in out.stdout and "16 chains" in out.stdout and "Breakdowns of the factorisation: 0" in out.stdout


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mixture_chains_reach_both_modes_without_a_breakdown(dtype):
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.models import DistributionModel, NormalMixture
    from eeyore_amd.samplers import AM, SoftAbs
    means = torch.tensor([[-2., -2.], [2., 2.]])
    model = DistributionModel(NormalMixture([1., 1.], means, torch.eye(2).expand(2, 2, 2), normalized=False), 2,
                              dtype=dtype, device=DEV)
    s = AM(model, theta0=torch.zeros(256, 2, dtype=dtype, device=DEV), dataloader=DataLoader(EmptyXYDataset()), l=0.01,
           b=2., c=2., transform=SoftAbs(A), seed=1)
    assert s._can_fuse(False)
    s.run(num_epochs=1100, num_burnin_epochs=100)
    samples = s.get_chain().get_samples().double()  # [1000, 256, 2]
    pooled = samples.mean((0, 1))
    assert pooled.abs().max() < 0.5, pooled
    frac = (samples.sum(-1) < 0).double().mean()
    assert 0.3 < float(frac) < 0.7  # both modes, about evenly
    assert int(s.breakdowns.sum()) == 0  # the point of the transform
    assert float(torch.linalg.eigvalsh(s.cov).min()) > 0.9 / A
