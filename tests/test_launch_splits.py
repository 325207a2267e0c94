"""Host loops that split one call over several launches, block-index remaps that switch on at certain grid shapes, and
grid-stride loops behind a block cap: each against a plain reference at a shape that reaches the second launch, the
remapped grid or the second grid pass.

* ey_inse_multivariate's wide form sends the chains through a bounded workspace (EY_MV_WORKSPACE_MB, read at every call)
  in as many launches as that takes;
* the bf16x3 products of the layerwise path hand their workgroups to the XCDs by block rows (xcd_block_rows: the first
  layer's forward product on the pre-split data image) or block columns (xcd_block_cols: its weight gradient), when the
  grid has the shape for it;
* k_philox_normal / k_philox_uniform_blocks (65536 blocks), k_stats_update (4096) and k_stats_update_run (8192) stride
  over their elements when there are more than the capped grid covers.

(The chain-chunk loops of the layerwise path are in tests/test_chain_chunks.py, the base XCD map at block counts around
multiples of eight in tests/test_gpu_parity.py.)"""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import philox_oracle as po
from oracle.c_oracle import COracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _stream():
    return ct.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


# --------------------------------------------------------------------------- wide multivariate INSE: workspace chunks
MV_PAD = 2                 # canary chains on either side of every output
MV_CANARY, MV_CANARY_I = 777.25, 12345
# A chain's centred samples take n x 64 doubles of the workspace whatever p is; under a cap of 1 MiB:
#   n = 40   -> 20480 B per chain, 51 chains per launch: 120 chains run as 51 + 51 + 18; 35 chains are one launch (control;
#               n <= 2 p here, so the reference raises 'Not enough samples' for every chain: sig is NaN, pairs -1)
#   n = 100  -> 51200 B, 20 chains per launch: 45 chains run as 20 + 20 + 5, with real MC covariances in every launch
#   n = 5000 -> 2.56 MB: a chain does not fit the cap, one launch per chain
MV_CASES = [(20, 40, 120, 51), (64, 40, 35, 51), (17, 100, 45, 20), (5, 5000, 3, 1)]


def _mv_call(x, layout):
    """ey_inse_multivariate through the C ABI, the outputs in the middle of canary-filled buffers."""
    from eeyore_amd import _lib as L
    if layout == "ncp":
        n, C, p = x.shape
        sn, sc = C * p, p
    else:
        C, n, p = x.shape
        sn, sc = p, n * p
    kw = dict(dtype=torch.float64, device=DEV)
    bufs = dict(sig=torch.full((C + 2 * MV_PAD, p, p), MV_CANARY, **kw), cov=torch.full((C + 2 * MV_PAD, p, p), MV_CANARY, **kw),
                mean=torch.full((C + 2 * MV_PAD, p), MV_CANARY, **kw),
                pairs=torch.full((C + 2 * MV_PAD,), MV_CANARY_I, dtype=torch.int32, device=DEV))
    mid = {k: v[MV_PAD:MV_PAD + C] for k, v in bufs.items()}
    L.check(L.lib().ey_inse_multivariate(L.ptr(x), n, C, p, sn, sc, L.EY_F32 if x.dtype == torch.float32 else L.EY_F64,
                                         L.ptr(mid["sig"]), L.ptr(mid["cov"]), L.ptr(mid["mean"]), L.ptr(mid["pairs"]),
                                         _stream()), "ey_inse_multivariate")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        canary = MV_CANARY_I if k == "pairs" else MV_CANARY
        assert (v[:MV_PAD] == canary).all() and (v[MV_PAD + C:] == canary).all(), f"{k}: written outside its chains"
    return {k: v.clone() for k, v in mid.items()}


@pytest.mark.parametrize("p,n,C,per_launch", MV_CASES)
def test_multivariate_inse_workspace_chunks(p, n, C, per_launch, monkeypatch):
    """The wide form under a workspace cap of 1 MiB (several launches; per-launch pointers x + c0 stride_c, sig / cov +
    c0 p p, mean + c0 p, pairs + c0) against the per-chain port of the reference's estimator and st.cov at the tolerances
    of test_multivariate_inse_beyond_sixteen_parameters, both layouts, f64 and f32 storage, constant chains in the second
    and the last launch (where a launch holds more than one chain); and bit for bit the same call under the default cap
    (one launch: one workgroup per chain, so a chain's arithmetic cannot depend on its launch)."""
    import eeyore_amd.stats as st
    rng = np.random.default_rng(1000 * p + n)
    phi = rng.uniform(0.0, 0.9, size=(C, 1, p))
    e = rng.standard_normal((C, n, p))
    y = np.empty_like(e)
    y[:, 0] = e[:, 0]
    for t in range(1, n):
        y[:, t] = phi[:, 0] * y[:, t - 1] + e[:, t]
    y = y @ (np.eye(p) + 0.2 * rng.standard_normal((p, p))) + rng.standard_normal((C, 1, p))
    launches = -(-C // per_launch)
    # constant chains ('Not enough samples') in the second launch and in the last; none among the three long chains (a
    # chain that never gets going scans all n / 2 lag pairs: over a second per call at n = 5000)
    constant = [] if per_launch == 1 else ([per_launch + 2, C - 1] if launches > 1 else [C - 1])
    for c in constant:
        y[c] = 0.25 + c
    y = y.astype(np.float32).astype(np.float64)   # (f32 storage then holds the same numbers)
    want, covs = [], []
    for i in range(C):
        try:
            want.append(st.inse_mc_cov(torch.tensor(y[i])).numpy())
        except RuntimeError:  # 'Not enough samples' (inse_mc_cov.py:45-46): also what n <= 2 p gives
            want.append(None)
        covs.append(st.cov(torch.tensor(y[i]), rowvar=False).numpy())
    assert all(want[c] is None for c in constant)
    if n > 2 * p:  # every launch has chains with a real MC covariance
        for c0 in range(0, C, per_launch):
            assert any(w is not None for w in want[c0:c0 + per_launch]), c0
    for dt in (torch.float64, torch.float32):
        for layout in ("cnp", "ncp"):
            xs = _t(y, dt) if layout == "cnp" else _t(y, dt).permute(1, 0, 2).contiguous()
            monkeypatch.setenv("EY_MV_WORKSPACE_MB", "1")
            r = _mv_call(xs, layout)
            monkeypatch.delenv("EY_MV_WORKSPACE_MB")
            one = _mv_call(xs, layout)
            for k in r:
                a, b = r[k], one[k]
                same = torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)
                assert same, f"{k}: {launches} launches differ from one ({p}, {n}, {C}, {layout}, {dt})"
            sig, cov, mean, pairs = (r[k].cpu().numpy() for k in ("sig", "cov", "mean", "pairs"))
            np.testing.assert_allclose(mean, y.mean(1), rtol=1e-11, atol=1e-13)
            for i in range(C):
                info = str((i, p, n, layout, dt))
                scale = max(np.abs(covs[i]).max(), 0.0 if want[i] is None else np.abs(want[i]).max())
                np.testing.assert_allclose(cov[i], covs[i], rtol=1e-10, atol=1e-13 * scale, err_msg=info)
                if want[i] is None:
                    assert np.isnan(sig[i]).all() and pairs[i] == -1, info
                    continue
                np.testing.assert_allclose(sig[i], want[i], rtol=1e-8, atol=1e-11 * scale, err_msg=info)
                assert np.array_equal(sig[i], sig[i].T) and pairs[i] > 0, info


# ------------------------------------------------------------------------------------ XCD block maps under the oracle
# MLP(d0-d1-2), sigmoid hidden layer, CE-sum, f32 in the bf16x3 form, forced layerwise (variant bits 4 and 14).  The grids
# follow bgemm_one's tile rule (ey_large.hip): neither M nor N <= 32 -> 128 x 128 tiles, grid = (ceil(N / 128),
# ceil(M / 128), chains) = (gx, gy, gz).
#
# Rows map (xcd_block_rows; else the base map xcd_block): the first layer's forward product H1 = x W1^T, M = rows,
# N = d1 = 33 (not a multiple of 4, so the small-K kernel does not take it), K = d0 = 16, on the pre-split image of x
# (rows > 32, d1 > 32, d0 >= 16): gx = 1; the map needs gy even and gz % 4 == 0.
#   dims, rows, chains, bound on chains per chunk (0: none), what the grid is and which map it takes
XCD_ROWS = [
    ([16, 33, 2], 129, 4, 0, "(1, 2, 4): rows map"),
    ([16, 33, 2], 129, 8, 0, "(1, 2, 8): rows map"),
    ([16, 33, 2], 385, 4, 0, "(1, 4, 4): rows map"),
    ([16, 33, 2], 385, 8, 0, "(1, 4, 8): rows map"),
    ([16, 33, 2], 257, 4, 0, "(1, 3, 4): gy odd, base map (12 blocks: 8 remapped + 4)"),
    ([16, 33, 2], 257, 8, 0, "(1, 3, 8): gy odd, base map"),
    ([16, 33, 2], 129, 5, 0, "(1, 2, 5): gz % 4 != 0, base map (10 blocks: 8 remapped + 2)"),
    ([16, 33, 2], 129, 6, 0, "(1, 2, 6): gz % 4 != 0, base map (12 blocks)"),
    ([16, 33, 2], 385, 6, 0, "(1, 4, 6): gz % 4 != 0, base map (24 blocks)"),
    ([16, 33, 2], 129, 6, 4, "chunks of 4 + 2 chains in one call: (1, 2, 4) rows map, then (1, 2, 2) base map"),
    # beyond the generic kernels' LDS image, so that ey_forward runs the layerwise loop too: M = 129, N = 128, K = 300
    ([300, 128, 2], 129, 4, 0, "(1, 2, 4): rows map, in the evaluation and in ey_forward"),
]
# Cols map (xcd_block_cols): the first layer's weight gradient dW1 = delta1^T x, M = d1, N = d0, K = rows = 40, x
# pre-split as the B operand (d0 > 32): the map needs gx even and (gy gz) % 4 == 0.  bgemm() first splits a product whose
# N is 1 .. 32 columns past a multiple of 128 (and M > 32): the body keeps the image and has N - N % 128 columns, the
# remainder runs elsewhere without it.  So d0 = 129 leaves a body of ONE block column (base map), d0 = 257 a body of two.
XCD_COLS = [
    ([129, 33, 2], 40, 4, 0, "body 128 columns, (1, 1, 4): gx odd, base map (4 blocks: nothing remapped)"),
    ([129, 129, 2], 40, 2, 0, "body 128 columns, (1, 2, 2): gx odd, base map"),
    ([257, 33, 2], 40, 4, 0, "body 256 columns, (2, 1, 4): cols map"),
    ([257, 33, 2], 40, 3, 0, "body 256 columns, (2, 1, 3): gy gz % 4 != 0, base map (6 blocks)"),
    ([257, 129, 2], 40, 2, 0, "body 256 columns, (2, 2, 2): cols map through gy gz = 4"),
    ([161, 33, 2], 40, 4, 0, "no split (33 columns past 128), (2, 1, 4): cols map"),
    ([161, 33, 2], 40, 8, 0, "no split, (2, 1, 8): cols map"),
    ([289, 33, 2], 40, 4, 0, "no split, (3, 1, 4): gx odd, base map (12 blocks)"),
    ([161, 33, 2], 40, 6, 4, "chunks of 4 + 2 chains in one call: (2, 1, 4) cols map, then (2, 1, 2) base map"),
]


@pytest.mark.parametrize("dims,N,C,cap,grid", [pytest.param(*c, id=f"{'x'.join(map(str, c[0]))}-N{c[1]}-C{c[2]}-cap{c[3]}")
                                               for c in XCD_ROWS + XCD_COLS])
def test_xcd_block_maps_vs_oracle(dims, N, C, cap, grid):
    """Value and every gradient entry of every chain against the f64 C oracle at the f32 tolerances of
    test_small_batch_vs_oracle, on the SECOND of two different theta batches evaluated back to back on one plan, into
    NaN-filled outputs: a remap that is not a bijection leaves a tile to no workgroup, and that tile then holds the first
    batch's numbers (or NaN), not this batch's."""
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import Plan
    rng = np.random.default_rng(sum(dims) + 3 * N + C)
    x = rng.standard_normal((N, dims[0])).astype(np.float32)
    y = np.eye(2, dtype=np.float32)[rng.integers(0, 2, N)]
    old = L.lib().ey_debug_set_variant(16 | 16384)
    try:
        pl = Plan(dims, [1, 1], [1, 0], 1, torch.float32, DEV)
    finally:
        L.lib().ey_debug_set_variant(old)
    pl.set_data(_t(x, torch.float32), _t(y, torch.float32))
    P = pl.P
    mu = (0.1 * rng.standard_normal(P)).astype(np.float32).astype(np.float64)
    sigma = (0.5 + rng.random(P)).astype(np.float32).astype(np.float64)
    pl.set_prior(torch.tensor(mu), torch.tensor(sigma))
    assert pl.kernel == "bgemm" and pl.f32_products == "bf16x3"
    pl.max_chunk_chains = cap
    co = COracle(dims, [1, 0], 1, x.astype(np.float64), y.astype(np.float64), mu, sigma, dtype=np.float64, nthreads=4)
    temp = np.linspace(1.0, 0.5, C).astype(np.float32)
    ths = [(s / np.sqrt(dims[0]) * rng.standard_normal((C, P))).astype(np.float32) for s in (1.0, 1.7)]
    temp_d = _t(temp, torch.float32)
    for th in ths:   # the second batch's results stay in t, g
        th_d = _t(th, torch.float32)
        t = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
        g = torch.full((C, P), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.lib().ey_log_target_grad(pl.handle, L.ptr(th_d), L.ptr(temp_d), C, L.ptr(t), L.ptr(g), _stream()),
                "ey_log_target_grad")
        torch.cuda.synchronize()
    tk, gk = t.cpu().numpy(), g.cpu().numpy()
    assert np.isfinite(tk).all() and np.isfinite(gk).all(), grid
    rt, at = 3e-4, 3e-3
    for c in range(C):
        co.temp = float(temp[c])
        to, go, _, _ = co.log_target_grad(ths[1][c].astype(np.float64))
        g_first = co.log_target_grad(ths[0][c].astype(np.float64))[1]
        assert (np.abs(g_first - go) > 10 * (rt * 10 * np.abs(go) + at / 10 * max(1.0, np.abs(go).max()))).mean() > 0.5, \
            "the first batch's gradient must be far outside the tolerance of the second's"
        np.testing.assert_allclose(tk[c], to, rtol=rt, atol=at, err_msg=f"chain {c}: {grid}")
        np.testing.assert_allclose(gk[c], go, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(go).max()),
                                   err_msg=f"chain {c}: {grid}")
    # the network outputs take the first layer's product too (ey_forward runs the layerwise loop only for a model beyond
    # the generic kernels' LDS image; the smaller ones' outputs come from the generic kernel)
    out = torch.full((C, N, 2), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.lib().ey_forward(pl.handle, L.ptr(th_d), C, L.ptr(out), _stream()), "ey_forward")
    torch.cuda.synchronize()
    from tests.prior_restatement import Target
    ref = Target(dims, [1, 0], 1, x, y, None)
    for c in range(C):
        want = ref.forward(torch.tensor(ths[1][c].astype(np.float64))).numpy()
        np.testing.assert_allclose(out[c].cpu().numpy(), want, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(want).max()),
                                   err_msg=f"forward, chain {c}: {grid}")


# --------------------------------------------------------------------------------- grid-stride loops behind a block cap
PHILOX_PASS = 65536 * 256   # threads of the capped grid: flat index k and k + PHILOX_PASS are one thread's


@pytest.mark.parametrize("C", [664, 1321])
def test_philox_normal_beyond_one_grid_pass(C):
    """ey_philox_normal, f32, P = 101770 (MLP(784-128-10)): a thread draws one block of four elements, a chain has 25443 of
    them, the grid is capped at 65536 x 256 threads.  664 chains are 16 894 152 blocks, just past one pass; 1321 chains are
    past two.  Against the numpy twin (its chain_offset names the chains): chain 0, the chains around flat block
    16 777 216 (in chain 659) and twice that (in chain 1318), and the last chain, at test_philox.py's 4e-6."""
    from eeyore_amd import _lib as L
    P, seed, it, off = 101770, 2024, 3, 7
    nb = (P + 3) // 4
    assert C * nb > PHILOX_PASS * (1 if C == 664 else 2)
    out = torch.full((C, P), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.lib().ey_philox_normal(L.ptr(out), C, P, seed, it, off, L.EY_F32, _stream()), "ey_philox_normal")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    chains = {0, C - 1}
    for k in range(1, C * nb // PHILOX_PASS + 1):
        c = k * PHILOX_PASS // nb
        assert 0 < c < C - 1
        chains |= {c - 1, c, c + 1}
    assert len(chains) == (5 if C == 664 else 8)
    for c in sorted(chains):
        want = po.normal(1, P, seed, it, off + c, np.float32)[0]
        np.testing.assert_allclose(out[c].cpu().numpy(), want, rtol=4e-6, atol=4e-6, err_msg=f"chain {c}")


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_philox_uniform_blocks_beyond_one_grid_pass(tag):
    """ey_philox_uniform_blocks at C S = 4097 x 4096, 4096 elements past one pass of the capped grid: bit for bit against
    the twin on the first chain, the chains around element 16 777 216 (chain 4096, word 0) and the last chain."""
    from eeyore_amd import _lib as L
    C, S, seed, it, off = 4097, 4096, 77, 2 ** 32 + 9, 2 ** 33 + 5
    tdt, ndt, code = (torch.float32, np.float32, L.EY_F32) if tag == "f32" else (torch.float64, np.float64, L.EY_F64)
    assert PHILOX_PASS < C * S and PHILOX_PASS // S == C - 1
    out = torch.full((C, S), float("nan"), dtype=tdt, device=DEV)
    L.check(L.lib().ey_philox_uniform_blocks(L.ptr(out), C, S, seed, it, off, code, _stream()), "ey_philox_uniform_blocks")
    torch.cuda.synchronize()
    assert ((out >= 0) & (out < 1)).all()
    chains = [0, 1, C - 3, C - 2, C - 1]
    want = po.uniform_blocks([off + c for c in chains], S, seed, it, ndt)
    assert np.array_equal(out[chains].cpu().numpy(), want)
    assert np.array_equal(out[:, 0].cpu().numpy(), po.uniform(C, seed, it, off, ndt))


def test_stats_update_beyond_one_grid_pass():
    """ey_stats_update at C P = 3190 x 1315 = 4 194 850 f32 elements: more groups of four than 4096 x 256 threads (the
    second pass serves the last 137), and n % 4 == 2 (the last group takes the element-wise branch).  Three updates against
    torch's f64 sums as in test_chain_stats_hip_pass_equals_torch_formulas: s1 and acc exact, s2 at 1e-15."""
    from eeyore_amd.distributed import ChainStats
    C, P = 3190, 1315
    assert (C * P + 3) // 4 > 4096 * 256 and (C * P) % 4 == 2
    g = torch.Generator(device="cpu").manual_seed(3)
    xs = torch.randn(3, C, P, generator=g, dtype=torch.float32)
    acc = (torch.rand(3, C, generator=g) < 0.6).to(torch.uint8)
    hip = ChainStats(C, P, DEV)
    for i in range(3):
        hip.update(xs[i].to(DEV), acc[i].to(DEV))
    torch.cuda.synchronize()
    s1 = (xs[0].double() + xs[1].double()) + xs[2].double()
    s2 = (xs[0].double() ** 2 + xs[1].double() ** 2) + xs[2].double() ** 2
    assert torch.equal(hip.s1.cpu(), s1) and torch.equal(hip.acc.cpu(), acc.double().sum(0))
    np.testing.assert_allclose(hip.s2.cpu().numpy(), s2.numpy(), rtol=1e-15)


def test_stats_update_run_beyond_one_grid_pass():
    """ey_stats_update_run (the attached moments of a recorded run) at C P = 6380 x 1315 = 8 389 700 elements, five recorded
    iterations: more groups of four than 8192 x 256 threads (the second pass serves the last 273), and five iterations are
    one block of four plus one.  MLP(4-32-32-3) on eight rows, one leapfrog step per draw; the sums against torch's f64
    sums of the records in iteration order: s1 and acc exact, s2 at 1e-15."""
    from eeyore_amd.distributed import ChainStats
    from eeyore_amd.plan import Plan
    C, n_it = 6380, 5
    rng = np.random.default_rng(4)
    pl = Plan([4, 32, 32, 3], [1, 1, 1], [1, 1, 0], 1, torch.float32, DEV)
    pl.set_data(_t(rng.standard_normal((8, 4)), torch.float32), _t(np.eye(3)[rng.integers(0, 3, 8)], torch.float32))
    pl.set_prior(torch.zeros(pl.P), torch.full((pl.P,), 1.5))
    P = pl.P
    assert P == 1315 and (C * P + 3) // 4 > 8192 * 256 and (C * P) % 4 == 0
    th = (0.2 * pl.philox_normal(C, seed=5, it=0)).contiguous()
    t, g = pl.log_target_grad(th)
    st = ChainStats(C, P, DEV)
    st.attach(pl)
    samples, acc = pl.empty(n_it, C, P), pl.empty(n_it, C, dtype=torch.uint8)
    pl.hmc_run(th, t, g, 0.05, 1, n_it, seed=5, it=1, samples=samples, accepted_rec=acc)
    torch.cuda.synchronize()
    pl.detach_moments()
    assert 0 < int(acc.sum().item()) < n_it * C and not torch.equal(samples[0], samples[n_it - 1])
    s1 = torch.zeros(C, P, dtype=torch.float64, device=DEV)
    s2 = torch.zeros(C, P, dtype=torch.float64, device=DEV)
    for i in range(n_it):
        s1 += samples[i].double()
        s2 += samples[i].double() ** 2
    assert torch.equal(st.s1, s1) and torch.equal(st.acc, acc.double().sum(0))
    np.testing.assert_allclose(st.s2.cpu().numpy(), s2.cpu().numpy(), rtol=1e-15)
