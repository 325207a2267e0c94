"""Every wave slot and chain round of the persistent kernels: k_fused16 (ey_fused16.hip), k_mfma32 / k_mfma32p
(ey_mfma32.hip) and k_mid32 / k_mid (ey_mid.hip).

Each launches grid = min(C, n_cu) workgroups and lets every wave (fused16, mfma32) or workgroup (mid) walk over chains
blockIdx.x + gridDim.x * wave, + gridDim.x * WAVES, ...  A wave's chains reuse its LDS region, the zero padding written
once at kernel entry, the delta2 buffer and (k_mid32) a prefetch of the next round's parameters.  The oracle suites run
C = 11 (test_fused16.py, the mid tests): wave 0, round 0 only.  Here:

  * tiled replicas: B = 11 distinct base chains (11 is coprime to every grid and wave count in play, so a wave meets another
    base chain in each of its rounds), every per-chain input tiled as input[c] = base[c % 11], ONE launch with a C that
    keeps every wave of every workgroup busy for two rounds and a ragged third.  Every replica must equal replica 0 bit
    for bit, replica 0 must equal the same 11 chains launched alone (another grid, another chain-to-wave map), and those
    are held against the C oracle at the tolerances of tests/test_fused16.py (f64 1e-10, f32 2e-4) and of the mfma32 / mid
    tests of tests/test_gpu_parity.py.  No tolerance between replicas: a difference is a finding (the message names the
    (block, wave, round) slots that differ).
  * Philox blocks, the shard contract of eeyore_amd/distributed.py: a launch of distinct chains with in-kernel random
    streams and records against slices of 11 chains run alone with chain_offset = c0, bit for bit, the slices chosen with
    slot() from wave 0, a middle wave, the last wave, rounds 0, 1, 2 and the ragged end.

The non-persistent paths are left out on purpose: the generic kernels (one workgroup per chain; row_waves = 'auto' switches
at C > 4 n_cu, ey_generic.hip) and the layerwise bgemm products may order a sum by the launch."""
import numpy as np
import pytest
import torch

from oracle.c_oracle import COracle

DEV = "cuda:0"
B = 11  # base chains


# ------------------------------------------------------------------------------------------------ slot arithmetic (pure)
def slot(chain, grid, waves):
    """(block, wave, round) of a chain: chain = block + grid * wave + grid * waves * round (k_fused16, k_mfma32; the mid
    kernels with waves = 1: a workgroup is the unit there)."""
    return chain % grid, (chain // grid) % waves, chain // (grid * waves)


def fused16_waves(tag, H):
    """Waves per workgroup of the k_fused16 instantiation that serves hidden width H (f16_launch, ey_fused16.hip):
    f32 H <= 16: EY_F16_W16 = 16, H <= 32: 8, else 4; f64 H <= 16: 8, else 4."""
    return {("f32", 16): 16, ("f32", 32): 8, ("f32", 64): 4, ("f64", 16): 8, ("f64", 32): 4}[(tag, _tile_width(H))]


def _tile_width(H):
    return 16 if H <= 16 else (32 if H <= 32 else 64)


def chains_for(n_cu, waves):
    """Every wave of every workgroup busy, two full rounds, and a ragged third that ends partway through a workgroup row."""
    if waves == 1:  # the mid kernels
        return 2 * n_cu + n_cu // 2 + 7
    return 2 * n_cu * waves + min(3, waves - 1) * n_cu + 7


def check_coverage(C, grid, waves):
    rounds = {}
    for chain in range(C):
        b, w, r = slot(chain, grid, waves)
        assert chain == b + grid * (w + waves * r)
        rounds.setdefault((b, w), []).append(chain)
    assert len(rounds) == grid * waves, "every (block, wave) pair has a chain"
    counts = {len(v) for v in rounds.values()}
    assert min(counts) >= 2 and counts == {2, 3}, counts
    for chains in rounds.values():  # what makes the replicas meaningful: a wave never meets the same base chain twice running
        assert all(a % B != b % B for a, b in zip(chains, chains[1:]))
    last = slot(C - 1, grid, waves)
    assert last[0] < grid - 1, "the last round ends partway through a workgroup row"


def slice_offsets(C, grid, waves):
    """Starts of the 11-chain slices of the Philox-block tests: wave 0, the last wave (running over into round 1), a middle
    wave in round 1, round 2, and the ragged end of the launch."""
    at = lambda b, w, r: b + grid * (w + waves * r)
    return [0, at(grid - 5, waves - 1, 0), at(grid - 5, waves // 2, 1), at(5, 0, 2), C - B]


WAVE_TABLE = [16, 8, 4, 1]  # fused16 f32 H16 | fused16 f32 H32, f64 H16, mfma32 | fused16 f32 H64, f64 H32, mfma32p | mid


@pytest.mark.parametrize("waves", WAVE_TABLE)
@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_chosen_chain_count_covers_every_slot(n_cu, waves):
    C = chains_for(n_cu, waves)
    check_coverage(C, n_cu, waves)
    offs = slice_offsets(C, n_cu, waves)
    assert all(0 <= c0 and c0 + B <= C for c0 in offs) and offs[-1] + B == C
    seen = [slot(c, n_cu, waves) for c0 in offs for c in range(c0, c0 + B)]
    assert {0, waves // 2, waves - 1} <= {s[1] for s in seen} and {0, 1, 2} <= {s[2] for s in seen}


def test_slot_of_the_four_wave_launch_of_mfma32():
    """Variant bit 0 of k_mfma32: ceil(C / 4) workgroups of four waves, one chain per wave."""
    C = 2823
    grid = (C + 3) // 4
    assert {slot(c, grid, 4)[2] for c in range(C)} == {0}
    assert len({slot(c, grid, 4)[:2] for c in range(C)}) == C


# ------------------------------------------------------------------------------------------------ replicas on the device
def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _t(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


class Replicas:
    def __init__(self, C, grid, waves):
        self.C, self.grid, self.waves = C, grid, waves
        self.idx = torch.arange(C, device=DEV) % B

    def tile(self, t):
        return None if t is None else t[self.idx].contiguous()

    def _where(self, bad):
        bad = bad.reshape(bad.shape[0], -1).any(1)
        first = ", ".join(f"chain {c} (base {c % B}) at (block, wave, round) {slot(c, self.grid, self.waves)}"
                          for c in torch.nonzero(bad).flatten()[:6].tolist())
        n0 = min(self.C, self.grid * self.waves)
        return (f"{int(bad.sum())} of {bad.shape[0]} chains differ, {int(bad[:n0].sum())} of them in round 0; first: {first}")

    def check(self, what, big, small):
        """big: outputs of the tiled launch, small: of the 11 base chains launched alone."""
        for k, v in big.items():
            assert v.shape[0] == self.C and small[k].shape[0] == B
            if v.is_floating_point():
                assert torch.isfinite(v).all() and torch.isfinite(small[k]).all(), (what, k)
            want = v[:B][self.idx]
            if not torch.equal(v, want):
                raise AssertionError(f"{what}: '{k}' of a replica differs from replica 0: {self._where(v != want)}")
            if not torch.equal(v[:B], small[k]):
                raise AssertionError(f"{what}: '{k}' of replica 0 differs from the same chains launched alone (C = {B}): "
                                     f"base chains {torch.nonzero((v[:B] != small[k]).reshape(B, -1).any(1)).flatten().tolist()}")

    def both(self, what, fn, *base):
        """fn on the tiled inputs and on the base inputs (each call gets tensors of its own: the steps work in place)."""
        big = fn(*[self.tile(a) for a in base])
        small = fn(*[None if a is None else a.clone() for a in base])
        self.check(what, big, small)
        return small


def _value_grad(pl):
    def fn(th, temp=None):
        t, g = pl.log_target_grad(th, temp=temp)
        return dict(target=t, grad=g)
    return fn


def _leapfrog(pl, eps, Ls):
    def fn(th, p):
        t, g = pl.leapfrog(th, p, eps, Ls)
        return dict(theta=th, p=p, target=t, grad=g)
    return fn


def _hmc(pl, eps, Ls, flags=0):
    def fn(th, t, g, p0, u, temp=None, step_vec=None):
        out = pl.hmc_step(th, t, g, eps, Ls, p0=p0, u=u, temp=temp, step_vec=step_vec, flags=flags)
        return dict(theta=th, target=t, grad=g, **out)
    return fn


def _mala(pl, step):
    def fn(th, t, g, z, u):
        out = pl.mala_step(th, t, g, step, z=z, u=u)
        return dict(theta=th, target=t, grad=g, **out)
    return fn


def _mh(pl, scale):
    def fn(th, t, z, u):
        out = pl.mh_step(th, t, torch.full((pl.P,), scale, dtype=pl.dtype), z=z, u=u)
        return dict(theta=th, target=t, **out)
    return fn


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _data(rng, dims, lik, N):
    x = rng.standard_normal((N, dims[0]))
    y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)] if lik == 1 else (rng.random((N, dims[-1])) < 0.5).astype(np.float64)
    return x, y


def _f64_oracle(co, dims, acts, lik, bias=None):
    return COracle(dims, acts, lik, co.x.astype(np.float64), co.y.astype(np.float64), co.mu.astype(np.float64),
                   co.sigma.astype(np.float64), dtype=np.float64, nthreads=4, bias=bias)


def _hmc_oracle(co, th0, t0, g0, p0, u, eps, Ls, temps=None, steps=None):
    """co.hmc_draw of the base chains; with per-chain temperatures / steps one call per chain."""
    tho, tvo, go = th0.copy(), t0.copy(), g0.copy()
    if temps is None and steps is None:
        acc, hc, hp = co.hmc_draw(tho, tvo, go, p0, u, eps, Ls)
        return tho, tvo, go, acc, hc, hp
    acc, hc, hp = np.zeros(B, np.uint8), np.zeros(B, co.dt), np.zeros(B, co.dt)
    keep = co.temp
    for c in range(B):
        co.temp = float(temps[c])
        a, b, d = co.hmc_draw(tho[c:c + 1], tvo[c:c + 1], go[c:c + 1], np.ascontiguousarray(p0[c:c + 1]),
                              np.ascontiguousarray(u[c:c + 1]), float(steps[c]), Ls)
        acc[c], hc[c], hp[c] = a[0], b[0], d[0]
    co.temp = keep
    return tho, tvo, go, acc, hc, hp


# ------------------------------------------------------------------------------------------------ fused16
# one shape per instantiation group (dtype, H) x {two hidden / one hidden} x {exact / padded}, from the shapes
# tests/test_fused16.py holds against the oracle at C = 11
FUSED16_SHAPES = [
    ([4, 16, 16, 3], [1, 1, 0], 1, "f32"), ([4, 16, 3], [1, 0], 1, "f32"), ([4, 10, 7, 3], [1, 1, 0], 1, "f32"),
    ([3, 9, 4], [1, 0], 1, "f32"),
    ([5, 32, 32, 2], [3, 2, 1], 0, "f32"), ([8, 32, 2], [2, 0], 1, "f32"), ([4, 20, 20, 3], [1, 1, 0], 1, "f32"),
    ([16, 24, 12], [2, 0], 1, "f32"),
    ([3, 64, 64, 2], [1, 2, 1], 0, "f32"), ([4, 50, 1], [3, 1], 0, "f32"),
    ([4, 16, 16, 3], [1, 1, 0], 1, "f64"), ([4, 16, 3], [1, 0], 1, "f64"), ([3, 7, 12, 1], [2, 1, 1], 0, "f64"),
    ([3, 9, 4], [1, 0], 1, "f64"),
    ([4, 32, 32, 3], [1, 1, 0], 1, "f64"),  # the headline model in the reference's default dtype
    ([8, 32, 2], [2, 0], 1, "f64"), ([4, 20, 20, 3], [1, 1, 0], 1, "f64"), ([5, 20, 7], [1, 0], 1, "f64"),
]


def fused16_group(dims, tag):
    """(dtype, H, V) of the instantiation, as f16_launch / f16_launch_w choose it (every layer here has a bias)."""
    h1, h2 = dims[1], dims[-2]
    H = _tile_width(max(h1, h2))
    hidden = len(dims) - 2
    pad = h1 != H or h2 != H or H == 64 or dims[0] > 8 or dims[-1] > 4
    return f"{tag}-H{H}-{hidden}hidden-{'padded' if pad else 'exact'}"


def _fused16_id(case):
    dims, _, _, tag = case
    return fused16_group(dims, tag) + "-" + "x".join(map(str, dims))


def test_fused16_shapes_cover_every_group():
    groups_ = {fused16_group(d, tag) for d, _, _, tag in FUSED16_SHAPES}
    want = {f"{tag}-H{H}-{k}hidden-{e}" for tag, H in (("f32", 16), ("f32", 32), ("f64", 16), ("f64", 32))
            for k in (1, 2) for e in ("exact", "padded")}
    want |= {"f32-H64-1hidden-padded", "f32-H64-2hidden-padded"}  # H = 64 only ever takes the padded instantiations
    assert groups_ == want


def _fused16_setup(dims, acts, lik, tag, N):
    from eeyore_amd.plan import Plan
    npdt, dt = (np.float64, torch.float64) if tag == "f64" else (np.float32, torch.float32)
    rng = np.random.default_rng(sum(dims) + N + len(dims))
    x, y = _data(rng, dims, lik, N)
    pl = Plan(dims, [1] * (len(dims) - 1), acts, lik, dt, DEV)
    pl.set_data(_t(x, dt), _t(y, dt))
    P = pl.P
    mu, sigma = 0.1 * rng.standard_normal(P), 0.5 + rng.random(P)
    priors = {"elementwise": (mu, sigma), "uniform": (np.full(P, 0.05), np.full(P, 1.3))}
    oracles = {k: COracle(dims, acts, lik, x, y, m, s, dtype=npdt, nthreads=4) for k, (m, s) in priors.items()}
    return pl, priors, oracles, rng, npdt, dt


def _check_hmc_vs_oracle(o, ref, u, tag, tol):
    tho, tvo, go, acc, hc, hp = ref
    rate = np.minimum(np.exp(np.minimum(hc - hp, 0)), 1)
    decided = np.abs(u - rate) > (1e-8 if tag == "f64" else 5e-3)
    np.testing.assert_array_equal(o["accepted"][decided], acc[decided])
    np.testing.assert_allclose(o["h_prop"], hp, rtol=tol * 10, atol=tol * 100)
    np.testing.assert_allclose(o["h_cur"], hc, rtol=tol * 10, atol=tol * 100)
    same = o["accepted"] == acc
    np.testing.assert_allclose(o["theta"][same], tho[same], rtol=tol * 10, atol=tol)
    np.testing.assert_allclose(o["target"][same], tvo[same], rtol=tol * 5, atol=tol * 20)


def _check_log_rate(o, acc, lr, u, tag):
    ltol = (1e-9 if tag == "f64" else 2e-3) * np.maximum(1.0, np.abs(lr))
    assert (np.abs(o["log_rate"] - lr) <= ltol).all()
    decided = np.abs(np.log(u.astype(np.float64)) - lr) > ltol
    np.testing.assert_array_equal(o["accepted"][decided], acc[decided])


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED16_SHAPES, ids=_fused16_id)
def test_fused16_every_slot_and_round(case):
    """N = 33: three row tiles with a ragged last one, so the delta2 and label padding of the last tile is live when the wave's
    next chain starts.  Value + gradient (with and without a temperature), the leapfrog operator, the HMC draw three ways
    (uniform prior, no temperature: the F16_HMC_PLAIN instantiations of ey_fused16.hip / _plain.hip / _d32.hip; elementwise
    prior with per-chain temperature and step: the general ones; EY_RECOMPUTE_INITIAL_GRAD), MALA and MH."""
    from eeyore_amd import _lib as L
    dims, acts, lik, tag = case
    N, Ls = 33, 3
    pl, priors, oracles, rng, npdt, dt = _fused16_setup(dims, acts, lik, tag, N)
    assert pl.kernel == "fused16"
    waves, n_cu = fused16_waves(tag, max(dims[1:-1])), _n_cu()
    C = chains_for(n_cu, waves)
    grid = min(C, n_cu)
    check_coverage(C, grid, waves)
    rep = Replicas(C, grid, waves)
    P, tol = pl.P, (1e-10 if tag == "f64" else 2e-4)
    eps = 0.02 if lik == 1 else 0.01
    th0 = ((0.3 if lik == 1 else 0.15) * rng.standard_normal((B, P))).astype(npdt)
    p0, u = rng.standard_normal((B, P)).astype(npdt), rng.random(B).astype(npdt)
    th, p0_t, u_t = _t(th0, dt), _t(p0, dt), _t(u, dt)
    temps = torch.linspace(0.2, 1.0, B, dtype=dt, device=DEV)
    steps = (eps * torch.linspace(0.7, 1.3, B, dtype=torch.float64)).to(dt).to(DEV)

    # ---- the elementwise prior
    co = oracles["elementwise"]
    pl.set_prior(torch.tensor(priors["elementwise"][0]), torch.tensor(priors["elementwise"][1]))
    vg = rep.both("log_target_grad", _value_grad(pl), th)
    vgt = rep.both("log_target_grad, per-chain temperature", _value_grad(pl), th, temps)
    o, ot = _np(vg), _np(vgt)
    for c in range(B):
        to, go, _, _ = co.log_target_grad(th0[c])
        gs = max(1.0, float(np.abs(go).max()))
        np.testing.assert_allclose(o["target"][c], to, rtol=tol, atol=tol * 10)
        np.testing.assert_allclose(o["grad"][c], go, rtol=tol * 10, atol=tol * gs)
        np.testing.assert_allclose(ot["target"][c], temps[c].item() * to, rtol=tol * 2, atol=tol * 10)
        np.testing.assert_allclose(ot["grad"][c], temps[c].item() * go, rtol=tol * 10, atol=tol * gs)
    lf = _np(rep.both("leapfrog", _leapfrog(pl, eps, Ls), th, p0_t))
    for c in range(B):
        tho, po_, to, _ = co.leapfrog(th0[c], p0[c], eps, Ls)
        np.testing.assert_allclose(lf["theta"][c], tho, rtol=tol * 10, atol=tol)
        np.testing.assert_allclose(lf["p"][c], po_, rtol=tol * 50, atol=tol * 50)
        np.testing.assert_allclose(lf["target"][c], to, rtol=tol * 5, atol=tol * 20)
    t0, g0 = o["target"].astype(npdt), o["grad"].astype(npdt)
    gen = _np(rep.both("hmc_step, elementwise prior, per-chain temperature and step", _hmc(pl, 0.0, Ls),
                       th, vgt["target"], vgt["grad"], p0_t, u_t, temps, steps))
    _check_hmc_vs_oracle(gen, _hmc_oracle(co, th0, ot["target"].astype(npdt), ot["grad"].astype(npdt), p0, u, 0.0, Ls,
                                          temps.cpu().numpy(), steps.cpu().numpy()), u, tag, tol)
    rec = _np(rep.both("hmc_step, EY_RECOMPUTE_INITIAL_GRAD", _hmc(pl, eps, Ls, L.EY_RECOMPUTE_INITIAL_GRAD),
                       th, vg["target"], vg["grad"], p0_t, u_t))
    _check_hmc_vs_oracle(rec, _hmc_oracle(co, th0, t0, g0, p0, u, eps, Ls), u, tag, tol)
    co64 = _f64_oracle(co, dims, acts, lik)
    f8 = lambda a_: np.asarray(a_, dtype=np.float64).copy()
    ml = _np(rep.both("mala_step", _mala(pl, 0.004), th, vg["target"], vg["grad"], p0_t, u_t))
    _check_log_rate(ml, *co64.mala_draw(f8(th0), f8(t0), f8(g0), f8(p0), f8(u), 0.004), u, tag)
    mh = _np(rep.both("mh_step", _mh(pl, 0.02), th, vg["target"], p0_t, u_t))
    _check_log_rate(mh, *co64.mh_draw(f8(th0), f8(t0), f8(p0), f8(u), 0.02), u, tag)

    # ---- one prior for every parameter, no temperature: the plain HMC instantiations
    co = oracles["uniform"]
    pl.set_prior(torch.tensor(priors["uniform"][0]), torch.tensor(priors["uniform"][1]))
    vgu = rep.both("log_target_grad, uniform prior", _value_grad(pl), th)
    ou = _np(vgu)
    plain = _np(rep.both("hmc_step, uniform prior (plain)", _hmc(pl, eps, Ls), th, vgu["target"], vgu["grad"], p0_t, u_t))
    _check_hmc_vs_oracle(plain, _hmc_oracle(co, th0, ou["target"].astype(npdt), ou["grad"].astype(npdt), p0, u, eps, Ls),
                         u, tag, tol)


# ------------------------------------------------------------------------------------------------ Philox blocks
def _philox_blocks(pl, C, grid, waves, kind, step, Ls):
    """A launch of n_iters = 3 iterations of C distinct chains with in-kernel random streams and every record, against slices
    of 11 chains run alone with chain_offset = c0: state, records and counts equal the big launch's rows, bit for bit."""
    n, P = 3, pl.P

    def run(th, t, g, c0):
        c = th.shape[0]
        smp, tgt, acr = pl.empty(n, c, P), pl.empty(n, c), pl.empty(n, c, dtype=torch.uint8)
        cnt = torch.zeros(c, dtype=torch.int32, device=DEV)
        kw = dict(seed=3, it=10, chain_offset=c0, samples=smp, targets=tgt, accepted_rec=acr, accept_count=cnt)
        out = pl.hmc_run(th, t, g, step, Ls, n, **kw) if kind == "hmc" else pl.mala_run(th, t, g, step, n, **kw)
        return dict(theta=th, target=t, grad=g, accept_count=cnt, accepted=out["accepted"]), dict(samples=smp, targets=tgt,
                                                                                                  accepted_rec=acr)
    th0 = (0.2 * pl.philox_normal(C, seed=9, it=0)).contiguous()
    t0, g0 = pl.log_target_grad(th0)
    state, recs = run(th0.clone(), t0.clone(), g0.clone(), 0)
    for v in (state["theta"], state["target"], state["grad"], recs["samples"], recs["targets"]):
        assert torch.isfinite(v).all()
    assert 0 < int(state["accept_count"].sum().item()) < n * C  # accepted and rejected draws both
    offs = slice_offsets(C, grid, waves)
    seen = [slot(c, grid, waves) for c0 in offs for c in range(c0, c0 + B)]
    assert {0, waves // 2, waves - 1} <= {s[1] for s in seen} and {0, 1, 2} <= {s[2] for s in seen}
    for c0 in offs:
        s_state, s_recs = run(th0[c0:c0 + B].clone(), t0[c0:c0 + B].clone(), g0[c0:c0 + B].clone(), c0)
        where = f"{kind}_run, chains [{c0}, {c0 + B}) from (block, wave, round) {slot(c0, grid, waves)}"
        for k, v in s_state.items():
            assert torch.equal(v, state[k][c0:c0 + B]), (where, k)
        for k, v in s_recs.items():
            assert torch.equal(v, recs[k][:, c0:c0 + B]), (where, k)


PHILOX_FUSED16 = [
    ([4, 16, 16, 3], [1, 1, 0], 1, "f32", "hmc"), ([4, 20, 20, 3], [1, 1, 0], 1, "f32", "hmc"),
    ([4, 20, 20, 3], [1, 1, 0], 1, "f32", "mala"),
    ([4, 32, 32, 3], [1, 1, 0], 1, "f64", "hmc"), ([3, 9, 4], [1, 0], 1, "f64", "hmc"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PHILOX_FUSED16, ids=lambda c: _fused16_id(c[:4]) + "-" + c[4])
def test_fused16_philox_blocks_are_the_big_launch_rows(case):
    dims, acts, lik, tag, kind = case
    pl, priors, _, _, _, _ = _fused16_setup(dims, acts, lik, tag, 33)
    pl.set_prior(torch.tensor(priors["uniform"][0]), torch.tensor(priors["uniform"][1]))
    assert pl.kernel == "fused16"
    waves, n_cu = fused16_waves(tag, max(dims[1:-1])), _n_cu()
    C = chains_for(n_cu, waves)
    _philox_blocks(pl, C, min(C, n_cu), waves, kind, 0.03 if kind == "hmc" else 0.002, 3)


# ------------------------------------------------------------------------------------------------ mfma32
HEADLINE = ([4, 32, 32, 3], [1, 1, 0], 1)
MFMA32_CASES = [
    # model, N, product form, variant, prior, waves, operations
    (HEADLINE, 33, "bf16x3", 0, "uniform", 8, "all"),
    (HEADLINE, 150, "bf16x3", 0, "uniform", 8, "all"),
    (HEADLINE, 33, "exact", 0, "uniform", 8, "all"),
    (HEADLINE, 150, "exact", 0, "uniform", 8, "all"),
    (HEADLINE, 33, "bf16x3", 0, "elementwise", 8, "all"),
    (HEADLINE, 150, "exact", 0, "elementwise", 8, "all"),
    (HEADLINE, 33, "bf16x3", 1, "uniform", 4, "hmc"),   # variant bit 0: four-wave workgroups, one chain per wave
    (HEADLINE, 33, "bf16x3", 8, "uniform", 4, "hmc"),   # variant bit 3: k_mfma32p, one wave per SIMD
    (([4, 32, 32, 3], [2, 2, 0], 1), 33, "bf16x3", 0, "uniform", 8, "all"),        # tanh: bf16x3 form only
    (([4, 32, 32, 1], [1, 1, 1], 0), 150, "bf16x3", 0, "elementwise", 8, "all"),   # the BCE head
]


def _mfma32_id(case):
    (dims, acts, _), N, products, variant, prior, waves, ops = case
    return f"{'x'.join(map(str, dims))}-act{acts[0]}-N{N}-{products}-v{variant}-{prior}-{waves}waves"


def _mfma32_setup(model, N, products, prior):
    from eeyore_amd.plan import Plan
    dims, acts, lik = model
    rng = np.random.default_rng(N + dims[-1] + acts[0])
    x, y = _data(rng, dims, lik, N)
    pl = Plan(dims, [1, 1, 1], acts, lik, torch.float32, DEV)
    pl.f32_products = products
    pl.set_data(_t(x, torch.float32), _t(y, torch.float32))
    P = pl.P
    mu, sigma = (0.2 * rng.standard_normal(P), 0.5 + rng.random(P)) if prior == "elementwise" else (np.zeros(P), np.full(P, np.sqrt(3.0)))
    pl.set_prior(torch.tensor(mu), torch.tensor(sigma))
    co = COracle(dims, acts, lik, x, y, mu, sigma, dtype=np.float32, nthreads=4)
    return pl, co, rng


@pytest.mark.gpu
@pytest.mark.parametrize("case", MFMA32_CASES, ids=_mfma32_id)
def test_mfma32_every_slot_and_round(case):
    """N = 33 (a last tile of one row: the peeled copy) and N = 150, both product forms, the elementwise-prior path, the
    four-wave launch, the pipelined kernel and two of the other 4-32-32 models.  Replica 0 against the f32 C oracle as
    test_mfma32_row_counts_vs_oracle / test_mfma32_elementwise_prior_vs_oracle / test_mfma32_mala_and_mh_vs_oracle_and_generic
    of tests/test_gpu_parity.py do."""
    model, N, products, variant, prior, waves, ops = case
    dims, acts, lik = model
    pl, co, rng = _mfma32_setup(model, N, products, prior)
    assert pl.kernel == "mfma32" and pl.f32_products == products
    n_cu = _n_cu()
    C = chains_for(n_cu, waves)
    grid = min(C, n_cu) if variant != 1 else (C + 3) // 4
    if variant != 1:
        check_coverage(C, grid, waves)
    dt, P = torch.float32, pl.P
    th0 = (0.3 * rng.standard_normal((B, P))).astype(np.float32)
    p0, u = rng.standard_normal((B, P)).astype(np.float32), rng.random(B).astype(np.float32)
    th, p0_t, u_t = _t(th0, dt), _t(p0, dt), _t(u, dt)
    rep8 = Replicas(chains_for(n_cu, 8), min(chains_for(n_cu, 8), n_cu), 8)
    vg = rep8.both("log_target_grad", _value_grad(pl), th)   # (the variants concern the HMC draw alone)
    o = _np(vg)
    for c in range(B):
        to, go, _, _ = co.log_target_grad(th0[c])
        np.testing.assert_allclose(o["target"][c], to, rtol=2e-4, atol=2e-3)
        np.testing.assert_allclose(o["grad"][c], go, rtol=2e-4, atol=2e-4 * max(1.0, np.abs(go).max()))
    rep = Replicas(C, grid, waves)
    pl.set_variant(variant)
    try:
        assert pl.kernel == "mfma32"
        eps, Ls = 0.02, 3
        hm = _np(rep.both(f"hmc_step, variant {variant}", _hmc(pl, eps, Ls), th, vg["target"], vg["grad"], p0_t, u_t))
    finally:
        pl.set_variant(0)
    tho, tvo, go, acc, hc, hp = _hmc_oracle(co, th0, o["target"].copy(), o["grad"].copy(), p0, u, eps, Ls)
    np.testing.assert_allclose(hm["h_prop"], hp, rtol=2e-3, atol=2e-2)
    rate = np.minimum(np.exp(np.minimum(hc - hp, 0.0)), 1)
    decided = np.abs(u - rate) > 2e-3
    np.testing.assert_array_equal(hm["accepted"][decided], acc[decided])
    if ops != "all":
        return
    co64 = _f64_oracle(co, dims, acts, lik)
    f8 = lambda a_: np.asarray(a_, dtype=np.float64).copy()
    ml = _np(rep.both("mala_step", _mala(pl, 2e-4), th, vg["target"], vg["grad"], p0_t, u_t))
    _check_log_rate(ml, *co64.mala_draw(f8(th0), f8(o["target"]), f8(o["grad"]), f8(p0), f8(u), 2e-4), u, "f32")
    mh = _np(rep.both("mh_step", _mh(pl, 4e-3), th, vg["target"], p0_t, u_t))
    _check_log_rate(mh, *co64.mh_draw(f8(th0), f8(o["target"]), f8(p0), f8(u), 4e-3), u, "f32")


@pytest.mark.gpu
def test_mfma32_philox_blocks_are_the_big_launch_rows():
    pl, _, _ = _mfma32_setup(HEADLINE, 33, "bf16x3", "uniform")
    assert pl.kernel == "mfma32"
    n_cu = _n_cu()
    C = chains_for(n_cu, 8)
    _philox_blocks(pl, C, min(C, n_cu), 8, "hmc", 0.03, 3)


# ------------------------------------------------------------------------------------------------ mid kernels
MID_CASES = [
    # dims, activations, variant that selects the kernel, kernel (k_mid32<NB0>: NB0 = 2 with more than 32 inputs, ey_mid32_eval)
    ([16, 32, 32, 32, 3], [1, 1, 1, 0], 0, "k_mid32_nb1"),
    ([64, 32, 32, 10], [1, 1, 0], 0, "k_mid32_nb2"),
    ([20, 100, 100, 5], [1, 1, 0], 8192, "k_mid"),
]


def _mid_setup(dims, acts, N):
    from eeyore_amd.plan import Plan
    rng = np.random.default_rng(sum(dims) + N)
    x = rng.standard_normal((N, dims[0])).astype(np.float32)
    y = np.eye(dims[-1], dtype=np.float32)[rng.integers(0, dims[-1], N)]
    pl = Plan(dims, [1] * (len(dims) - 1), acts, 1, torch.float32, DEV)
    pl.set_data(_t(x, torch.float32), _t(y, torch.float32))
    mu = (0.1 * rng.standard_normal(pl.P)).astype(np.float32)
    sg = (1.0 + rng.random(pl.P)).astype(np.float32)
    pl.set_prior(torch.tensor(mu), torch.tensor(sg))
    co = COracle(dims, acts, 1, x.astype(np.float64), y, mu.astype(np.float64), sg.astype(np.float64), dtype=np.float64,
                 nthreads=4)
    return pl, co, rng


@pytest.mark.gpu
@pytest.mark.parametrize("case", MID_CASES, ids=lambda c: c[3] + "-" + "x".join(map(str, c[0])))
def test_mid_kernels_every_workgroup_and_round(case):
    """A workgroup is the unit of k_mid32 / k_mid: grid = min(C, n_cu), chain = blockIdx.x, + gridDim.x, ...; k_mid32 fetches the
    next round's parameters during the current chain.  Tiled replicas of value + gradient (per-chain temperature), an HMC and
    a MALA draw on recorded randomness; replica 0 against the f64 oracle and against the layerwise launches (variant bit 14)
    at the tolerances of test_fused_narrow_deep_kernel_* / test_fused_midsize_kernel_* of tests/test_gpu_parity.py."""
    dims, acts, variant, kernel = case
    N = 33
    pl, co, rng = _mid_setup(dims, acts, N)
    assert pl.kernel == "bgemm"   # the family the mid kernels evaluate for
    n_cu = _n_cu()
    C = chains_for(n_cu, 1)
    grid = min(C, n_cu)
    check_coverage(C, grid, 1)
    rep = Replicas(C, grid, 1)
    dt, P = torch.float32, pl.P
    th = (0.4 * pl.philox_normal(B, seed=5, it=0)).contiguous()
    p0_t = pl.philox_normal(B, seed=5, it=1)
    u_t = pl.philox_uniform(B, seed=5, it=1)
    temps = torch.linspace(0.3, 1.0, B, device=DEV)
    res = {}
    try:
        pl.set_variant(variant)
        vg = rep.both(f"{kernel} log_target_grad", _value_grad(pl), th, temps)
        hm = rep.both(f"{kernel} hmc_step", _hmc(pl, 0.004, 3), th, vg["target"], vg["grad"], p0_t, u_t, temps)
        ml = rep.both(f"{kernel} mala_step", _mala(pl, 0.002), th, vg["target"], vg["grad"], p0_t, u_t)
        res["mid"] = (_np(vg), _np(hm), _np(ml))
        pl.set_variant(16384)   # the layerwise launches, on the 11 base chains
        vg2 = _value_grad(pl)(th.clone(), temps)
        hm2 = _hmc(pl, 0.004, 3)(th.clone(), vg["target"].clone(), vg["grad"].clone(), p0_t, u_t, temps)
        ml2 = _mala(pl, 0.002)(th.clone(), vg["target"].clone(), vg["grad"].clone(), p0_t, u_t)
        res["layerwise"] = (_np(vg2), _np(hm2), _np(ml2))
    finally:
        pl.set_variant(0)
    a, b = res["mid"], res["layerwise"]
    assert not np.array_equal(a[0]["grad"], b[0]["grad"])  # two different kernels (not the same launch twice)
    thn = th.cpu().numpy().astype(np.float64)
    for c in range(B):
        co.temp = float(temps[c].item())
        to, go, _, _ = co.log_target_grad(thn[c])
        for r in (a, b):
            np.testing.assert_allclose(r[0]["target"][c], to, rtol=2e-5, atol=2e-3)
            np.testing.assert_allclose(r[0]["grad"][c], go, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(go).max()))
    np.testing.assert_allclose(b[0]["target"], a[0]["target"], rtol=2e-5, atol=2e-3)
    un = u_t.cpu().numpy()
    np.testing.assert_allclose(b[1]["h_prop"], a[1]["h_prop"], rtol=1e-4, atol=2e-2)
    decided = np.abs(un - a[1]["rate"]) > 2e-3
    np.testing.assert_array_equal(a[1]["accepted"][decided], b[1]["accepted"][decided])
    same = a[1]["accepted"] == b[1]["accepted"]
    np.testing.assert_allclose(b[1]["theta"][same], a[1]["theta"][same], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(b[2]["log_rate"], a[2]["log_rate"], rtol=1e-3, atol=2e-2)
    decided = np.abs(np.log(un.astype(np.float64)) - a[2]["log_rate"]) > 2e-3 * np.maximum(1.0, np.abs(a[2]["log_rate"]))
    np.testing.assert_array_equal(a[2]["accepted"][decided], b[2]["accepted"][decided])


@pytest.mark.gpu
def test_mid32_philox_blocks_are_the_big_launch_rows():
    dims, acts, _, _ = MID_CASES[0]
    pl, _, _ = _mid_setup(dims, acts, 33)
    assert pl.kernel == "bgemm"
    n_cu = _n_cu()
    C = chains_for(n_cu, 1)
    _philox_blocks(pl, C, min(C, n_cu), 1, "hmc", 0.01, 3)
