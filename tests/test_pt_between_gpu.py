"""The between-chain move on the device (ey_pt_between, k_pt_between in eeyore_amd/csrc/ey_pt.hip) against the host path of
PowerPosteriorSampler and the numpy restatement (tests/pt_restatement.py), and the sampler's device run loop against
draw by draw.

Decisions are compared on tables chosen so that every step of the f64 restatement has the margin
|log u - log_rate| > 1e-3 max(1, |log_rate|) (``_decided_tables``): with it, the last bits of ``log`` cannot turn a decision,
and every later state is comparable bit for bit."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

from tests import pt_restatement as pr
from tests.helpers import load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {torch.float32: np.float32, torch.float64: np.float64}
RTOL = {torch.float32: 1e-5, torch.float64: 1e-12}   # log rates: tests/test_power_posterior.py's f32 tolerance, and f64's


def _partner_q(K, b=0.5):
    """PowerPosteriorSampler._partner_matrix for K temperatures: weights exp(-b |i - j|), rows normalised."""
    d = np.abs(np.arange(K)[:, None] - np.arange(K)[None, :]).astype(np.float64)
    w = np.exp(-b * d)
    np.fill_diagonal(w, 0.0)
    q = w / w.sum(1, keepdims=True)
    np.fill_diagonal(q, 1.0)
    return q


def _ladders(K, dtype):
    from eeyore_amd.plan import PtLadder
    t = [(i / K) ** 4 for i in range(1, K + 1)]
    q = _partner_q(K)
    return PtLadder(t, q, dtype, DEV), pr.Ladder(t, q, NP[dtype]), pr.Ladder(t, q, np.float64)


def _tables(K, R, seed, dtype):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, K - 1, size=(K, R))
    partners = np.where(k < np.arange(K)[:, None], k, k + 1).astype(np.int32)
    return partners, rng.random((K, R)).astype(NP[dtype])


def _decided_tables(ld64, theta, target, grad, partners, u):
    """Halve the accept variate of every step that misses the margin in the f64 restatement until none does (a step's
    state depends on the steps before it, so the restatement runs again after every change)."""
    f64 = [None if a is None else np.asarray(a, np.float64) for a in (theta, target, grad)]
    for _ in range(64):
        out = pr.between(ld64, *f64, partners=partners, u=u.astype(np.float64))
        bad = ~pr.decided(out)
        if not bad.any():
            return u
        u = np.where(bad, u * u.dtype.type(0.5), u)
    raise AssertionError("no table with the margin at every step")


def _synthetic(K, R, P, dtype, seed, grad=True):
    """theta, tempered target and gradient rows [K*R, ...] that are all distinct: ell ~ N(-60, 15), target = t ell."""
    rng = np.random.default_rng(seed)
    T = NP[dtype]
    t = np.array([(i / K) ** 4 for i in range(1, K + 1)])
    theta = rng.standard_normal((K * R, P)).astype(T)
    target = (np.repeat(t, R) * (-60.0 + 15.0 * rng.standard_normal(K * R))).astype(T)
    g = rng.standard_normal((K * R, P)).astype(T) if grad else None
    return theta, target, g


def _dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV).contiguous()


def _same_bits(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), \
        (what, int((got != want).sum()), float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64)))))


def _against_restatement(K, R, P, dtype, grad, seed):
    from eeyore_amd.plan import pt_between
    dev_ld, ld, ld64 = _ladders(K, dtype)
    theta, target, g = _synthetic(K, R, P, dtype, seed, grad)
    partners, u = _tables(K, R, seed + 1, dtype)
    u = _decided_tables(ld64, theta, target, g, partners, u)
    want = pr.between(ld, theta, target, g, partners=partners, u=u)
    th, tg, gr = _dev(theta), _dev(target), _dev(g)
    rec_th, rec_tg = th.clone(), torch.zeros_like(tg)
    out = pt_between(dev_ld, th, tg, gr, partners=_dev(partners), u=_dev(u), rec_theta=rec_th, rec_target=rec_tg)
    assert np.array_equal(out["swap"].cpu().numpy(), want["swap"])
    if K * R >= 15:
        assert 0 < int(want["swap"].sum()) < K * R       # the tables mix exchanges and refusals
    assert np.array_equal(out["partners"].cpu().numpy(), partners) and np.array_equal(out["u"].cpu().numpy(), u)
    np.testing.assert_allclose(out["log_rate"].cpu().numpy(), want["log_rate"], rtol=RTOL[dtype])
    _same_bits(th, want["theta"], "theta")
    _same_bits(tg, want["target"], "target")     # one division and one multiplication per exchange on both sides
    if grad:
        _same_bits(gr, want["grad"], "grad")
    assert torch.equal(rec_th, th) and torch.equal(rec_tg, tg)   # the record of the draw holds the state after the move


# ------------------------------------------------------------------------------------------------ 7: against the host path
def _sampler(dtype, name, K, R, between_step=1000, seed=5, **kw):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import PowerPosteriorSampler
    z = load("g6_power_posterior.npz")
    hp = mlp.Hyperparameters(dims=[2, 3, 2, 1], bias=3 * [True], activations=3 * [torch.sigmoid])
    m = mlp.MLP(loss=loss_functions['binary_classification'], hparams=hp, dtype=dtype, device=DEV)
    m.prior = Normal(torch.tensor(z["prior_mu"], dtype=dtype, device=DEV), torch.tensor(z["prior_sigma"], dtype=dtype, device=DEV))
    ds = XYDataset(torch.tensor(z["x"], dtype=dtype, device=DEV), torch.tensor(z["y"], dtype=dtype, device=DEV))
    loader = DataLoader(ds, batch_size=len(ds), shuffle=False)
    th0 = 0.5 * torch.randn(R, 20, dtype=dtype, generator=torch.Generator().manual_seed(seed))
    args = {'MALA': {'step': 0.1}, 'HMC': {'step': 0.1, 'num_steps': 3}, 'MetropolisHastings': {}}[name]
    s = PowerPosteriorSampler(m, loader, [[name, dict(args)] for _ in range(K)], theta0=th0.to(DEV),
                              between_step=between_step, b=0.5, rng='philox', seed=3, **kw)
    return m, ds, s


@pytest.mark.parametrize("name", ["MALA", "MetropolisHastings"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_given_variates_against_the_host_path(dtype, name):
    """K = 5, R = 5 (the second workgroup holds one replica).  target and grad are compared bit for bit: the host path
    and the kernel both do one division (t_i / t_j) and one multiplication per element, uncontracted."""
    K, R = 5, 5
    m, ds, s = _sampler(dtype, name, K, R)
    w = s.sampler
    start = 0.5 * torch.randn(K * R, 20, dtype=dtype, generator=torch.Generator().manual_seed(8))
    w.set_current(start.to(DEV), data=(ds.x, ds.y))      # one state per chain: every exchange moves something
    for _ in range(3):
        s.within_chain_moves(ds.x, ds.y)
    has_grad = hasattr(w, '_grad')
    th, tg, gr = w._theta.clone(), w._target.clone(), w._grad.clone() if has_grad else None
    partners, u = _tables(K, R, 21, dtype)
    ld64 = pr.Ladder(s.temperature, s._partner_matrix(), np.float64)
    u = _decided_tables(ld64, th.cpu().numpy(), tg.cpu().numpy(), gr.cpu().numpy() if has_grad else None, partners, u)
    steps = iter(range(K))
    s._sample_partners = lambda i: torch.as_tensor(partners[i].astype(np.int64)).to(DEV)
    s._rand = lambda n: torch.as_tensor(u[next(steps)]).to(DEV)
    s.between_chain_moves(ds.x, ds.y)
    host_swap = torch.stack([sw for _, sw, _ in s.last_swaps])
    host_rate = torch.stack([lr for _, _, lr in s.last_swaps])
    plan = m._plan(ds.x, ds.y)
    out = plan.pt_between(plan.pt_ladder(s.temperature, s._partner_matrix()), th, tg, gr, partners=_dev(partners), u=_dev(u))
    assert 0 < int(host_swap.sum()) < K * R
    assert torch.equal(out["swap"], host_swap)
    assert torch.equal(th, w._theta)
    np.testing.assert_allclose(out["log_rate"].cpu().numpy(), host_rate.cpu().numpy(), rtol=RTOL[dtype])
    _same_bits(tg, w._target.cpu().numpy(), "target")
    if has_grad:
        _same_bits(gr, w._grad.cpu().numpy(), "grad")


# ------------------------------------------------------------------------------------------------ 8: the Philox path
@pytest.mark.parametrize("K", [5, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_philox_path(dtype, K):
    from eeyore_amd.plan import pt_between
    R, P, seed, it, off = 37, 20, 11, 6, 1000
    dev_ld, ld, _ = _ladders(K, dtype)
    theta, target, g = _synthetic(K, R, P, dtype, 2)
    for offset in (0, off):
        v, u = pr.variates(K, R, seed, it, offset, NP[dtype])
        partners = np.stack([pr.draw_partners(ld.cdf[i], v[i], i) for i in range(K)])
        th, tg, gr = _dev(theta), _dev(target), _dev(g)
        out = pt_between(dev_ld, th, tg, gr, seed=seed, it=it, replica_offset=offset)
        assert np.array_equal(out["partners"].cpu().numpy(), partners)
        _same_bits(out["u"], u, "u")
        # the explicit path fed with them: the same bits in every output and state
        th2, tg2, gr2 = _dev(theta), _dev(target), _dev(g)
        out2 = pt_between(dev_ld, th2, tg2, gr2, partners=out["partners"], u=out["u"])
        for key in out:
            assert torch.equal(out[key].view(torch.uint8), out2[key].view(torch.uint8)), key
        assert torch.equal(th, th2) and torch.equal(tg, tg2) and torch.equal(gr, gr2)
        assert 0 < int(out["swap"].sum()) < K * R
    # replicas 10 .. 19 alone, with replica_offset, are rows 10 .. 19 of the big call
    rows = (np.arange(K)[:, None] * R + np.arange(10, 20)[None, :]).reshape(-1)
    big = [_dev(theta), _dev(target), _dev(g)]
    out_big = pt_between(dev_ld, *big, seed=seed, it=it, replica_offset=off)
    part = [_dev(theta[rows]), _dev(target[rows]), _dev(g[rows])]
    out_part = pt_between(dev_ld, *part, seed=seed, it=it, replica_offset=off + 10)
    for a, b in zip(big, part):
        assert torch.equal(a[torch.as_tensor(rows, device=DEV)], b)
    for key in out_big:
        assert torch.equal(out_big[key][:, 10:20].contiguous().view(torch.uint8), out_part[key].view(torch.uint8)), key
    # another iteration draws other variates
    other = pt_between(dev_ld, _dev(theta), _dev(target), _dev(g), seed=seed, it=it + 1, replica_offset=off)
    assert not torch.equal(other["u"], out_big["u"])


# ------------------------------------------------------------------------------------------------ 9: shapes
SHAPES = [  # (K, R, P, grad): every P, K and R of interest at least once; PT_WAVES = 4 replicas per workgroup
    (2, 1, 1, True),
    (5, 3, 63, True),
    (5, 5, 64, False),
    (5, 257, 65, True),
    (2, 4, 1315, True),
    (5, 1, 1315, False),
    (pr.PT_KMAX, 3, 1, True),
    (pr.PT_KMAX, 5, 65, False),
]


@pytest.mark.parametrize("K,R,P,grad", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_shapes_against_the_restatement(dtype, K, R, P, grad):
    _against_restatement(K, R, P, dtype, grad, seed=100 + K + R + P)


def test_a_ladder_beyond_the_limit_is_refused():
    from eeyore_amd.plan import PtLadder
    K = pr.PT_KMAX + 1
    with pytest.raises(RuntimeError, match="temperatures"):
        PtLadder([1.0] * K, np.ones((K, K)), torch.float32, DEV)


@pytest.mark.parametrize("K,R,P,grad", [(5, 5, 65, True), (64, 3, 7, False)])
def test_all_accepting_variates_permute_the_rows_of_each_replica(K, R, P, grad):
    from eeyore_amd.plan import pt_between
    dtype = torch.float64
    dev_ld, ld, _ = _ladders(K, dtype)
    theta, target, g = _synthetic(K, R, P, dtype, 7, grad)
    partners, _ = _tables(K, R, 8, dtype)
    u = np.full((K, R), 1e-300)                      # log u = -690: every exchange is accepted
    th, tg, gr = _dev(theta), _dev(target), _dev(g)
    out = pt_between(dev_ld, th, tg, gr, partners=_dev(partners), u=_dev(u))
    assert bool(out["swap"].all())
    after = th.cpu().numpy().reshape(K, R, P)
    before = theta.reshape(K, R, P)
    for r in range(R):   # states move between temperatures within a replica, never across replicas
        assert sorted(map(tuple, before[:, r])) == sorted(map(tuple, after[:, r]))
    assert not np.array_equal(before, after)
    # the untempered target travels with its state: ell = target / t is permuted the same way (to rounding)
    ell_b = (target.reshape(K, R) / ld.t[:, None])
    ell_a = (tg.cpu().numpy().reshape(K, R) / ld.t[:, None])
    for r in range(R):
        order = [int(np.flatnonzero((before[:, r] == after[k, r]).all(1))[0]) for k in range(K)]
        np.testing.assert_allclose(ell_a[:, r], ell_b[order, r], rtol=1e-12)


@pytest.mark.parametrize("grad", [True, False])
def test_a_bad_partner_exchanges_nothing(grad):
    from eeyore_amd.plan import pt_between
    K, R, P, dtype = 5, 6, 65, torch.float32
    dev_ld, ld, _ = _ladders(K, dtype)
    theta, target, g = _synthetic(K, R, P, dtype, 9, grad)
    partners = np.empty((K, R), np.int32)
    partners[:, 0] = np.arange(K)                     # itself
    partners[:, 1:] = np.array([-1, K, K + 1000, 2 ** 31 - 1, -2 ** 31], np.int32)[None, :]
    u = np.full((K, R), 1e-30, np.float32)            # would accept anything
    th, tg, gr = _dev(theta), _dev(target), _dev(g)
    out = pt_between(dev_ld, th, tg, gr, partners=_dev(partners), u=_dev(u))
    assert not bool(out["swap"].any()) and bool(torch.isnan(out["log_rate"]).all())
    _same_bits(th, theta, "theta")
    _same_bits(tg, target, "target")
    if grad:
        _same_bits(gr, g, "grad")
    with pytest.raises(ValueError, match="together"):
        pt_between(dev_ld, th, tg, gr, partners=_dev(partners))


# ------------------------------------------------------------------------------------------------ 10, 11: the run loop
KEYS = ['sample', 'target_val', 'accepted']


def _run(dtype, name, fused_block, iters=13, burnin=4, prepare=None):
    m, ds, s = _sampler(dtype, name, 5, 6, between_step=3, between='device', keys=KEYS, replica_offset=2)
    s.sampler.fused_block = fused_block
    if prepare is not None:
        prepare(s)
    s.run(num_epochs=iters, num_burnin_epochs=burnin)
    return m, ds, s


@pytest.mark.parametrize("name", ["MALA", "HMC"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_fused_run_equals_draw_by_draw(dtype, name):
    m, ds, ref = _run(dtype, name, 0)
    assert not ref.sampler._can_fuse(False)
    assert ref._backing.n == 9
    for fb in (256, 2):
        m2, ds2, s = _run(dtype, name, fb)
        assert s.sampler._can_fuse(False) and s.counter.idx == 13 and s.sampler._iter == 13
        for key in KEYS:
            a, b = s._backing.bufs[key][:9], ref._backing.bufs[key][:9]
            assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (fb, key)
        for a, b in ((s.sampler._theta, ref.sampler._theta), (s.sampler._target, ref.sampler._target),
                     (s.sampler._grad, ref.sampler._grad)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), fb
        for k in range(5):
            assert s.get_chain(k).get_samples().shape == (9, 6, 20)
            assert torch.equal(s.get_chain(k).get_accepted(), ref.get_chain(k).get_accepted())
    if dtype == torch.float64:   # the tolerances of test_power_posterior_on_gpu_with_hip_decide_kernel
        plan = m2._plan(ds2.x, ds2.y)
        t, g = plan.log_target_grad(s.sampler._theta.clone(), temp=s._tvec)
        np.testing.assert_allclose(s.sampler._target.cpu().numpy(), t.cpu().numpy(), rtol=1e-9)
        np.testing.assert_allclose(s.sampler._grad.cpu().numpy(), g.cpu().numpy(), rtol=1e-8, atol=1e-10)


def test_the_record_of_a_between_draw_is_the_state_after_its_exchange():
    """13 draws, 4 of them burn-in, a move behind draws 0, 3, 6, 9, 12.  When the move of a recorded draw starts, the
    draw's record holds the state the within-chain launch left; afterwards it holds the state after the exchange, which
    moved rows.  A run that stops behind draw d is left in exactly the state the long run recorded for d."""
    dtype = torch.float64
    m, ds, full = _run(dtype, "MALA", 256)
    moved = 0
    for d in (6, 9, 12):
        seen = []

        def prepare(s):
            inner = s._between_on_device

            def spy(x, y, rec_theta=None, rec_target=None):
                seen.append((s.counter.idx, s.sampler._theta.clone(), None if rec_theta is None else rec_theta.clone()))
                return inner(x, y, rec_theta=rec_theta, rec_target=rec_target)
            s._between_on_device = spy

        m2, ds2, s = _run(dtype, "MALA", 256, iters=d + 1, prepare=prepare)
        assert [idx for idx, _, _ in seen] == list(range(0, d + 1, 3))
        assert all((rec is None) == (idx < 4) for idx, _, rec in seen)      # burn-in moves have no record to mend
        idx, before, rec_before = seen[-1]
        swaps = torch.stack([sw for _, sw, _ in s.last_swaps])
        moved += int(swaps.sum())
        row = d - 4
        assert torch.equal(rec_before, before)
        assert torch.equal(s._backing.bufs['sample'][row], s.sampler._theta)
        assert torch.equal(s._backing.bufs['target_val'][row], s.sampler._target)
        assert torch.equal(full._backing.bufs['sample'][row], s.sampler._theta), d
        assert torch.equal(full._backing.bufs['target_val'][row], s.sampler._target), d
        assert torch.equal(before, s.sampler._theta) == (int(swaps.sum()) == 0)
    assert moved > 0
