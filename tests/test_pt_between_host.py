"""PowerPosteriorSampler(between='device') without a GPU: the numpy restatement of the between-chain move
(tests/pt_restatement.py) against the host path, its partner draws, the C ABI's host-side validation, the segment
function of the device run loop, and the sampler itself on the oracle test double."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import Normal
from torch.utils.data import DataLoader

from eeyore_amd import _lib as L
from eeyore_amd.chains import ChainBuffer, ChainBufferView
from eeyore_amd.constants import loss_functions
from eeyore_amd.datasets import XYDataset
from eeyore_amd.models import mlp
from eeyore_amd.samplers import PowerPosteriorSampler
from eeyore_amd.samplers.power_posterior_sampler import pt_segments
from tests import pt_restatement as pr
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(R=4, K=5, between_step=1, seed=5, **kw):
    z = load("g6_power_posterior.npz")
    dt = torch.float64
    hp = mlp.Hyperparameters(dims=[2, 3, 2, 1], bias=3 * [True], activations=3 * [torch.sigmoid])
    m = mlp.MLP(loss=loss_functions['binary_classification'], hparams=hp, dtype=dt, device="cpu")
    m.prior = Normal(torch.tensor(z["prior_mu"], dtype=dt), torch.tensor(z["prior_sigma"], dtype=dt))
    pr.attach_pt(m)
    ds = XYDataset(torch.tensor(z["x"], dtype=dt), torch.tensor(z["y"], dtype=dt))
    loader = DataLoader(ds, batch_size=len(ds), shuffle=False)
    torch.manual_seed(seed)
    th0 = 0.5 * torch.randn(R, 20, dtype=dt)
    s = PowerPosteriorSampler(m, loader, [['MALA', {'step': 0.1}] for _ in range(K)], theta0=th0,
                              between_step=between_step, b=0.5, rng='torch', **kw)
    return m, ds, s


def _ladder(s, dtype=np.float64):
    return pr.Ladder(s.temperature, s._partner_matrix(), dtype)


def _tables(K, R, seed):
    """Seeded partner and accept-variate tables [K, R]: partners uniform over the others, u uniform."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, K - 1, size=(K, R))
    partners = np.where(k < np.arange(K)[:, None], k, k + 1).astype(np.int32)
    return partners, rng.random((K, R))


def test_restatement_reproduces_the_host_path():
    K, R = 5, 4
    m, ds, s = _setup(R=R, K=K, between_step=1000)
    for _ in range(3):
        s.within_chain_moves(ds.x, ds.y)
    w = s.sampler
    theta, target, grad = w._theta.numpy().copy(), w._target.numpy().copy(), w._grad.numpy().copy()
    partners, u = _tables(K, R, seed=17)
    steps = iter(range(K))
    s._sample_partners = lambda i: torch.as_tensor(partners[i].astype(np.int64))
    s._rand = lambda n: torch.as_tensor(u[next(steps)])
    s.between_chain_moves(ds.x, ds.y)
    out = pr.between(_ladder(s), theta, target, grad, partners=partners, u=u)
    host_swap = np.stack([sw.numpy() for _, sw, _ in s.last_swaps])
    host_rate = np.stack([lr.numpy() for _, _, lr in s.last_swaps])
    assert 0 < host_swap.sum() < K * R                      # the tables mix exchanges and refusals
    assert np.array_equal(out["swap"], host_swap)
    assert np.array_equal(out["theta"], w._theta.numpy())
    assert not np.array_equal(out["theta"], theta)
    np.testing.assert_allclose(out["log_rate"], host_rate, rtol=1e-12)
    np.testing.assert_allclose(out["target"], w._target.numpy(), rtol=1e-12)
    np.testing.assert_allclose(out["grad"], w._grad.numpy(), rtol=1e-12)


def test_partner_draws_of_the_restatement():
    K, R = 5, 20000
    m, ds, s = _setup(R=1, K=K)
    Q, ld = s._partner_matrix(), _ladder(s)
    v, u = pr.variates(K, R, seed=4, it=9, replica_offset=3)
    assert v.shape == u.shape == (K, R) and (0 <= v).all() and (v < 1).all() and (0 <= u).all() and (u < 1).all()
    for i in range(K):
        j = pr.draw_partners(ld.cdf[i], v[i], i)
        assert ((j >= 0) & (j < K) & (j != i)).all()
        freq = np.bincount(j, minlength=K) / R
        for other in range(K):
            if other != i:
                sd = np.sqrt(Q[i, other] * (1 - Q[i, other]) / R)
                assert abs(freq[other] - Q[i, other]) < 4 * sd, (i, other, freq[other], Q[i, other])
        # v in the gap between the rounded total and 1 goes to the last index that is not i
        last = K - 2 if i == K - 1 else K - 1
        beyond = np.array([np.nextafter(ld.cdf[i, -1], 2.0), 1.0 - 2.0 ** -53, 5.0])
        assert (pr.draw_partners(ld.cdf[i], beyond, i) == last).all()
        # ... and the first index takes v = 0 (index 1 for chain 0, whose own slot adds nothing)
        assert pr.draw_partners(ld.cdf[i], np.array([0.0]), i)[0] == (1 if i == 0 else 0)
    # the f32 accept variate is the 24-bit conversion of word 2; the partner variate does not depend on the dtype
    v32, u32 = pr.variates(K, 64, seed=4, it=9, replica_offset=3, dtype=np.float32)
    assert np.array_equal(v32, v[:, :64]) and u32.dtype == np.float32
    # a replica's variates depend on (seed, replica_offset + r, it) alone
    v2, u2 = pr.variates(K, 10, seed=4, it=9, replica_offset=13)
    assert np.array_equal(v2, v[:, 10:20]) and np.array_equal(u2, u[:, 10:20])


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ey_pt_ladder_create", "ey_pt_ladder_destroy", "ey_pt_between"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name), name


def _create(t, q, dtype=L.EY_F64):
    K = len(t)
    h = ct.c_void_p()
    rc = L.lib().ey_pt_ladder_create((ct.c_double * max(K, 1))(*t), (ct.c_double * max(K * K, 1))(*np.ravel(q).tolist()), K,
                                     dtype, ct.byref(h))
    return rc, L.lib().ey_last_error().decode(), h


_Q3 = [[0, 1, 1], [1, 0, 1], [1, 1, 0]]


@pytest.mark.parametrize("t,q,msg", [
    ([1.0], [[0.0]], "at least two"),
    ([0.5, float("nan"), 1.0], _Q3, "temperature 1"),
    ([0.5, float("inf"), 1.0], _Q3, "temperature 1"),
    ([0.5, 0.0, 1.0], _Q3, "temperature 1"),
    ([-0.5, 0.7, 1.0], _Q3, "temperature 0"),
    ([0.2, 0.5, 1.0], [[0, 1, 1], [1, 0, -0.1], [1, 1, 0]], "q[1,2]"),
    ([0.2, 0.5, 1.0], [[0, 1, 1], [1, 0, float("nan")], [1, 1, 0]], "q[1,2]"),
    ([0.2, 0.5, 1.0], [[0, 1, 1], [1, 0, 1], [0, 0, 7]], "row 2"),
    ([0.2, 0.5, 1.0], [[0, 1, float("inf")], [1, 0, 1], [1, 1, 0]], "row 0"),
])
def test_ladder_validation_fails_before_any_device_call(t, q, msg):
    rc, err, h = _create(t, q)
    assert rc == -1 and msg in err and not h.value, (rc, err)


def test_c_abi_argument_errors_without_gpu():
    lib = L.lib()
    p = ct.c_void_p(1)
    h = ct.c_void_p()
    assert lib.ey_pt_ladder_create(None, None, 3, L.EY_F64, ct.byref(h)) == -1
    assert lib.ey_pt_ladder_create((ct.c_double * 2)(0.5, 1.0), (ct.c_double * 4)(0, 1, 1, 0), 2, 7, ct.byref(h)) == -1
    assert b"dtype" in lib.ey_last_error()
    big = pr.PT_KMAX + 1   # beyond the kernel's limit: refused as unsupported, still on the host
    assert lib.ey_pt_ladder_create((ct.c_double * big)(*([1.0] * big)), (ct.c_double * (big * big))(*([1.0] * (big * big))),
                                   big, L.EY_F64, ct.byref(h)) == -2 and not h.value
    assert lib.ey_pt_between(None, p, p, None, 1, 1, None, None, 0, 0, 0, None, None, None, None, None, None, None) == -1
    assert b"null ladder" in lib.ey_last_error()
    assert lib.ey_pt_ladder_destroy(None) == 0


def _walk(idx, num_iters, burnin, between_step, fused_block):
    """The segments by brute force: one draw at a time, closing the block behind a between-draw, before the burn-in
    boundary, when it is full, and at the end."""
    out, first = [], idx
    for d in range(idx, num_iters):
        between = d % between_step == 0
        if between or d + 1 == burnin or d + 1 - first == fused_block or d + 1 == num_iters:
            out.append((first, d + 1 - first, between))
            first = d + 1
    return out


@pytest.mark.parametrize("between_step", [1, 3, 10, 1000])
@pytest.mark.parametrize("burnin", [0, 4, 10])
@pytest.mark.parametrize("fused_block", [1, 2, 256])
def test_segments_against_a_brute_force_walk(between_step, burnin, fused_block):
    for idx, num_iters in ((0, 37), (5, 37), (0, 1), (12, 12), (0, 600)):
        segs = pt_segments(idx, num_iters, burnin, between_step, fused_block)
        assert segs == _walk(idx, num_iters, burnin, between_step, fused_block)
        covered = [d for first, count, _ in segs for d in range(first, first + count)]
        assert covered == list(range(idx, num_iters))                      # every draw once, in order
        for first, count, between in segs:
            assert 1 <= count <= fused_block
            inner = range(first, first + count - 1)
            assert not any(d % between_step == 0 for d in inner)           # a between-draw only ever ends a block
            assert between == ((first + count - 1) % between_step == 0)
            assert first >= burnin or first + count <= burnin              # recorded as a whole or not at all


def test_sampler_on_the_device_path_with_the_test_double():
    K, R, P = 5, 6, 20
    m, ds, s = _setup(R=R, K=K, between_step=3, between='device', seed=5, replica_offset=7)
    plan = m._plan(ds.x, ds.y)
    w = s.sampler
    assert w.chain is s._backing and not w._can_fuse(False)          # rng='torch': draw by draw
    # every move is ONE pt_between on the state the within-chain move left, keyed by the draw's index
    seen = []
    inner = plan.pt_between

    def spy(ladder, theta, target, grad=None, **kw):
        want = pr.between(ladder, theta.numpy(), target.numpy(), grad.numpy(), seed=kw["seed"], it=kw["it"],
                          replica_offset=kw["replica_offset"])
        out = inner(ladder, theta, target, grad, **kw)
        assert np.array_equal(theta.numpy(), want["theta"]) and np.array_equal(target.numpy(), want["target"])
        assert np.array_equal(grad.numpy(), want["grad"]) and np.array_equal(out["swap"].numpy(), want["swap"])
        seen.append((kw["seed"], kw["it"], kw["replica_offset"], int(want["swap"].sum())))
        return out

    plan.pt_between = spy
    s.run(num_epochs=25, num_burnin_epochs=5)
    assert [(a, b, c) for a, b, c, _ in seen] == [(0, it, 7) for it in range(0, 25, 3)]
    assert sum(n for *_, n in seen) > 0                                # exchanges did happen
    assert len(s.last_swaps) == K and all(j.shape == sw.shape == lr.shape == (R,) for j, sw, lr in s.last_swaps)
    # the chains are views of ONE backing buffer
    assert isinstance(s._backing, ChainBuffer) and s._backing.get_samples().shape == (20, K * R, P)
    for k in range(K):
        chain = s.get_chain(k)
        assert isinstance(chain, ChainBufferView) and len(chain) == 20
        assert chain.get_samples().shape == (20, R, P) and chain.get_target_vals().shape == (20, R)
        assert chain.get_samples().data_ptr() == s._backing.get_samples()[:, k * R:].data_ptr()
        assert torch.equal(chain.get_samples(), s._backing.get_samples()[:, k * R:(k + 1) * R])
        assert chain.num_chains() == R and chain.num_params() == P and chain.mean().shape == (R, P)
        assert len(chain.get_chain(1).vals['sample']) == 20
        with pytest.raises(RuntimeError, match="records nothing"):
            chain.update({})
    assert s.get_chain() is s.chains[K - 1]
    assert s.get_param(4).shape == (20, R) and s.get_sample(2, chain_idx=1).shape == (R, P)
    assert torch.equal(s.get_chain().get_samples()[-1], w._theta[(K - 1) * R:])   # the last draw (24) had its move before it was saved
    # after all the exchanges the cached tempered target / gradient equal a fresh evaluation
    t, g = plan.log_target_grad(w._theta.clone(), temp=s._tvec)
    np.testing.assert_allclose(w._target.numpy(), t.numpy(), rtol=1e-9)
    np.testing.assert_allclose(w._grad.numpy(), g.numpy(), rtol=1e-8, atol=1e-10)
    s.reset_chains()
    assert all(len(s.get_chain(k)) == 0 for k in range(K)) and len(s._backing) == 0
    with pytest.raises(ValueError, match="between"):
        _setup(between='tape')


def test_device_path_keeps_file_storage_and_the_host_default(tmp_path):
    m, ds, s = _setup(R=2, K=3, between_step=2, between='device', storage='file', path=tmp_path, mode='a')
    assert s._backing is None
    s.run(num_epochs=5, num_burnin_epochs=1)
    from eeyore_amd.chains import ChainFile
    for i in range(3):
        for r in range(2):
            cl = ChainFile(keys=['sample', 'target_val'], path=tmp_path / f"chain{i + 1}" / f"replica{r + 1}", mode='a').to_chainlist()
            assert len(cl.vals['sample']) == 4
    m2, ds2, host = _setup(R=2, K=3)
    assert host.between == 'host' and host._backing is None and type(host.chains[0]) is ChainBuffer
