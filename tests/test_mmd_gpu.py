"""ey_kernel_pair_sums / stats.batched.mmd_chains / ChainBuffer.mmd on the GPU: against the reference's numbers
(tests/golden/g15_mmd.npz) and the numpy restatement (tests/mmd_restatement.py) within the bound derived there, at every size
at which the kernel takes another path: its tile edge (64 rows) and column chunk (16), one and several prefixes with
boundaries inside a tile and on its edge, few chains (tiles split over workgroups) and many (one workgroup per chain)."""
import ctypes as ct

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from eeyore_amd.kernels import IsoSEKernel
from eeyore_amd.kernels.homogeneous import pair_sums
from eeyore_amd.stats import batched
from tests import mmd_restatement as mr
from tests.test_mmd_host import CLASSES, KERNELS, g15, kernel_of, shape_data

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TILE, CHUNK = 64, 16   # MM_T, MM_PK of csrc/ey_mmd.hip
TORCH = {"f32": torch.float32, "f64": torch.float64}
PARAMS = {0: [0.7, 1.3], 1: [1.2, 0.8, 1.5], 2: [0.9, 1.1, 2.5]}


def check_sums(got, want, len1, len2, scale, p, diag):
    """got / want: (s11, s22, s12), each [k]; the bound of tests/mmd_restatement.py per sum"""
    a, b = np.array(len1, np.float64), np.array(len2, np.float64)
    for name, g, w, n in zip(("s11", "s22", "s12"), got, want, (mr.terms_symm(a, diag), mr.terms_symm(b, diag), a * b)):
        err, tol = np.abs(np.asarray(g) - w), mr.bound(n, scale, p)
        print(f"{name}: max error / bound = {np.max(err / tol):.3f}")
        assert np.all(err <= tol), (name, err, tol)


# ------------------------------------------------------------------------------------------------- the reference's numbers
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kn", KERNELS)
@pytest.mark.parametrize("s", range(3))
def test_fixture_through_the_c_abi_and_mmd_chains(s, kn, dt):
    z, g = g15(), f"s{s}/{kn}/"
    x1, x2, pre1, pre2 = shape_data(s)
    _, par, ker = kernel_of(kn)
    p, n2 = x1.shape[1], x2.shape[0]
    t1 = torch.tensor(x1, dtype=TORCH[dt], device=DEV)[:, None, :]   # [n1, 1, p]: the fixture's values are exact in f32
    t2 = torch.tensor(x2, dtype=TORCH[dt], device=DEV)
    for tag, l2 in (("c", pre2), ("a", [n2] * len(pre1))):               # all prefixes in one call
        for d in (1, 0):
            got = [v[0].cpu().numpy() for v in pair_sums(t1, t2, ker, lengths=pre1, lengths2=l2, include_diag=bool(d))]
            want = (z[g + f"sum11_d{d}"], z[g + f"sum22{tag}_d{d}"] * np.ones(len(pre1)), z[g + f"sum12{tag}"])
            check_sums(got, want, pre1, l2, par[0], p, d)
            sq = batched.mmd_chains(t1, t2, ker, lengths=pre1, lengths2=None if tag == "a" else l2, biased=bool(d), squared=True)
            assert sq.shape == (len(pre1), 1) and sq.dtype == torch.float64 and sq.is_cuda
            err = np.abs(sq[:, 0].cpu().numpy() - z[g + f"sqmmd_b{d}_{tag}"])
            assert np.all(err <= mr.bound_squared_mmd(par[0], p)), err
        m = batched.mmd_chains(t1, t2, ker, lengths=pre1, lengths2=None if tag == "a" else l2)
        torch.testing.assert_close(m, torch.sqrt(sq_biased(t1, t2, ker, pre1, None if tag == "a" else l2)), rtol=0, atol=0,
                                   equal_nan=True)
    whole = batched.mmd_chains(t1, t2, ker, squared=True)
    assert whole.shape == (1,) and abs(whole.item() - z[g + "sqmmd_b1_a"][-1]) <= mr.bound_squared_mmd(par[0], p)


@pytest.mark.parametrize("kn", KERNELS[:3])
def test_kernel_methods_on_device_tensors(kn):
    """Kernel.sum_symm_K / sum_K / stats.squared_mmd on device tensors and lists of them: the HIP kernel with C = 1"""
    from eeyore_amd import stats
    z, g = g15(), f"s1/{kn}/"
    x1, x2, _, _ = shape_data(1)
    _, par, ker = kernel_of(kn)
    n1, n2, p = x1.shape[0], x2.shape[0], x1.shape[1]
    t1, t2 = torch.tensor(x1, device=DEV), torch.tensor(x2, device=DEV)
    for d in (1, 0):
        for a, b in ((t1, t2), (list(t1.unbind(0)), list(t2.unbind(0)))):
            got = ker.sum_symm_K(a, include_diag=bool(d))
            assert got.shape == (1,) and got.is_cuda and got.dtype == torch.float64
            assert abs(got.item() - z[g + f"sum11_d{d}"][-1]) <= mr.bound(mr.terms_symm(n1, d), par[0], p)
            assert abs(ker.sum_symm_K(b, include_diag=bool(d)).item() - z[g + f"sum22a_d{d}"]) <= mr.bound(mr.terms_symm(n2, d), par[0], p)
            sq = stats.squared_mmd(a, b, ker, biased=bool(d))
            assert sq.shape == (1,) and abs(sq.item() - z[g + f"sqmmd_b{d}_a"][-1]) <= mr.bound_squared_mmd(par[0], p)
    assert abs(ker.sum_K(t1, t2).item() - z[g + "sum12a"][-1]) <= mr.bound(n1 * n2, par[0], p)
    assert abs(ker.sum_symm_K(t1[:1]).item() - par[0]) <= mr.bound(1, par[0], p)      # one point: k(x, x) = scale
    assert ker.sum_symm_K(t1[:1], include_diag=False).item() == 0.0
    f32 = stats.mmd(t1.float(), t2.float(), ker)
    assert f32.dtype == torch.float32 and abs(f32.item() ** 2 - z[g + "sqmmd_b1_a"][-1]) <= 2.0 ** -22


def sq_biased(t1, t2, ker, l1, l2):
    return batched.mmd_chains(t1, t2, ker, lengths=l1, lengths2=l2, squared=True)


# ------------------------------------------------------------------------------------------------- the restatement
def make_lengths(n, k, min_len=1):
    """k non-decreasing lengths up to n: inside a tile, on the tile's edge and around it, with equal neighbours"""
    if k == 1:
        return [n]
    cand = sorted({v for v in (min_len, 5, TILE - 1, TILE, TILE, TILE + 1, 100, 2 * TILE, n) if min_len <= v <= n} | {n})
    out = sorted((cand * k)[:k]) if len(cand) < k else sorted(cand[:k - 1] + [n])
    return out


def run_case(C, n1, n2, p, k, kind, dt, layout, shared, diag=True, len2_const=False, seed=0, x1=None):
    rng = np.random.default_rng([seed, n1, n2, p])
    x2 = (0.3 + 1.2 * rng.standard_normal((1 if shared else C, n2, p))).astype(np.float32).astype(np.float64)
    if x1 is None:
        x1 = rng.standard_normal((C, n1, p)).astype(np.float32).astype(np.float64)
    lo = 1 if diag else 2
    l1 = make_lengths(n1, k, lo)
    l2 = [n2] * k if len2_const else make_lengths(n2, k, lo)
    par = PARAMS[kind]
    ker = CLASSES[kind](*par)
    t1 = torch.tensor(x1, dtype=TORCH[dt], device=DEV)
    t2 = torch.tensor(x2[0] if shared else x2, dtype=TORCH[dt], device=DEV)
    if layout == "ncp":
        t1 = t1.transpose(0, 1).contiguous()
        t2 = t2 if shared else t2.transpose(0, 1).contiguous()
    got = pair_sums(t1, t2, ker, layout=layout, lengths=None if k == 1 else l1, lengths2=None if k == 1 else l2,
                    include_diag=diag)
    torch.cuda.synchronize()
    got = [v.cpu().numpy() for v in got]
    assert all(v.shape == (C, k) for v in got)
    for c in range(C):
        want = mr.pair_sums(x1[c], x2[0 if shared else c], kind, par, l1, l2, diag)
        check_sums([v[c] for v in got], want, l1, l2, par[0], p, diag)
    return got, (t1, t2, ker, l1, l2)


N1, N2 = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 2), (1, TILE, TILE + 33)
ROWS = [(n1, n2) for n1 in N1 for n2 in N2]


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("i", range(len(ROWS)))
def test_rows_against_the_restatement(i, k):
    n1, n2 = ROWS[i]
    diag = not (i % 3 == 1 and min(n1, n2) >= 2)       # a third of the sizes that allow it: without the diagonal
    run_case(C=3, n1=n1, n2=n2, p=3, k=k, kind=i % 3, dt=("f64", "f32")[i % 2], layout=("ncp", "cnp")[(i // 2) % 2],
             shared=bool((i // 3) % 2), diag=diag, len2_const=(i % 4 == 3))


@pytest.mark.parametrize("p", [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 33, 70, 128, 1315])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_columns_against_the_restatement(p, kind):
    big = p == 1315                                      # the headline model's width: a handful of rows
    run_case(C=1 if big else 3, n1=9 if big else TILE + 1, n2=8 if big else TILE, p=p, k=7 if p in (2, 70) else 1, kind=kind,
             dt=("f64", "f32")[(p + kind) % 2], layout=("ncp", "cnp")[p % 2], shared=bool(kind % 2))


@pytest.mark.parametrize("layout", ["ncp", "cnp"])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("C", [1, 3, 11])
def test_chains_layouts_and_second_samples(C, shared, layout):
    run_case(C=C, n1=2 * TILE + 2, n2=TILE + 33, p=2, k=7, kind=0, dt="f64", layout=layout, shared=shared)


def test_split_over_workgroups_and_not(monkeypatch):
    """A call aims at EY_MMD_SPLIT_TARGET workgroups (4 per CU by default): fewer chains than that and each chain's tiles are
    split over several workgroups whose partial sums meet in a workspace, at least that many and every chain has one."""
    target = 8
    monkeypatch.setenv("EY_MMD_SPLIT_TARGET", str(target))
    x1 = np.random.default_rng(5).standard_normal((target, 2 * TILE + 2, 3)).astype(np.float32).astype(np.float64)
    run_case(C=target - 1, n1=2 * TILE + 2, n2=TILE + 33, p=3, k=7, kind=0, dt="f64", layout="cnp", shared=True,
             x1=x1[:target - 1])
    assert L.lib().ey_debug_mmd_last_split() == 2        # ceil(8 / 7) workgroups per chain
    run_case(C=target, n1=2 * TILE + 2, n2=TILE + 33, p=3, k=7, kind=0, dt="f64", layout="cnp", shared=True, x1=x1)
    assert L.lib().ey_debug_mmd_last_split() == 1
    run_case(C=1, n1=2 * TILE + 2, n2=TILE + 33, p=3, k=7, kind=0, dt="f64", layout="cnp", shared=False, x1=x1[:1])
    assert L.lib().ey_debug_mmd_last_split() == 8        # s11: 6 tiles, s22: 3, s12: 6 -- more than the target
    monkeypatch.setenv("EY_MMD_SPLIT_TARGET", "1")
    for C in (1, 3):                                     # never split, whatever C
        run_case(C=C, n1=2 * TILE + 2, n2=TILE + 33, p=3, k=7, kind=1, dt="f32", layout="ncp", shared=False)
        assert L.lib().ey_debug_mmd_last_split() == 1


@pytest.mark.parametrize("target", [None, "1"], ids=["split", "whole"])
def test_replicas_and_repeats_are_bit_identical(monkeypatch, target):
    if target:
        monkeypatch.setenv("EY_MMD_SPLIT_TARGET", target)
    got, (t1, t2, ker, l1, l2) = run_case(C=11, n1=2 * TILE + 2, n2=TILE + 33, p=3, k=7, kind=2, dt="f64", layout="cnp",
                                          shared=False)
    r1, r2 = t1.repeat(28, 1, 1)[:300], t2.repeat(28, 1, 1)[:300]     # chain c holds the data of chain c % 11
    a = torch.stack(pair_sums(r1, r2, ker, layout="cnp", lengths=l1, lengths2=l2))
    b = torch.stack(pair_sums(r1, r2, ker, layout="cnp", lengths=l1, lengths2=l2))
    assert a.shape == (3, 300, 7) and torch.equal(a.view(torch.int64), b.view(torch.int64))
    first = a[:, :11].repeat(1, 28, 1)[:, :300]
    assert torch.equal(a.view(torch.int64), first.view(torch.int64))
    check = [v.cpu().numpy() for v in a[:, :11]]
    for c in range(11):   # 300 chains take fewer workgroups per chain than 11 did: two results within the bound of the truth
        check_sums([v[c] for v in check], [v[c] for v in got], l1, l2, 2 * PARAMS[2][0], 3, True)


def abi(t1, t2, kind, par, l1, l2, out, k, C, diag=1):
    """a direct call on [C, n, p] tensors with the three outputs at out[q] (pointers into larger buffers)"""
    n1, n2, p = t1.shape[1], t2.shape[1], t1.shape[2]
    arr = lambda v: (ct.c_int64 * len(v))(*v)  # noqa: E731
    rc = L.lib().ey_kernel_pair_sums(L.ptr(t1), n1, C, p, p, n1 * p, L.ptr(t2), n2, p, n2 * p, L.EY_F64, kind,
                                     (ct.c_double * 3)(*(par + [0.0])[:3]), arr(l1), arr(l2), k, diag, *[L.ptr(o) for o in out],
                                     ct.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    L.check(rc, "ey_kernel_pair_sums")
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [5, 2000], ids=["split", "whole"])
def test_guards(C):
    k, pad, n1, n2, p = 3, 64, TILE + 6, TILE, 2
    rng = np.random.default_rng(9)
    t1 = torch.tensor(rng.standard_normal((5, n1, p)), device=DEV).repeat(C // 5, 1, 1).contiguous()
    t2 = torch.tensor(rng.standard_normal((5, n2, p)), device=DEV).repeat(C // 5, 1, 1).contiguous()
    l1, l2 = [3, TILE, n1], [2, TILE - 1, n2]

    def run(x1):
        buf = torch.full((3, C * k + 2 * pad), -7.25, dtype=torch.float64, device=DEV)
        abi(x1, t2, 0, PARAMS[0], l1, l2, [buf[q, pad:pad + C * k] for q in range(3)], k, C)
        assert bool((buf[:, :pad] == -7.25).all()) and bool((buf[:, pad + C * k:] == -7.25).all())   # the padding is kept
        return buf[:, pad:pad + C * k].reshape(3, C, k).clone()

    clean = run(t1)
    assert torch.isfinite(clean).all()
    bad = t1.clone()
    bad[2, TILE + 1, 1] = float("nan")                   # one sample of chain 2, in its last prefix only
    got = run(bad)
    assert torch.isnan(got[0, 2, 2]) and torch.isnan(got[2, 2, 2])
    keep = torch.ones(3, C, k, dtype=torch.bool, device=DEV)
    keep[0, 2, 2] = keep[2, 2, 2] = False                # everything else, its own s22 and earlier prefixes included: same bits
    assert torch.equal(got[keep].view(torch.int64), clean[keep].view(torch.int64))


# ------------------------------------------------------------------------------------------------- end to end
def test_mixture_chains_against_a_direct_sample():
    """The workflow of examples/mixture_mmd.py: Metropolis-Hastings on the bivariate normal mixture for 64 chains, each
    chain's MMD curve against a direct sample of the target -- equal to the torch host path chain by chain."""
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.models import DistributionModel, NormalMixture
    from eeyore_amd.samplers import MetropolisHastings
    from eeyore_amd import stats
    C, n, lengths = 64, 200, [50, 100, 200]
    means = torch.tensor([[-2., -2.], [2., 2.]])
    model = DistributionModel(NormalMixture([1., 1.], means, torch.eye(2).expand(2, 2, 2), normalized=False), 2,
                              dtype=torch.float32, device=DEV)
    sampler = MetropolisHastings(model, theta0=torch.zeros(C, 2, device=DEV), dataloader=DataLoader(EmptyXYDataset()), seed=1)
    sampler.run(num_epochs=n, num_burnin_epochs=0)
    chain = sampler.get_chain()
    gen = torch.Generator().manual_seed(3)
    direct = (means[torch.randint(2, (n,), generator=gen)] + torch.randn(n, 2, generator=gen)).to(DEV)
    curve = chain.mmd(direct, lengths=lengths)            # IsoSEKernel() by default, every prefix against all of `direct`
    assert curve.shape == (3, C) and curve.dtype == torch.float64 and torch.isfinite(curve).all()
    sq = batched.mmd_chains(chain.get_samples(), direct, IsoSEKernel(), lengths=lengths, squared=True).cpu().numpy()
    torch.testing.assert_close(curve.cpu() ** 2, torch.tensor(sq), rtol=1e-12, atol=1e-300)
    host, dh, ker = chain.get_samples().cpu().double(), direct.cpu().double(), IsoSEKernel()   # exact copies of the f32 samples
    assert host.shape == (n, C, 2)
    tol = mr.bound_squared_mmd(1.0, 2)
    for c in range(C):
        want = np.array([stats.squared_mmd(host[:m, c], dh, ker).item() for m in lengths])
        assert np.all(np.abs(sq[:, c] - want) <= tol), (c, sq[:, c], want)
    same = chain.mmd(direct, lengths=lengths, lengths2=lengths)   # the reference example's curve: prefix against prefix
    assert same.shape == (3, C) and bool(((same[-1] ** 2 - curve[-1] ** 2).abs() <= 2 * tol).all())
    want = stats.squared_mmd(host[:50, 7], dh[:50], ker).item()
    assert abs(same[0, 7].item() ** 2 - want) <= tol
