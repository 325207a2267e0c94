"""Kernel sums and MMD without a GPU: the numpy restatement (tests/mmd_restatement.py) and the torch host path of
kernels.Kernel / stats.squared_mmd / stats.mmd against the reference's own numbers (tests/golden/g15_mmd.npz), the pairwise
fallback of a k-only kernel, the C symbol, the host-side validation of ey_kernel_pair_sums and mmd_chains' argument errors."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from eeyore_amd import stats
from eeyore_amd.kernels import HomogeneousKernel, IsoSEKernel, Kernel, PeriodicKernel, RQKernel
from eeyore_amd.stats import batched
from tests import mmd_restatement as mr
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 29, 1), (37, 29, 3), (19, 17, 70)]
KERNELS = ("isose", "rq", "periodic", "isose_default", "rq_default", "periodic_default")
CLASSES = {0: IsoSEKernel, 1: RQKernel, 2: PeriodicKernel}
_G15 = {}


def g15():
    if not _G15:
        z = load("g15_mmd.npz")
        _G15.update({k: z[k] for k in z.files})
    return _G15


def kernel_of(kn):
    kind, *par = g15()[f"kernels/{kn}"]
    par = [float(v) for v in par if not np.isnan(v)]
    return int(kind), par, CLASSES[int(kind)](*par)


def shape_data(s):
    z = g15()
    return z[f"s{s}/x1"], z[f"s{s}/x2"], z[f"s{s}/prefix1"].tolist(), z[f"s{s}/prefix2c"].tolist()


def check_against_fixture(s, kn, sums_of, sq_of):
    """``sums_of(len1, len2, include_diag)`` -> (s11, s22, s12) arrays; ``sq_of(len1, len2, biased)`` -> squared_mmd array;
    compared with group s<s>/<kn> of the fixture within the derived bounds."""
    z, g = g15(), f"s{s}/{kn}/"
    x1, x2, pre1, pre2 = shape_data(s)
    scale, p, n2 = z[f"kernels/{kn}"][1], x1.shape[1], x2.shape[0]
    a, b = np.array(pre1, np.float64), np.array(pre2, np.float64)
    for d in (1, 0):
        s11, s22, s12 = sums_of(pre1, pre2, bool(d))
        assert np.all(np.abs(s11 - z[g + f"sum11_d{d}"]) <= mr.bound(mr.terms_symm(a, d), scale, p))
        assert np.all(np.abs(s22 - z[g + f"sum22c_d{d}"]) <= mr.bound(mr.terms_symm(b, d), scale, p))
        assert np.all(np.abs(s12 - z[g + "sum12c"]) <= mr.bound(a * b, scale, p))
        s11, s22, s12 = sums_of(pre1, [n2] * len(pre1), bool(d))
        assert np.all(np.abs(s22 - z[g + f"sum22a_d{d}"]) <= mr.bound(mr.terms_symm(n2, d), scale, p))
        assert np.all(np.abs(s12 - z[g + "sum12a"]) <= mr.bound(a * n2, scale, p))
    for bi in (1, 0):
        assert np.all(np.abs(sq_of(pre1, pre2, bool(bi)) - z[g + f"sqmmd_b{bi}_c"]) <= mr.bound_squared_mmd(scale, p))
        assert np.all(np.abs(sq_of(pre1, [n2] * len(pre1), bool(bi)) - z[g + f"sqmmd_b{bi}_a"]) <= mr.bound_squared_mmd(scale, p))
    # the fixture's mmd is the square root of its biased estimate, NaN where that is negative (the periodic kernel at p = 70);
    # compared through the square: sqrt is ill-conditioned at 0
    for v in "ca":
        sq = z[g + f"sqmmd_b1_{v}"]
        np.testing.assert_allclose(z[g + f"mmd_{v}"] ** 2, np.where(sq < 0, np.nan, sq), rtol=1e-14,
                                   atol=mr.bound_squared_mmd(scale, p))


@pytest.mark.parametrize("kn", KERNELS)
@pytest.mark.parametrize("s", range(3))
def test_restatement_reproduces_the_fixture(s, kn):
    z, g = g15(), f"s{s}/{kn}/"
    x1, x2, _, _ = shape_data(s)
    assert x1.shape == SHAPES[s][::2] and x2.shape == SHAPES[s][1:]
    assert np.array_equal(x1, x1.astype(np.float32)) and np.array_equal(x2, x2.astype(np.float32))
    kind, par, _ = kernel_of(kn)
    one = mr.bound(1, par[0], x1.shape[1])
    rows = z[g + "K"].shape[0]   # the fixture keeps the first rows of the two matrices
    assert np.all(np.abs(mr.kernel_matrix(x1, x2, kind, par)[:rows] - z[g + "K"]) <= one)
    assert np.all(np.abs(mr.kernel_matrix(x1, x1, kind, par)[:rows] - z[g + "symm_K"]) <= one)

    def sums_of(l1, l2, d):
        return mr.pair_sums(x1, x2, kind, par, l1, l2, d)

    def sq_of(l1, l2, biased):
        return mr.squared_mmd(*mr.pair_sums(x1, x2, kind, par, l1, l2, biased), l1, l2, biased)

    check_against_fixture(s, kn, sums_of, sq_of)


@pytest.mark.parametrize("as_list", [False, True], ids=["tensor", "list"])
@pytest.mark.parametrize("kn", KERNELS)
@pytest.mark.parametrize("s", range(3))
def test_torch_host_path_reproduces_the_fixture(s, kn, as_list):
    z, g = g15(), f"s{s}/{kn}/"
    x1, x2, _, _ = shape_data(s)
    _, par, ker = kernel_of(kn)
    t1, t2 = torch.tensor(x1), torch.tensor(x2)
    if as_list:
        t1, t2 = list(t1.unbind(0)), list(t2.unbind(0))
    one = mr.bound(1, par[0], x1.shape[1])
    K, SK = ker.K(t1, t2), ker.symm_K(t1)
    assert K.dtype == torch.float64 and K.shape == (x1.shape[0], x2.shape[0])
    rows = z[g + "K"].shape[0]   # the fixture keeps the first rows of the two matrices
    assert np.all(np.abs(K.numpy()[:rows] - z[g + "K"]) <= one) and np.all(np.abs(SK.numpy()[:rows] - z[g + "symm_K"]) <= one)
    assert torch.equal(SK, SK.T) and SK.shape == (x1.shape[0], x1.shape[0])
    assert np.all(np.abs(SK.numpy()[:, :rows].T - z[g + "symm_K"]) <= one)
    assert abs(float(ker.k(t1[2], t2[1])) - z[g + "K"][2, 1]) <= one

    def sums_of(l1, l2, d):
        r = [(ker.sum_symm_K(t1[:a], include_diag=d), ker.sum_symm_K(t2[:b], include_diag=d), ker.sum_K(t1[:a], t2[:b]))
             for a, b in zip(l1, l2)]
        assert all(v.shape == (1,) and v.dtype == torch.float64 for row in r for v in row)   # as the reference returns them
        return tuple(np.array([row[i].item() for row in r]) for i in range(3))

    def sq_of(l1, l2, biased):
        r = [stats.squared_mmd(t1[:a], t2[:b], ker, biased=biased) for a, b in zip(l1, l2)]
        assert all(v.shape == (1,) for v in r)
        return np.array([v.item() for v in r])

    check_against_fixture(s, kn, sums_of, sq_of)
    m = stats.mmd(t1, t2, ker)
    torch.testing.assert_close(m, torch.sqrt(stats.squared_mmd(t1, t2, ker)), rtol=0, atol=0, equal_nan=True)
    want = z[g + "sqmmd_b1_a"][-1]
    assert torch.isnan(m).all() if want < 0 else abs(m.item() ** 2 - want) <= mr.bound_squared_mmd(par[0], x1.shape[1])


def test_f32_samples_give_the_f64_result_rounded_once():
    x1, x2, _, _ = shape_data(1)
    ker = kernel_of("rq")[2]
    t1, t2 = torch.tensor(x1), torch.tensor(x2)
    got = ker.sum_K(t1.float(), t2.float())
    assert got.dtype == torch.float32 and torch.equal(got, ker.sum_K(t1, t2).float())
    assert ker.K(t1.float(), t2.float()).dtype == torch.float32


def test_check_input():
    ker = IsoSEKernel()
    x = [torch.zeros(2), torch.ones(2, dtype=torch.float64)]
    with pytest.raises(ValueError):
        ker.sum_symm_K(x, check_input=True)
    with pytest.raises(ValueError):
        ker.K([torch.zeros(2)], x, check_input=True)
    ker.K([torch.zeros(2)], [torch.ones(2)], check_input=True)


class OnlyK(Kernel):
    """what a user writes: nothing but k (here IsoSEKernel(0.7, 1.3)'s formula)"""

    calls = 0

    def k(self, x1, x2):
        OnlyK.calls += 1
        return 0.7 * torch.exp(-(x1 - x2).pow(2).sum() / 2.6)


class OverriddenK(IsoSEKernel):
    def k(self, x1, x2):
        return super().k(x1, x2) * 2.0


def test_a_k_only_subclass_goes_through_the_pairwise_fallback():
    x1, x2, _, _ = shape_data(1)
    t1, t2 = torch.tensor(x1[:7]), torch.tensor(x2[:5])
    ref, ker = IsoSEKernel(0.7, 1.3), OnlyK()
    OnlyK.calls = 0
    torch.testing.assert_close(ker.K(t1, t2), ref.K(t1, t2), rtol=1e-13, atol=1e-15)
    assert OnlyK.calls == 35
    torch.testing.assert_close(ker.symm_K(list(t1)), ref.symm_K(t1), rtol=1e-13, atol=1e-15)
    assert OnlyK.calls == 35 + 28   # the upper triangle and the diagonal, mirrored
    for d in (True, False):
        torch.testing.assert_close(ker.sum_symm_K(t1, include_diag=d), ref.sum_symm_K(t1, include_diag=d), rtol=1e-13, atol=0)
    torch.testing.assert_close(ker.sum_K(t1, t2), ref.sum_K(t1, t2), rtol=1e-13, atol=0)
    torch.testing.assert_close(stats.mmd(t1, t2, ker), stats.mmd(t1, t2, ref), rtol=1e-10, atol=0)
    # a subclass of one of the three that changes k is no longer the function the vectorised forms (and the HIP kernel) compute
    assert OverriddenK().device_kind() is None and IsoSEKernel().device_kind() == (0, [1.0, 1.0])
    torch.testing.assert_close(OverriddenK(0.7, 1.3).sum_K(t1, t2), 2.0 * ref.sum_K(t1, t2), rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        batched.mmd_chains(torch.zeros(4, 2, 2), torch.zeros(3, 2), OverriddenK())
    assert issubclass(RQKernel, HomogeneousKernel) and RQKernel().device_kind() == (1, [1.0, 1.0, 1.0])
    assert PeriodicKernel().device_kind() == (2, [1.0, 1.0, 2.0])
    a, b = torch.tensor([3.0, 0.0]), torch.tensor([0.0, 4.0])
    assert float(ref.dist(a, b)) == 5.0 and abs(float(ref.squared_dist(a, b)) - 25.0) < 1e-12


# ------------------------------------------------------------------------------------------------- the C entry point
def test_symbol_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    assert re.search(r"\bint ey_kernel_pair_sums\(const void\* x1, int64_t n1, int64_t C, int64_t p,", header)
    assert "ey_kernel_pair_sums" in L.SYMBOLS and len(L.SYMBOLS["ey_kernel_pair_sums"][1]) == 21
    assert hasattr(ct.CDLL(L.LIB_PATH), "ey_kernel_pair_sums")
    assert "int ey_debug_mmd_last_split(void);" in header and isinstance(L.lib().ey_debug_mmd_last_split(), int)


FAKE = ct.c_void_p(0x1000)   # never dereferenced: every call below is rejected before anything touches the device


def call(n1=8, n2=6, C=2, p=3, x1=FAKE, x2=FAKE, dtype=L.EY_F64, kind=0, params=(1.0, 1.0, 1.0), len1=None, len2=None, k=1,
         include_diag=1, s11=FAKE, s22=FAKE, s12=FAKE):
    arr = lambda v: None if v is None else (ct.c_int64 * len(v))(*v)  # noqa: E731
    rc = L.lib().ey_kernel_pair_sums(x1, n1, C, p, C * p, p, x2, n2, p, 0, dtype, kind, (ct.c_double * 3)(*params), arr(len1),
                                     arr(len2), k, include_diag, s11, s22, s12, None)
    return rc, L.lib().ey_last_error().decode()


NAN, INF = float("nan"), float("inf")
INVALID = {
    "n1": dict(n1=0), "n2": dict(n2=0), "C": dict(C=0), "p": dict(p=0), "k": dict(k=0), "k_negative": dict(k=-1),
    "kind_high": dict(kind=3), "kind_low": dict(kind=-1), "dtype": dict(dtype=2),
    "scale_zero": dict(params=(0.0, 1.0, 1.0)), "scale_negative": dict(params=(-1.0, 1.0, 1.0)),
    "scale_nan": dict(params=(NAN, 1.0, 1.0)), "scale_inf": dict(params=(INF, 1.0, 1.0)),
    "l_zero": dict(params=(1.0, 0.0, 1.0)), "l_nan": dict(params=(1.0, NAN, 1.0)), "l_inf": dict(params=(1.0, INF, 1.0)),
    "a_zero": dict(kind=1, params=(1.0, 1.0, 0.0)), "a_negative": dict(kind=1, params=(1.0, 1.0, -2.0)),
    "a_nan": dict(kind=1, params=(1.0, 1.0, NAN)), "a_inf": dict(kind=1, params=(1.0, 1.0, INF)),
    "period_zero": dict(kind=2, params=(1.0, 1.0, 0.0)), "period_nan": dict(kind=2, params=(1.0, 1.0, NAN)),
    "period_inf": dict(kind=2, params=(1.0, 1.0, INF)),
    "len1_only": dict(len1=[2, 4], k=2), "len2_only": dict(len2=[2, 4], k=2), "no_lengths_k2": dict(k=2),
    "decreasing1": dict(len1=[4, 3], len2=[2, 2], k=2), "decreasing2": dict(len1=[3, 4], len2=[3, 2], k=2),
    "len1_zero": dict(len1=[0, 3], len2=[2, 2], k=2), "len1_beyond": dict(len1=[3, 9], len2=[2, 2], k=2),
    "len2_zero": dict(len1=[3, 3], len2=[0, 2], k=2), "len2_beyond": dict(len1=[3, 3], len2=[2, 7], k=2),
    "no_diag_len1": dict(len1=[1, 3], len2=[2, 2], k=2, include_diag=0),
    "no_diag_len2": dict(len1=[2, 3], len2=[1, 2], k=2, include_diag=0), "no_diag_n1": dict(n1=1, include_diag=0),
    "null_s11": dict(s11=None), "null_s22": dict(s22=None), "null_s12": dict(s12=None), "null_x1": dict(x1=None),
    "null_x2": dict(x2=None),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_rejected_before_the_device(case):
    rc, msg = call(**INVALID[case])
    assert rc == -1 and msg.startswith("ey_kernel_pair_sums:") and len(msg) > 25, (rc, msg)


def test_more_than_1024_prefixes_are_unsupported():
    n = 2000
    rc, msg = call(n1=n, n2=n, len1=list(range(1, 1026)), len2=list(range(1, 1026)), k=1025)
    assert rc == -2 and "1024" in msg


def test_period_may_be_negative_and_diag_free_sums_accept_length_two():
    # accepted by the validation: without a device the call then fails in the HIP runtime, with one it must not be made on
    # fake pointers -- so only the host path, which computes the same function, is run here
    t = torch.tensor(shape_data(1)[0])
    torch.testing.assert_close(PeriodicKernel(0.9, 1.1, -2.5).sum_symm_K(t[:2], include_diag=False),
                               PeriodicKernel(0.9, 1.1, 2.5).sum_symm_K(t[:2], include_diag=False))


# ------------------------------------------------------------------------------------------------- mmd_chains' arguments
def test_mmd_chains_argument_errors():
    x, y, ker = torch.zeros(8, 3, 2), torch.zeros(6, 2), IsoSEKernel()
    bad = [
        dict(kernel=OnlyK()), dict(kernel=Kernel()),
        dict(x2=y.double()), dict(x2=torch.zeros(6, 3)), dict(x2=torch.zeros(6, 4, 2)),
        dict(samples=x.to(torch.float16), x2=y.to(torch.float16)),
        dict(biased=False, squared=True, lengths=[1, 4]), dict(biased=False, squared=True, lengths=[2, 4], lengths2=[1, 2]),
        dict(samples=torch.zeros(1, 3, 2), biased=False, squared=True),
        dict(lengths=[4, 3]), dict(lengths=[0, 3]), dict(lengths=[3, 9]), dict(lengths=[]),
        dict(lengths=[2, 3], lengths2=[3, 2]), dict(lengths=[2, 3], lengths2=[2, 7]), dict(lengths=[2, 3], lengths2=[2]),
        dict(lengths2=[2]), dict(layout="pnc"), dict(samples=torch.zeros(8, 2)),
    ]
    for kw in bad:
        args = dict(samples=x, x2=y, kernel=ker)
        args.update(kw)
        with pytest.raises(ValueError):
            batched.mmd_chains(**args)
    with pytest.raises(RuntimeError, match="ROCm device"):
        batched.mmd_chains(x, y, ker)
    with pytest.raises(RuntimeError, match="ROCm device"):
        batched.mmd_chains(x, y, ker, lengths=[2, 8], lengths2=[2, 6])
