"""One chain and tiny batches on every kernel family, against the f64 C oracle.

The reference's normal use is one chain (theta of shape [P]) on a small batch or a minibatch; the rest of the suite runs
five chains or more.  Every case here starts on a FRESH plan whose first call is the small one (a plan's workspace only
grows, so an earlier larger call would hide a kernel that writes past what the small call sized), pins the route with
`Plan.kernel` and the variant bits, and runs the entry points in a fixed order against the oracle with the tolerances of
test_random_architectures_vs_oracle.  Every buffer a kernel is handed is the middle of a larger one filled with a canary
(NaN, 0xAB bytes): the canary must survive and read-only inputs must keep their bits.  Then the same calls on a second
plan, each behind a 1024-chain call through the same entry point, must give the same bits: a chain's arithmetic does not
depend on the workspace's history.

Variant bits (ey_debug_set_variant / Plan.set_variant, include/eeyore_amd.h): 16 the layerwise family whatever the model,
8192 the fused mid-size kernel k_mid, 16384 k_mid32 off."""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle.c_oracle import COracle
from tests.test_gpu_parity import F32_DECISION_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 32           # canary chains on either side of every buffer
GROW = 1024        # the chain count of the call that grows the second plan's workspace
STEP, LSTEPS = 0.01, 4
CANARY_U8 = 0xAB

# family, dims, acts, bias, lik, dtype, expected kernel, plan options, chain counts, row counts
#   options: variant (ey_debug_set_variant while the plan is made), products (f32_products), row_waves, plain (one
#   prior scale and no temperature: the fused16 plain-HMC instantiation)
FAMILIES = [
    ("mfma32-bf16x3", [4, 32, 32, 3], [1, 1, 0], None, 1, "f32", "mfma32", dict(products="bf16x3"), (1, 2, 3), (1, 10, 33)),
    ("mfma32-exact", [4, 32, 32, 3], [1, 1, 0], None, 1, "f32", "mfma32", dict(products="exact"), (1, 2, 3), (1, 10, 33)),
    ("mfma32-kind2", [4, 32, 32, 1], [1, 1, 1], None, 0, "f32", "mfma32", dict(products="bf16x3"), (1, 3), (1, 10)),
    ("fused16", [6, 20, 24, 2], [2, 1, 0], None, 1, "f64", "fused16", {}, (1, 3), (1, 4, 17)),
    ("fused16", [3, 64, 64, 4], [1, 3, 0], None, 1, "f32", "fused16", dict(products="exact"), (1, 3), (1, 4, 17)),
    ("fused16", [5, 20, 3], [1, 0], None, 1, "f64", "fused16", {}, (1, 3), (1, 4, 17)),
    ("fused16-plain", [6, 20, 24, 2], [2, 1, 0], None, 1, "f64", "fused16", dict(plain=True), (1, 3), (1, 4, 17)),
    ("fused16-plain", [3, 64, 64, 4], [1, 3, 0], None, 1, "f32", "fused16", dict(products="exact", plain=True), (1, 3), (1, 4, 17)),
    ("fused16-plain", [5, 20, 3], [1, 0], None, 1, "f64", "fused16", dict(plain=True), (1, 3), (1, 4, 17)),
    ("generic-regs", [2, 3, 2, 1], [1, 1, 1], None, 0, "f32", "generic", {}, (1, 2), (1, 5)),
    ("generic-regs", [2, 3, 2, 1], [1, 1, 1], None, 0, "f64", "generic", {}, (1, 2), (1, 5)),
    ("generic-lds", [4, 8, 8, 8, 3], [1, 2, 3, 0], None, 1, "f64", "generic", {}, (1, 2), (1, 5)),
    ("generic-logreg", [5, 3], [0], None, 1, "f64", "generic", {}, (1, 2), (1, 5)),
    ("generic-rowwaves", [3, 4, 2, 2], [2, 3, 0], None, 1, "f64", "generic", dict(row_waves="auto"), (1,), (128, 129, 257)),
    ("layerwise", [5, 32, 1], [2, 1], None, 0, "f32", "bgemm", dict(variant=16 | 16384), (1, 3), (1, 10)),
    ("layerwise", [5, 32, 1], [2, 1], None, 0, "f64", "bgemm", dict(variant=16 | 16384), (1, 3), (1, 10)),
    ("layerwise", [6, 16, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 16384), (1, 3), (1, 10)),
    ("layerwise", [6, 16, 10], [1, 0], None, 1, "f64", "bgemm", dict(variant=16 | 16384), (1, 3), (1, 10)),
    ("layerwise", [784, 128, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 16384), (1, 3), (1, 10)),
    ("layerwise", [784, 128, 10], [1, 0], None, 1, "f64", "bgemm", dict(variant=16 | 16384), (1, 3), (1, 10)),
    ("k_mid32", [16, 32, 32, 32, 3], [1, 1, 1, 0], None, 1, "f32", "bgemm", {}, (1, 2, 3), (1, 4, 10, 13)),
    ("k_mid32", [64, 32, 32, 10], [1, 2, 0], [1, 0, 1], 1, "f32", "bgemm", {}, (1, 2, 3), (1, 4, 10, 13)),
    ("k_mid32", [5, 32, 1], [2, 1], None, 0, "f32", "bgemm", dict(variant=16), (1, 2, 3), (1, 4, 10, 13)),
    ("k_mid", [10, 100, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 8192), (1, 3), (1, 10)),
    ("k_mid", [20, 100, 100, 5], [1, 2, 0], None, 1, "f32", "bgemm", dict(variant=16 | 8192), (1, 3), (1, 10)),
]
# Families whose per-chain arithmetic depends on how many chains share the launch, so that the bits after a 1024-chain
# call may differ (the history check then compares against the oracle only): row_waves='auto' gives a chain several waves
# when the launch leaves the chip idle and one when it does not (ey_generic.hip, row_waves_for), by design.
HISTORY_EXEMPT = {"generic-rowwaves"}

CASES = [pytest.param(fam, dims, acts, bias, lik, tag, kern, opts, C, N,
                      id=f"{fam}-{'x'.join(map(str, dims))}-{tag}-C{C}-N{N}")
         for fam, dims, acts, bias, lik, tag, kern, opts, Cs, Ns in FAMILIES for C in Cs for N in Ns]


# ------------------------------------------------------------------------------------------------- guarded buffers
def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


class Guarded:
    """A tensor of `shape` that is the middle of a larger buffer: PAD chains of canary on either side (`row` elements per
    chain, by default everything behind the first axis).  `readonly` remembers the bits of the middle too."""

    def __init__(self, shape, dtype, value=None, row=None, readonly=False):
        shape = tuple(shape)
        n = int(np.prod(shape))
        row = row if row is not None else int(np.prod(shape[1:]))
        self.pad = PAD * row
        self.buf = torch.empty(n + 2 * self.pad, dtype=dtype, device=DEV)
        if dtype.is_floating_point:
            self.buf.fill_(float("nan"))
        elif dtype == torch.uint8:
            self.buf.fill_(CANARY_U8)
        else:
            self.buf.view(torch.uint8).fill_(CANARY_U8)
        self.t = self.buf[self.pad:self.pad + n].view(shape)
        if value is not None:
            self.t.copy_(torch.as_tensor(value).to(device=DEV, dtype=dtype).reshape(shape))
        self.head = _bits(self.buf[:self.pad]).clone()
        self.tail = _bits(self.buf[self.pad + n:]).clone()
        self.orig = _bits(self.t).clone() if readonly else None

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert torch.equal(_bits(self.buf[:self.pad]), self.head), f"{what}: written before the first chain"
        assert torch.equal(_bits(self.buf[self.pad + n:]), self.tail), f"{what}: written beyond the last chain"
        if self.orig is not None:
            assert torch.equal(_bits(self.t), self.orig), f"{what}: a read-only input was changed"


def _check(**bufs):
    for name, g in bufs.items():
        if g is not None:
            g.check(name)


def _p(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ct.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _call(name, *args):
    from eeyore_amd import _lib as L
    L.check(getattr(L.lib(), name)(*args), name)


# ---------------------------------------------------------------------------------------------------------- the case
class Case:
    def __init__(self, fam, dims, acts, bias, lik, tag, kern, opts, C, N):
        self.fam, self.dims, self.acts, self.lik, self.kern, self.opts, self.C, self.N = fam, dims, acts, lik, kern, opts, C, N
        self.nl = len(dims) - 1
        self.bias = bias if bias is not None else [1] * self.nl
        self.f64 = tag == "f64"
        self.npdt, self.dt = (np.float64, torch.float64) if self.f64 else (np.float32, torch.float32)
        self.P = sum((dims[l] + self.bias[l]) * dims[l + 1] for l in range(self.nl))
        rng = np.random.default_rng(sum(dims) * 7 + 31 * C + N + (1 if self.f64 else 0))
        self.x = rng.standard_normal((N, dims[0])).astype(self.npdt)
        if lik == 1:
            self.y = np.eye(dims[-1], dtype=self.npdt)[rng.integers(0, dims[-1], N)]
        else:
            self.y = (rng.random((N, dims[-1])) < 0.5).astype(self.npdt)
        self.plain = bool(opts.get("plain"))
        if self.plain:
            self.mu, self.sigma = np.full(self.P, 0.05), np.full(self.P, 1.3)
        else:
            self.mu = (0.1 * rng.standard_normal(self.P)).astype(self.npdt).astype(np.float64)
            self.sigma = (0.5 + rng.random(self.P)).astype(self.npdt).astype(np.float64)
        self.temp = None if self.plain else (np.array([0.7]) if C == 1 else np.linspace(1.0, 0.4, C)).astype(self.npdt)
        self.th0 = (0.3 / np.sqrt(max(dims)) * 4 * rng.standard_normal((C, self.P))).astype(self.npdt)
        self.p0 = rng.standard_normal((C, self.P)).astype(self.npdt)
        self.z = rng.standard_normal((C, self.P)).astype(self.npdt)
        self.u = rng.random(C).astype(self.npdt)
        self.co = COracle(dims, acts, lik, self.x.astype(np.float64), self.y.astype(np.float64), self.mu, self.sigma,
                          dtype=np.float64, bias=self.bias, nthreads=4)
        self.rt, self.at = (1e-9, 1e-9) if self.f64 else (3e-4, 3e-3)
        self.seed = 5 + C + N

    def plan(self):
        from eeyore_amd import _lib as L
        from eeyore_amd.plan import Plan
        old = L.lib().ey_debug_set_variant(self.opts.get("variant", 0))
        try:
            pl = Plan(self.dims, self.bias, self.acts, self.lik, self.dt, DEV)
        finally:
            L.lib().ey_debug_set_variant(old)
        if "products" in self.opts:
            pl.f32_products = self.opts["products"]
        if "row_waves" in self.opts:
            pl.row_waves = self.opts["row_waves"]
        pl.set_data(torch.tensor(self.x, device=DEV), torch.tensor(self.y, device=DEV))
        pl.set_prior(torch.tensor(self.mu), torch.tensor(self.sigma))
        assert pl.P == self.P and pl.kernel == self.kern, (self.fam, pl.kernel)
        return pl

    def oracle(self, c):
        self.co.temp = float("nan") if self.temp is None else float(self.temp[c])
        return self.co

    def g(self, value, shape=None, readonly=False, dtype=None, row=None):
        dtype = dtype or self.dt
        shape = shape if shape is not None else np.shape(value)
        return Guarded(shape, dtype, value=value, readonly=readonly, row=row)


def _f8(a):
    return np.asarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64).copy()


# ---------------------------------------------------------------------------------------------- the call sequence
def _grow(pl, ca, entry):
    """One call through `entry` at GROW chains: the workspace (and any chain-count-sized state) now has that size."""
    C, P, dt = GROW, ca.P, ca.dt
    th = (0.1 * pl.philox_normal(C, seed=99, it=0)).contiguous()
    temp = None if ca.temp is None else torch.full((C,), 0.8, dtype=dt, device=DEV)
    t = torch.zeros(C, dtype=dt, device=DEV)
    g = torch.zeros(C, P, dtype=dt, device=DEV)
    if entry == "hmc_step":
        pl.hmc_step(th, t, g, STEP, LSTEPS, temp=temp, seed=99, it=1)
    elif entry == "log_target_grad":
        pl.log_target_grad(th, temp=temp)
    elif entry == "leapfrog":
        pl.leapfrog(th, (0.1 * pl.philox_normal(C, seed=99, it=2)).contiguous(), STEP, LSTEPS, temp=temp)
    elif entry == "mala_step":
        pl.mala_step(th, t, g, 1e-4, temp=temp, seed=99, it=3)
    elif entry == "mh_step":
        pl.mh_step(th, t, 1e-3, temp=temp, seed=99, it=4)
    elif entry == "hmc_run":
        pl.hmc_run(th, t, g, STEP, LSTEPS, 1, temp=temp, seed=99, it=5)
    elif entry == "log_lik_rows":
        pl.log_lik_rows(th)
    torch.cuda.synchronize()


def _sequence(pl, ca, grow=False):
    """The seven entry points in order on the plan, every buffer guarded; returns their results (host copies)."""
    C, P, dt = ca.C, ca.P, ca.dt
    h = pl.handle
    res = {}

    def temp_g():
        return None if ca.temp is None else ca.g(ca.temp, readonly=True)

    # the starting target and gradient: the oracle's, in the plan's dtype (the plan computes nothing before the first call)
    t0 = np.array([ca.oracle(c).log_target_grad(ca.th0[c].astype(np.float64))[0] for c in range(C)]).astype(ca.npdt)
    g0 = np.stack([ca.oracle(c).log_target_grad(ca.th0[c].astype(np.float64))[1] for c in range(C)]).astype(ca.npdt)

    # 1. hmc_step on recorded randomness
    if grow:
        _grow(pl, ca, "hmc_step")
    th, t, g = ca.g(ca.th0), ca.g(t0), ca.g(g0)
    p0, u, tp = ca.g(ca.p0, readonly=True), ca.g(ca.u, readonly=True), temp_g()
    out = {k: Guarded((C,), torch.uint8 if k == "accepted" else dt) for k in ("accepted", "rate", "h_cur", "h_prop")}
    o = pl.hmc_step(th.t, t.t, g.t, STEP, LSTEPS, p0=p0.t, u=u.t, temp=None if tp is None else tp.t,
                    out={k: v.t for k, v in out.items()})
    _check(theta=th, target=t, grad=g, p0=p0, u=u, temp=tp, **out)
    res["hmc"] = [th.t, t.t, g.t] + [o[k] for k in ("accepted", "rate", "h_cur", "h_prop")]

    # 2. log_target_grad through the C ABI (Plan allocates its outputs itself)
    if grow:
        _grow(pl, ca, "log_target_grad")
    th2, tp = ca.g(ca.th0, readonly=True), temp_g()
    t2, g2 = Guarded((C,), dt), Guarded((C, P), dt)
    _call("ey_log_target_grad", h, _p(th2.t), _p(None if tp is None else tp.t), C, _p(t2.t), _p(g2.t), _stream())
    _check(theta=th2, temp=tp, target=t2, grad=g2)
    res["ltg"] = [t2.t, g2.t]

    # 3. leapfrog (C ABI: guarded target and gradient)
    if grow:
        _grow(pl, ca, "leapfrog")
    th3, p3, tp = ca.g(ca.th0), ca.g(ca.p0), temp_g()
    t3, g3 = Guarded((C,), dt), Guarded((C, P), dt)
    _call("ey_hmc_leapfrog", h, _p(th3.t), _p(p3.t), ct.c_double(STEP), None, LSTEPS, _p(None if tp is None else tp.t), C,
          _p(t3.t), _p(g3.t), _stream())
    _check(theta=th3, p=p3, temp=tp, target=t3, grad=g3)
    res["leap"] = [th3.t, p3.t, t3.t, g3.t]

    # the target and gradient at th0 as the plan computes them: the starting point of the remaining draws
    tk, gk = t2.t.clone(), g2.t.clone()

    # 4. mala_step on recorded randomness
    if grow:
        _grow(pl, ca, "mala_step")
    th4, t4, g4 = ca.g(ca.th0), ca.g(tk), ca.g(gk)
    z4, u4, tp = ca.g(ca.z, readonly=True), ca.g(ca.u, readonly=True), temp_g()
    out4 = {"accepted": Guarded((C,), torch.uint8), "log_rate": Guarded((C,), dt)}
    o4 = pl.mala_step(th4.t, t4.t, g4.t, 1e-4, z=z4.t, u=u4.t, temp=None if tp is None else tp.t,
                      out={k: v.t for k, v in out4.items()})
    _check(theta=th4, target=t4, grad=g4, z=z4, u=u4, temp=tp, **out4)
    res["mala"] = [th4.t, t4.t, g4.t, o4["accepted"], o4["log_rate"]]

    # 5. random-walk mh_step on recorded randomness
    if grow:
        _grow(pl, ca, "mh_step")
    th5, t5 = ca.g(ca.th0), ca.g(tk)
    z5, u5, tp = ca.g(ca.z, readonly=True), ca.g(ca.u, readonly=True), temp_g()
    out5 = {"accepted": Guarded((C,), torch.uint8), "log_rate": Guarded((C,), dt)}
    o5 = pl.mh_step(th5.t, t5.t, 1e-3, z=z5.t, u=u5.t, temp=None if tp is None else tp.t,
                    out={k: v.t for k, v in out5.items()})
    _check(theta=th5, target=t5, z=z5, u=u5, temp=tp, **out5)
    res["mh"] = [th5.t, t5.t, o5["accepted"], o5["log_rate"]]

    # 6. hmc_run of three iterations with records, on the in-kernel streams
    if grow:
        _grow(pl, ca, "hmc_run")
    n_it = 3
    th6, t6, g6, tp = ca.g(ca.th0), ca.g(tk), ca.g(gk), temp_g()
    smp, tgs = Guarded((n_it, C, P), dt, row=P), Guarded((n_it, C), dt, row=1)
    acr = Guarded((n_it, C), torch.uint8, row=1)
    cnt = Guarded((C,), torch.int32, value=torch.zeros(C, dtype=torch.int32))
    out6 = {"accepted": Guarded((C,), torch.uint8)}
    pl.hmc_run(th6.t, t6.t, g6.t, STEP, LSTEPS, n_it, temp=None if tp is None else tp.t, seed=ca.seed, it=1,
               samples=smp.t, targets=tgs.t, accepted_rec=acr.t, accept_count=cnt.t, out={"accepted": out6["accepted"].t})
    _check(theta=th6, target=t6, grad=g6, temp=tp, samples=smp, targets=tgs, accepted_rec=acr, accept_count=cnt, **out6)
    res["run"] = [th6.t, t6.t, g6.t, smp.t, tgs.t, acr.t, cnt.t, out6["accepted"].t]

    # 7. log_lik_rows (C ABI: guarded rows)
    if grow:
        _grow(pl, ca, "log_lik_rows")
    th7 = ca.g(ca.th0, readonly=True)
    rows = Guarded((C, ca.N), dt)
    _call("ey_log_lik_rows", h, _p(th7.t), None, C, _p(rows.t), _stream())
    _check(theta=th7, rows=rows)
    res["rows"] = [rows.t]
    torch.cuda.synchronize()
    return {k: [v.detach().clone().cpu() for v in vs] for k, vs in res.items()}


def _equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _compare(pl, ca, r):
    """The results of `_sequence` on `pl` against the oracle, chain by chain (tests/test_chain_chunks.py uses it too)."""
    f64, rt, at, C = ca.f64, ca.rt, ca.at, ca.C
    info = (ca.fam, ca.dims, "f64" if f64 else "f32", C, ca.N)

    # 1. hmc_step: decisions outside the margin and the states they lead to
    th, t, g, acc_k, _, _, _ = r["hmc"]
    t0 = np.array([ca.oracle(c).log_target_grad(ca.th0[c].astype(np.float64))[0] for c in range(C)]).astype(ca.npdt)
    g0 = np.stack([ca.oracle(c).log_target_grad(ca.th0[c].astype(np.float64))[1] for c in range(C)]).astype(ca.npdt)
    acc, hc, hp = np.zeros(C, np.uint8), np.zeros(C), np.zeros(C)
    tho = _f8(ca.th0)
    for c in range(C):
        sl = slice(c, c + 1)
        a_, hc_, hp_ = ca.oracle(c).hmc_draw(tho[sl], _f8(t0[sl]), _f8(g0[sl]),
                                             _f8(ca.p0[sl]), _f8(ca.u[sl]), STEP, LSTEPS)
        acc[c], hc[c], hp[c] = a_[0], hc_[0], hp_[0]
    rate = np.minimum(np.exp(np.minimum(hc - hp, 0)), 1)
    margin = 1e-9 if f64 else np.maximum(5e-3, 8 * np.finfo(np.float32).eps * np.abs(hc))
    decided = np.isfinite(hp) & (np.abs(ca.u - rate) > margin)
    got = acc_k.numpy()
    np.testing.assert_array_equal(got[decided], acc[decided], err_msg=str(info))
    same = (got == acc) & np.isfinite(hp)
    np.testing.assert_allclose(th.numpy()[same], tho[same], rtol=rt * 10, atol=at / 10, err_msg=str(info))
    assert np.array_equal(th.numpy()[got == 0], ca.th0[got == 0]), "a rejected chain must keep its state"

    # 2. log_target_grad
    tk, gk = r["ltg"]
    for c in range(C):
        to, go, _, _ = ca.oracle(c).log_target_grad(ca.th0[c].astype(np.float64))
        np.testing.assert_allclose(tk[c].item(), to, rtol=rt, atol=at, err_msg=str(info))
        np.testing.assert_allclose(gk[c].numpy(), go, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(go).max()),
                                   err_msg=str(info))

    # 3. leapfrog: position, momentum, target and gradient at the end of the trajectory
    thl, pll, tl, gl = r["leap"]
    for c in range(C):
        tho_, po_, to, go = ca.oracle(c).leapfrog(ca.th0[c].astype(np.float64), ca.p0[c].astype(np.float64), STEP, LSTEPS)
        np.testing.assert_allclose(thl[c].numpy(), tho_, rtol=rt * 10, atol=at / 10, err_msg=str(info))
        np.testing.assert_allclose(pll[c].numpy(), po_, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(po_).max()),
                                   err_msg=str(info))
        np.testing.assert_allclose(tl[c].item(), to, rtol=rt, atol=at, err_msg=str(info))
        np.testing.assert_allclose(gl[c].numpy(), go, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(go).max()),
                                   err_msg=str(info))

    # 4. / 5. MALA and random-walk MH: log-rates against the oracle, decisions outside the margin, states
    tkn, gkn = _f8(tk), _f8(gk)
    for key, step in (("mala", 1e-4), ("mh", 1e-3)):
        thm = r[key][0].numpy()
        acc_k, lr_k = r[key][-2].numpy(), r[key][-1].numpy()
        tho, lr, acc = _f8(ca.th0), np.zeros(C), np.zeros(C, np.uint8)
        for c in range(C):
            sl = slice(c, c + 1)
            if key == "mala":
                a_, l_ = ca.oracle(c).mala_draw(tho[sl], tkn[sl].copy(), gkn[sl].copy(), _f8(ca.z[sl]), _f8(ca.u[sl]), step)
            else:
                a_, l_ = ca.oracle(c).mh_draw(tho[sl], tkn[sl].copy(), _f8(ca.z[sl]), _f8(ca.u[sl]), step)
            acc[c], lr[c] = a_[0], l_[0]
        ok = np.isfinite(lr)
        tol = (1e-7 if f64 else F32_DECISION_TOL) * np.maximum(1.0, np.abs(lr)) + (0 if f64 else 8e-7 * np.abs(hc))
        assert (np.abs(lr_k[ok] - lr[ok]) <= tol[ok]).all(), (key, info, lr_k, lr)
        decided = ok & (np.abs(np.log(ca.u.astype(np.float64)) - lr) > tol)
        np.testing.assert_array_equal(acc_k[decided], acc[decided], err_msg=str((key, info)))
        same = acc_k == acc
        np.testing.assert_allclose(thm[same], tho[same], rtol=rt * 10, atol=at / 10, err_msg=str((key, info)))

    # 6. hmc_run: bit-equal to three hmc_step calls on the in-kernel streams from the same state
    th6, t6, g6, smp, tgs, acr, cnt, acc6 = r["run"]
    temp = None if ca.temp is None else torch.tensor(ca.temp, device=DEV)
    a = [torch.tensor(ca.th0, device=DEV), tk.to(DEV), gk.to(DEV)]
    for i in range(3):
        o = pl.hmc_step(*a, STEP, LSTEPS, temp=temp, seed=ca.seed, it=1 + i)
        assert _equal_bits(smp[i], a[0].cpu()), (i, info)
        assert _equal_bits(tgs[i], a[1].cpu()), (i, info)
        assert torch.equal(acr[i], o["accepted"].cpu()), (i, info)
    assert _equal_bits(th6, a[0].cpu()) and _equal_bits(t6, a[1].cpu()) and _equal_bits(g6, a[2].cpu()), info
    assert torch.equal(acc6, o["accepted"].cpu()) and torch.equal(cnt, acr.sum(0, dtype=torch.int32)), info

    # 7. log_lik_rows: row sums are the (untempered) log-likelihood
    rows = r["rows"][0].numpy()
    for c in range(C):
        ca.co.temp = float("nan")
        _, _, lk, _ = ca.co.log_target_grad(ca.th0[c].astype(np.float64), want_grad=False)
        np.testing.assert_allclose(rows[c].sum(), lk, rtol=1e-9 if f64 else 2e-4, atol=1e-9 if f64 else 2e-3,
                                   err_msg=str(info))


@pytest.mark.parametrize("fam,dims,acts,bias,lik,tag,kern,opts,C,N", CASES)
def test_small_batch_vs_oracle(fam, dims, acts, bias, lik, tag, kern, opts, C, N):
    ca = Case(fam, dims, acts, bias, lik, tag, kern, opts, C, N)
    pl = ca.plan()
    r = _sequence(pl, ca)
    _compare(pl, ca, r)
    info = (fam, dims, tag, C, N)

    # independence from workspace history: a second plan, each call behind a GROW-chain call through the same entry point
    if C == 1:
        pl2 = ca.plan()
        r2 = _sequence(pl2, ca, grow=True)
        if fam not in HISTORY_EXEMPT:
            for k in r:
                for i, (u_, v_) in enumerate(zip(r[k], r2[k])):
                    assert _equal_bits(u_, v_), f"{info}: {k}[{i}] after a {GROW}-chain call differs from a fresh plan's"


# ----------------------------------------------------------------------------------------- the sampler, one chain
def _narrow_model():
    from torch.distributions import Normal
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    model = mlp.MLP(loss=loss_functions['multiclass_classification'],
                    hparams=mlp.Hyperparameters(dims=[16, 32, 32, 32, 3], bias=4 * [True],
                                                activations=[torch.sigmoid, torch.sigmoid, torch.sigmoid, None]),
                    dtype=torch.float32, device=DEV)
    P = model.num_params()
    model.prior = Normal(torch.zeros(P, device=DEV), torch.full((P,), 3.0, device=DEV).sqrt())
    return model


def test_single_chain_hmc_sampler_on_minibatches_vs_oracle():
    """samplers.HMC with theta0 of shape [P] on MLP(16-32-32-32-3) f32 (k_mid32), minibatches of 10 rows over 95 (the last
    one 5), three epochs on the in-kernel streams: every iteration replayed by the oracle on that iteration's batch from
    the recorded previous state with the same momentum and uniform.  Then the same run on a model whose plan first served
    a 1024-chain call must give the same bits."""
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.plan import Plan
    from eeyore_amd.samplers import HMC
    dims, rows, bs, epochs, seed, step, L = [16, 32, 32, 32, 3], 95, 10, 3, 7, 0.2, 4
    rng = np.random.default_rng(12)
    centres = rng.standard_normal((3, 16))
    labels = np.arange(rows) % 3
    x = (centres[labels] + 0.7 * rng.standard_normal((rows, 16))).astype(np.float32)
    y = np.eye(3, dtype=np.float32)[labels]
    loader = DataLoader(XYDataset(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)), batch_size=bs, shuffle=False)
    batches = [(x[i:i + bs], y[i:i + bs]) for i in range(0, rows, bs)]
    assert len(batches) == 10 and len(batches[-1][0]) == 5

    def run(model):
        P = model.num_params()
        th0 = (0.3 * torch.tensor(np.random.default_rng(4).standard_normal(P), dtype=torch.float32, device=DEV))
        s = HMC(model, theta0=th0, dataloader=loader, step=step, num_steps=L, rng='philox', seed=seed)
        s.run(num_epochs=epochs, num_burnin_epochs=0)
        assert model._plan(None, None).kernel == "bgemm"
        ch = s.get_chain().vals
        return th0.cpu().numpy(), [v.cpu() for v in ch['sample']], list(ch['accepted']), [v.cpu() for v in ch['target_val']]

    th0, smp, accs, tvs = run(_narrow_model())
    n = epochs * len(batches)
    assert len(smp) == n
    P = th0.size
    sigma = np.full(P, np.sqrt(3.0))
    streams = Plan(dims, [1] * 4, [1, 1, 1, 0], 1, torch.float32, DEV)   # only for its Philox streams (P, f32)
    oracles = [COracle(dims, [1, 1, 1, 0], 1, xb.astype(np.float64), yb.astype(np.float64), 0.0, sigma, dtype=np.float64,
                       nthreads=4) for xb, yb in batches]
    prev, n_acc, n_dec = th0.astype(np.float64), 0, 0
    for i in range(n):
        co = oracles[i % len(batches)]
        p0 = _f8(streams.philox_normal(1, seed=seed, it=i))
        u = _f8(streams.philox_uniform(1, seed=seed, it=i))
        tho = prev[None].copy()
        tv, gv, _, _ = co.log_target_grad(tho[0])
        acc, hc, hp = co.hmc_draw(tho, np.array([tv]), gv[None].copy(), p0, u, step, L)
        rate = np.minimum(np.exp(np.minimum(hc - hp, 0)), 1)
        margin = np.maximum(5e-3, 8 * np.finfo(np.float32).eps * np.abs(hc))
        got = smp[i].numpy()
        if np.isfinite(hp[0]) and abs(u[0] - rate[0]) > margin[0]:
            n_dec += 1
            assert accs[i] == acc[0], (i, accs[i], acc[0], rate[0], u[0])
        if accs[i] == acc[0]:
            np.testing.assert_allclose(got, tho[0], rtol=3e-3, atol=3e-4, err_msg=f"iteration {i}")
        n_acc += accs[i]
        prev = got.astype(np.float64)
    assert n_dec >= n - 3 and 3 <= n_acc <= n - 3, (n_dec, n_acc)  # decisions checked, accepts and rejects both seen

    # the same run on a model whose plan first served a 1024-chain call
    model2 = _narrow_model()
    pl2 = model2._plan(*next(iter(loader)))
    big = (0.3 * pl2.philox_normal(GROW, seed=1, it=0)).contiguous()
    t, g = pl2.log_target_grad(big)
    pl2.hmc_step(big, t, g, step, L, seed=1, it=1)
    torch.cuda.synchronize()
    th0b, smp2, accs2, tvs2 = run(model2)
    assert np.array_equal(th0b, th0) and accs2 == accs
    for i in range(n):
        assert _equal_bits(smp2[i], smp[i]) and _equal_bits(tvs2[i], tvs[i]), i
