"""The chain-chunk loops of the layerwise path ("bgemm", ey_large.hip) against the f64 C oracle.

The path runs a call's chains in chunks of chunk_size() chains -- min(16 GiB / activations per chain, 32768) -- with one
set of launches per chunk, every pointer and the Philox chain index moved on by the chunk's first chain c0.  No other GPU
test has more chains than one chunk holds, so c0 is 0 everywhere else.  The plan option EY_OPT_MAX_CHUNK_CHAINS
(Plan.max_chunk_chains) bounds a chunk: 7 chains at a bound of 3 run as 3 + 3 + 1, so every `+ c0` offset, the workspace
carve sized by 3 chains but used by 1, and `chain_offset + c0` are exercised; 4 chains at a bound of 4 are the control (one
chunk, the bound exactly met).

Criterion 1: every chain's outputs against the oracle, with the harness, tolerances and decision margins of
tests/test_small_batches.py (`_sequence` / `_compare`), plus the entries and inputs that file does not use: the lik and
prior parts, the network outputs, per-chain steps, a chain offset (2**33 + 5 once) and the in-kernel Philox streams, and a
recorded mala_run.  The inputs differ per chain (temperature, step, momentum, stream), so a wrong offset moves a value; every
buffer lies between canary chains that must survive, and no output of a chain behind the first chunk may still hold canary.
Criterion 2: the same calls on a plan with the option at 0 give the same bits in every output (a workgroup of this path
sees one chain, so a chain's arithmetic cannot depend on its launch).

The C oracle has no network-output entry: ey_forward is compared with the f64 torch restatement of the reference's forward
(tests/prior_restatement.py).  Only MLP(784-128-10) is beyond the generic kernels' LDS image, so only there does ey_forward
run the layerwise loop (large_forward); the smaller models' outputs come from the generic kernel and are checked all the same.

test_default_rule_second_chunk runs without the option: 32768 + 3 chains of a forced-layerwise MLP(2-2-1), so the first
chunk has gridDim.z = 32768 and the default rule's second pass serves the last three chains."""
import ctypes as ct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle.c_oracle import COracle
from tests.prior_restatement import Target
from tests.test_gpu_parity import F32_DECISION_TOL
from tests.test_small_batches import (DEV, FAMILIES, LSTEPS, STEP, Case, Guarded, _bits, _call, _check, _compare,
                                      _equal_bits, _f8, _p, _sequence, _stream)

pytestmark = pytest.mark.gpu

BIG_OFFSET = 2 ** 33 + 5
N_IT = 3
MALA_STEP, MH_SCALE = 1e-4, 1e-3

# the layerwise rows of tests/test_small_batches.py FAMILIES (family, dims, dtype) ...
_WANTED = [("layerwise", [5, 32, 1], "f32"), ("layerwise", [5, 32, 1], "f64"), ("layerwise", [6, 16, 10], "f32"),
           ("layerwise", [6, 16, 10], "f64"), ("layerwise", [784, 128, 10], "f32"), ("layerwise", [784, 128, 10], "f64"),
           ("k_mid32", [16, 32, 32, 32, 3], "f32"), ("k_mid32", [64, 32, 32, 10], "f32"), ("k_mid", [10, 100, 10], "f32")]
ROWS = [r for w in _WANTED for r in FAMILIES if (r[0], r[1], r[5]) == w]
assert len(ROWS) == len(_WANTED)
# ... and both branches of `fuse` in large_hmc with and without k_tail.  In f32 the plain rows above take the fused last
# layer k_tail (tail_ok: at most 10 outputs, a last hidden width of 16 / 32 / 128) and the leapfrog update fused into the
# gradient kernels; variant bit 7 keeps the update in k_leap (the separate-leapfrog branch), bit 6 switches k_tail off
# (k_loss and the narrow products instead, still fused).  f64 has neither k_tail nor the fused update.
ROWS += [("layerwise-sepleap", [6, 16, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 16384 | 128), None, None),
         ("layerwise-sepleap", [784, 128, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 16384 | 128), None, None),
         ("layerwise-notail", [6, 16, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 16384 | 64), None, None),
         ("layerwise-notail", [784, 128, 10], [1, 0], None, 1, "f32", "bgemm", dict(variant=16 | 16384 | 64), None, None)]
SHAPES = [(7, 3), (4, 4)]     # chains, bound: chunks of 3 + 3 + 1; one chunk with the bound exactly met

CASES = [pytest.param(fam, dims, acts, bias, lik, tag, kern, opts, C, cap, N,
                      id=f"{fam}-{'x'.join(map(str, dims))}-{tag}-C{C}-cap{cap}-N{N}")
         for fam, dims, acts, bias, lik, tag, kern, opts, _, _ in ROWS for C, cap in SHAPES for N in (10, 40)]


def _offset(ca):
    return BIG_OFFSET if ca.dims == [6, 16, 10] else 3


def _steps(ca, base):
    """A step per chain, in the plan's dtype (the oracle takes the rounded value)."""
    return (base * (0.6 + 0.15 * np.arange(ca.C))).astype(ca.npdt)


def _each(ca, fn):
    """[fn(c, oracle of chain c) for every chain], the chains side by side: an oracle object per chain (its own
    temperature and work buffer), and the C calls release the interpreter lock."""
    if not hasattr(ca, "per_chain"):
        ca.per_chain = [COracle(ca.dims, ca.acts, ca.lik, ca.x.astype(np.float64), ca.y.astype(np.float64), ca.mu, ca.sigma,
                                dtype=np.float64, bias=ca.bias, temperature=float(ca.temp[c])) for c in range(ca.C)]
    with ThreadPoolExecutor(min(ca.C, 8)) as ex:
        return list(ex.map(lambda c: fn(c, ca.per_chain[c]), range(ca.C)))


def _start(ca):
    """Target and gradient at th0: the oracle's, in the plan's dtype (as `_sequence` starts its draws)."""
    if not hasattr(ca, "start"):
        tg = _each(ca, lambda c, o: o.log_target_grad(ca.th0[c].astype(np.float64))[:2])
        ca.start = np.array([t for t, _ in tg]).astype(ca.npdt), np.stack([g for _, g in tg]).astype(ca.npdt)
    return ca.start[0].copy(), ca.start[1].copy()


def _extras(pl, ca):
    """The entries and inputs `_sequence` leaves out, every buffer guarded; returns host copies."""
    C, P, N, dt, h = ca.C, ca.P, ca.N, ca.dt, pl.handle
    off, seed = _offset(ca), ca.seed + 100
    res = {}
    t0, g0 = _start(ca)
    sv_h, sv_m = _steps(ca, STEP), _steps(ca, MALA_STEP)

    def temp_g():
        return ca.g(ca.temp, readonly=True)

    # a. the lik and prior parts (ey_log_target)
    th, tp = ca.g(ca.th0, readonly=True), temp_g()
    lik, pri = Guarded((C,), dt), Guarded((C,), dt)
    _call("ey_log_target", h, _p(th.t), _p(tp.t), C, _p(lik.t), _p(pri.t), _stream())
    _check(theta=th, temp=tp, lik=lik, prior=pri)
    res["parts"] = [lik.t, pri.t]

    # b. the network outputs (ey_forward)
    th = ca.g(ca.th0, readonly=True)
    out = Guarded((C, N, ca.dims[-1]), dt)
    _call("ey_forward", h, _p(th.t), C, _p(out.t), _stream())
    _check(theta=th, out=out)
    res["forward"] = [out.t]

    # c. hmc_step on the in-kernel streams, a step per chain, a chain offset
    th, t, g, sv, tp = ca.g(ca.th0), ca.g(t0), ca.g(g0), ca.g(sv_h, readonly=True), temp_g()
    o = {k: Guarded((C,), torch.uint8 if k == "accepted" else dt) for k in ("accepted", "rate", "h_cur", "h_prop")}
    pl.hmc_step(th.t, t.t, g.t, STEP, LSTEPS, step_vec=sv.t, temp=tp.t, seed=seed, it=1, chain_offset=off,
                out={k: v.t for k, v in o.items()})
    _check(theta=th, target=t, grad=g, step_vec=sv, temp=tp, **o)
    res["hmc"] = [th.t, t.t, g.t] + [o[k].t for k in ("accepted", "rate", "h_cur", "h_prop")]

    # d. leapfrog with a step per chain
    th, p, sv, tp = ca.g(ca.th0), ca.g(ca.p0), ca.g(sv_h, readonly=True), temp_g()
    t, g = Guarded((C,), dt), Guarded((C, P), dt)
    _call("ey_hmc_leapfrog", h, _p(th.t), _p(p.t), ct.c_double(STEP), _p(sv.t), LSTEPS, _p(tp.t), C, _p(t.t), _p(g.t),
          _stream())
    _check(theta=th, p=p, step_vec=sv, temp=tp, target=t, grad=g)
    res["leap"] = [th.t, p.t, t.t, g.t]

    # e. mala_step and mh_step on the in-kernel streams
    th, t, g, sv, tp = ca.g(ca.th0), ca.g(t0), ca.g(g0), ca.g(sv_m, readonly=True), temp_g()
    o = {"accepted": Guarded((C,), torch.uint8), "log_rate": Guarded((C,), dt)}
    pl.mala_step(th.t, t.t, g.t, MALA_STEP, step_vec=sv.t, temp=tp.t, seed=seed, it=2, chain_offset=off,
                 out={k: v.t for k, v in o.items()})
    _check(theta=th, target=t, grad=g, step_vec=sv, temp=tp, **o)
    res["mala"] = [th.t, t.t, g.t, o["accepted"].t, o["log_rate"].t]
    th, t, tp = ca.g(ca.th0), ca.g(t0), temp_g()
    o = {"accepted": Guarded((C,), torch.uint8), "log_rate": Guarded((C,), dt)}
    pl.mh_step(th.t, t.t, MH_SCALE, temp=tp.t, seed=seed, it=3, chain_offset=off, out={k: v.t for k, v in o.items()})
    _check(theta=th, target=t, temp=tp, **o)
    res["mh"] = [th.t, t.t, o["accepted"].t, o["log_rate"].t]

    # f. / g. recorded runs of three iterations: hmc_run with a step per chain and the offset, mala_run likewise
    for key, first in (("hmc_run", 10), ("mala_run", 20)):
        th, t, g, tp = ca.g(ca.th0), ca.g(t0), ca.g(g0), temp_g()
        sv = ca.g(sv_h if key == "hmc_run" else sv_m, readonly=True)
        smp, tgs = Guarded((N_IT, C, P), dt, row=P), Guarded((N_IT, C), dt, row=1)
        acr = Guarded((N_IT, C), torch.uint8, row=1)
        cnt = Guarded((C,), torch.int32, value=torch.zeros(C, dtype=torch.int32))
        acc = Guarded((C,), torch.uint8)
        kw = dict(step_vec=sv.t, temp=tp.t, seed=seed, it=first, chain_offset=off, samples=smp.t, targets=tgs.t,
                  accepted_rec=acr.t, accept_count=cnt.t, out={"accepted": acc.t})
        if key == "hmc_run":
            pl.hmc_run(th.t, t.t, g.t, STEP, LSTEPS, N_IT, **kw)
        else:
            pl.mala_run(th.t, t.t, g.t, MALA_STEP, N_IT, **kw)
        _check(theta=th, target=t, grad=g, step_vec=sv, temp=tp, samples=smp, targets=tgs, accepted_rec=acr,
               accept_count=cnt, accepted=acc)
        res[key] = [th.t, t.t, g.t, smp.t, tgs.t, acr.t, cnt.t, acc.t]
    torch.cuda.synchronize()
    return {k: [v.detach().clone().cpu() for v in vs] for k, vs in res.items()}


# in-margin decisions seen per case (recorded for the pull request's summary, printed with -s)
IN_MARGIN = {}


def _hmc_margin(ca, hc):
    return 1e-9 if ca.f64 else np.maximum(5e-3, 8 * np.finfo(np.float32).eps * np.abs(hc))


def _log_rate_tol(ca, lr, hc):
    return (1e-7 if ca.f64 else F32_DECISION_TOL) * np.maximum(1.0, np.abs(lr)) + (0 if ca.f64 else 8e-7 * np.abs(hc))


def _hmc_draws(ca, pl, th, t, g, p0, u, sv):
    """The oracle's HMC draw of every chain (its own temperature and step) in place on f64 th, t, g."""
    def one(c, o):
        sl = slice(c, c + 1)
        return [v[0] for v in o.hmc_draw(th[sl], t[sl], g[sl], _f8(p0[sl]), _f8(u[sl]), float(sv[c]), LSTEPS)]
    r = _each(ca, one)
    return (np.array([a for a, _, _ in r], np.uint8), np.array([b for _, b, _ in r], np.float64),
            np.array([c for _, _, c in r], np.float64))


def _mala_mh_draws(ca, key, th, t, g, z, u, sv):
    """The oracle's MALA (its own step per chain) or random-walk MH draw of every chain in place on f64 th, t, g."""
    def one(c, o):
        sl = slice(c, c + 1)
        if key == "mala":
            a_, l_ = o.mala_draw(th[sl], t[sl], g[sl], _f8(z[sl]), _f8(u[sl]), float(sv[c]))
        else:
            a_, l_ = o.mh_draw(th[sl], t[sl], _f8(z[sl]), _f8(u[sl]), MH_SCALE)
        return a_[0], l_[0]
    r = _each(ca, one)
    return np.array([a for a, _ in r], np.uint8), np.array([b for _, b in r], np.float64)


def _streams(pl, ca, it):
    off, seed = _offset(ca), ca.seed + 100
    return (pl.philox_normal(ca.C, seed=seed, it=it, chain_offset=off).cpu().numpy(),
            pl.philox_uniform(ca.C, seed=seed, it=it, chain_offset=off).cpu().numpy())


def _compare_extras(pl, ca, r, tag):
    C, f64, rt, at = ca.C, ca.f64, ca.rt, ca.at
    info = (tag, ca.fam, ca.dims, "f64" if f64 else "f32", C, ca.N)
    t0, g0 = _start(ca)
    sv_h, sv_m = _steps(ca, STEP), _steps(ca, MALA_STEP)
    margins = IN_MARGIN.setdefault((ca.fam, tuple(ca.dims), info[3], C, ca.N), {})

    # a. lik and prior, both tempered (bayesian_model.py:33-34,48-49)
    lik, pri = (v.numpy() for v in r["parts"])
    for c, (_, _, lo, po_) in enumerate(_each(ca, lambda c, o: o.log_target_grad(ca.th0[c].astype(np.float64), want_grad=False))):
        np.testing.assert_allclose(lik[c], lo, rtol=rt, atol=at, err_msg=str(info))
        np.testing.assert_allclose(pri[c], po_, rtol=rt, atol=at, err_msg=str(info))

    # b. the network outputs
    ref = Target(ca.dims, ca.acts, ca.lik, ca.x, ca.y, None, bias=ca.bias)
    out = r["forward"][0].numpy()
    for c in range(C):
        want = ref.forward(torch.tensor(ca.th0[c].astype(np.float64))).numpy()
        np.testing.assert_allclose(out[c], want, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(want).max()),
                                   err_msg=str(info))

    # c. hmc_step on the in-kernel streams
    p0, u = _streams(pl, ca, 1)
    th, t, g, acc_k = r["hmc"][0].numpy(), r["hmc"][1].numpy(), r["hmc"][2].numpy(), r["hmc"][3].numpy()
    tho, to, go = _f8(ca.th0), _f8(t0), _f8(g0)
    acc, hc, hp = _hmc_draws(ca, pl, tho, to, go, p0, u, sv_h)
    rate = np.minimum(np.exp(np.minimum(hc - hp, 0)), 1)
    decided = np.isfinite(hp) & (np.abs(u - rate) > _hmc_margin(ca, hc))
    margins["hmc_step"] = int((~decided).sum())
    np.testing.assert_array_equal(acc_k[decided], acc[decided], err_msg=str(info))
    same = (acc_k == acc) & np.isfinite(hp)
    np.testing.assert_allclose(th[same], tho[same], rtol=rt * 10, atol=at / 10, err_msg=str(info))
    np.testing.assert_allclose(t[same], to[same], rtol=rt, atol=at, err_msg=str(info))
    assert np.array_equal(th[acc_k == 0], ca.th0[acc_k == 0]), "a rejected chain must keep its state"
    np.testing.assert_allclose(r["hmc"][5].numpy(), hc, rtol=rt, atol=at, err_msg=str(info))

    # d. leapfrog with a step per chain
    thl, pll, tl, gl = (v.numpy() for v in r["leap"])
    for c, (tho_, po_, to_, go_) in enumerate(_each(ca, lambda c, o: o.leapfrog(
            ca.th0[c].astype(np.float64), ca.p0[c].astype(np.float64), float(sv_h[c]), LSTEPS))):
        np.testing.assert_allclose(thl[c], tho_, rtol=rt * 10, atol=at / 10, err_msg=str(info))
        np.testing.assert_allclose(pll[c], po_, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(po_).max()), err_msg=str(info))
        np.testing.assert_allclose(tl[c], to_, rtol=rt, atol=at, err_msg=str(info))
        np.testing.assert_allclose(gl[c], go_, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(go_).max()), err_msg=str(info))

    # e. MALA and random-walk MH on the in-kernel streams
    for key, it in (("mala", 2), ("mh", 3)):
        z, u = _streams(pl, ca, it)
        thm, acc_k, lr_k = r[key][0].numpy(), r[key][-2].numpy(), r[key][-1].numpy()
        tho = _f8(ca.th0)
        acc, lr = _mala_mh_draws(ca, key, tho, _f8(t0), _f8(g0), z, u, sv_m)
        ok = np.isfinite(lr)
        tol = _log_rate_tol(ca, lr, hc)
        assert (np.abs(lr_k[ok] - lr[ok]) <= tol[ok]).all(), (key, info, lr_k, lr)
        decided = ok & (np.abs(np.log(u.astype(np.float64)) - lr) > tol)
        margins[key + "_step"] = int((~decided).sum())
        np.testing.assert_array_equal(acc_k[decided], acc[decided], err_msg=str((key, info)))
        same = acc_k == acc
        np.testing.assert_allclose(thm[same], tho[same], rtol=rt * 10, atol=at / 10, err_msg=str((key, info)))

    # f. / g. the recorded runs: every iteration replayed by the oracle from the recorded previous state
    for key, first, sv in (("hmc_run", 10, sv_h), ("mala_run", 20, sv_m)):
        th_e, t_e, g_e, smp, tgs, acr, cnt, acc_e = r[key]
        prev_th, n_in = _f8(ca.th0), 0
        for i in range(N_IT):
            z, u = _streams(pl, ca, first + i)
            tho = prev_th.copy()
            tg = _each(ca, lambda c, o: o.log_target_grad(tho[c])[:2])
            to, go = np.array([a for a, _ in tg], dtype=np.float64), np.stack([b for _, b in tg]).astype(np.float64)
            if key == "hmc_run":
                acc, hc_i, hp = _hmc_draws(ca, pl, tho, to, go, z, u, sv)
                rate = np.minimum(np.exp(np.minimum(hc_i - hp, 0)), 1)
                decided = np.isfinite(hp) & (np.abs(u - rate) > _hmc_margin(ca, hc_i))
            else:
                acc, lr = _mala_mh_draws(ca, "mala", tho, to, go, z, u, sv)
                decided = np.isfinite(lr) & (np.abs(np.log(u.astype(np.float64)) - lr) > _log_rate_tol(ca, lr, hc))
            n_in += int((~decided).sum())
            got = acr[i].numpy()
            assert set(np.unique(got)) <= {0, 1}, (key, i, info)
            np.testing.assert_array_equal(got[decided], acc[decided], err_msg=str((key, i, info)))
            same = got == acc
            np.testing.assert_allclose(smp[i].numpy()[same], tho[same], rtol=rt * 10, atol=at / 10, err_msg=str((key, i, info)))
            np.testing.assert_allclose(tgs[i].numpy()[same], to[same], rtol=rt, atol=at, err_msg=str((key, i, info)))
            assert np.array_equal(smp[i].numpy()[got == 0], prev_th.astype(ca.npdt)[got == 0]), (key, i, info)
            prev_th = _f8(smp[i])
        margins[key] = n_in
        assert _equal_bits(th_e, smp[N_IT - 1]) and _equal_bits(t_e, tgs[N_IT - 1]) and torch.equal(acc_e, acr[N_IT - 1]), info
        assert torch.equal(cnt, acr.sum(0, dtype=torch.int32)), info
        assert torch.isfinite(g_e).all(), info
    if f64:  # (a margin of 1e-9: the seeds leave no decision inside it)
        assert not any(margins.values()), (info, margins)


def _chunks_were_served(ca, cap, r, rx):
    """Chains behind the first chunk hold results of their own: no canary (NaN, 0xAB), and no two chains' values alike."""
    for res in (r, rx):
        for key, vs in res.items():
            for v in vs:
                tail = v[cap:] if v.shape[0] == ca.C else v[:, cap:]    # (records are [n_it, C, ...])
                if v.dtype.is_floating_point:
                    assert torch.isfinite(tail).all(), (key, "canary or non-finite values behind the first chunk")
                elif v.dtype == torch.uint8:
                    assert (tail <= 1).all(), (key, "canary bytes behind the first chunk")
    for name, v in (("target", r["ltg"][0]), ("lik", rx["parts"][0]), ("prior", rx["parts"][1]), ("rows", r["rows"][0]),
                    ("grad", r["ltg"][1]), ("forward", rx["forward"][0]), ("leapfrog", rx["leap"][0])):
        flat = v.reshape(ca.C, -1)
        for a in range(ca.C):
            for b in range(a + 1, ca.C):
                assert not torch.equal(flat[a], flat[b]), (name, a, b, "two chains with the same values")


@pytest.mark.parametrize("fam,dims,acts,bias,lik,tag,kern,opts,C,cap,N", CASES)
def test_chunked_chains_vs_oracle(fam, dims, acts, bias, lik, tag, kern, opts, C, cap, N):
    ca = Case(fam, dims, acts, bias, lik, tag, kern, opts, C, N)
    pl = ca.plan()
    assert pl.max_chunk_chains == 0
    pl.max_chunk_chains = cap
    assert pl.max_chunk_chains == cap
    r, rx = _sequence(pl, ca), _extras(pl, ca)
    # criterion 1: the oracle
    _compare(pl, ca, r)
    _compare_extras(pl, ca, rx, "chunked")
    _chunks_were_served(ca, cap, r, rx)
    print("in-margin decisions", (fam, dims, tag, C, cap, N), IN_MARGIN.get((fam, tuple(dims), tag, C, N)))
    # criterion 2: the same bits as one chunk
    pl0 = ca.plan()
    assert pl0.max_chunk_chains == 0
    r0, rx0 = _sequence(pl0, ca), _extras(pl0, ca)
    for a, b in ((r, r0), (rx, rx0)):
        for k in a:
            for i, (u_, v_) in enumerate(zip(a[k], b[k])):
                assert _equal_bits(u_, v_), f"{(fam, dims, tag, C, cap, N)}: {k}[{i}] in chunks of {cap} differs from one chunk's"


def test_option_surface():
    from eeyore_amd import _lib as L
    ca = Case(*ROWS[0][:8], 2, 4)
    pl, other = ca.plan(), ca.plan()
    assert pl.max_chunk_chains == 0                      # the default of a new plan: the path's own rule
    for k in (1, 3, 32768, 2 ** 31 - 1, 0):
        pl.max_chunk_chains = k
        assert pl.max_chunk_chains == k and other.max_chunk_chains == 0
    pl.max_chunk_chains = 5
    for bad in (-1, -2 ** 31):
        with pytest.raises(ValueError, match="EY_OPT_MAX_CHUNK_CHAINS"):
            pl.max_chunk_chains = bad
        assert L.lib().ey_plan_set_option(pl.handle, L.EY_OPT_MAX_CHUNK_CHAINS, bad) == -1
        assert pl.max_chunk_chains == 5                  # a refused value changes nothing


# -------------------------------------------------------------------------------------------------- the real cap
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_default_rule_second_chunk(tag):
    """No option: MLP(2-2-1) forced layerwise, N = 4, 32768 + 3 chains.  chunk_size() caps a chunk at 32768 chains
    (gridDim.z), so the call is one chunk of 32768 and one of 3.  Value and gradient of every chain against the oracle, one
    HMC draw on the in-kernel streams (decisions outside the margin, states), and the last three chains bit for bit against
    a three-chain call at chain_offset = 32768."""
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import Plan
    f64 = tag == "f64"
    npdt, dt = (np.float64, torch.float64) if f64 else (np.float32, torch.float32)
    dims, acts, N, C, cap = [2, 2, 1], [2, 1], 4, 32768 + 3, 32768
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N, 2)).astype(npdt)
    y = (rng.random((N, 1)) < 0.5).astype(npdt)
    old = L.lib().ey_debug_set_variant(16)
    try:
        pl = Plan(dims, [1, 1], acts, 0, dt, DEV)
    finally:
        L.lib().ey_debug_set_variant(old)
    pl.set_data(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV))
    P = pl.P
    mu = (0.1 * rng.standard_normal(P)).astype(npdt).astype(np.float64)
    sigma = (0.5 + rng.random(P)).astype(npdt).astype(np.float64)
    pl.set_prior(torch.tensor(mu), torch.tensor(sigma))
    assert pl.kernel == "bgemm" and pl.max_chunk_chains == 0 and P == 9
    co = COracle(dims, acts, 0, x.astype(np.float64), y.astype(np.float64), mu, sigma, dtype=np.float64, nthreads=8)
    rt, at = (1e-9, 1e-9) if f64 else (3e-4, 3e-3)
    th0 = rng.standard_normal((C, P)).astype(npdt)
    step, seed = 0.5, 21      # (the oracle accepts about 86 % of such draws: thousands of rejections among the chains)

    th = Guarded((C, P), dt, value=th0, readonly=True)
    t, g = Guarded((C,), dt), Guarded((C, P), dt)
    _call("ey_log_target_grad", pl.handle, _p(th.t), None, C, _p(t.t), _p(g.t), _stream())
    _check(theta=th, target=t, grad=g)
    tk, gk = t.t.clone(), g.t.clone()
    to, go = np.zeros(C), np.zeros((C, P))
    for c in range(C):
        to[c], go[c], _, _ = co.log_target_grad(th0[c].astype(np.float64))
    np.testing.assert_allclose(tk.cpu().numpy(), to, rtol=rt, atol=at)
    np.testing.assert_allclose(gk.cpu().numpy(), go, rtol=rt * 10, atol=at / 10 * max(1.0, np.abs(go).max()))
    assert tk[cap:].unique().numel() == 3

    ths, ts, gs = Guarded((C, P), dt, value=th0), Guarded((C,), dt, value=tk), Guarded((C, P), dt, value=gk)
    o = {k: Guarded((C,), torch.uint8 if k == "accepted" else dt) for k in ("accepted", "rate", "h_cur", "h_prop")}
    pl.hmc_step(ths.t, ts.t, gs.t, step, LSTEPS, seed=seed, it=1, out={k: v.t for k, v in o.items()})
    _check(theta=ths, target=ts, grad=gs, **o)
    p0 = pl.philox_normal(C, seed=seed, it=1).cpu().numpy().astype(np.float64)
    u = pl.philox_uniform(C, seed=seed, it=1).cpu().numpy().astype(np.float64)
    tho, tvo, gvo = _f8(th0), _f8(tk), _f8(gk)
    acc, hc, hp = co.hmc_draw(tho, tvo, gvo, p0, u, step, LSTEPS)
    rate = np.minimum(np.exp(np.minimum(hc - hp, 0)), 1)
    margin = 1e-9 if f64 else np.maximum(5e-3, 8 * np.finfo(np.float32).eps * np.abs(hc))
    decided = np.isfinite(hp) & (np.abs(u - rate) > margin)
    got = o["accepted"].t.cpu().numpy()
    print("default rule", tag, "in-margin decisions", int((~decided).sum()), "of", C, "accepted", int(got.sum()))
    assert set(np.unique(got)) <= {0, 1}
    if f64:
        assert decided.all()
    np.testing.assert_array_equal(got[decided], acc[decided])
    same = (got == acc) & np.isfinite(hp)
    np.testing.assert_allclose(ths.t.cpu().numpy()[same], tho[same], rtol=rt * 10, atol=at / 10)
    np.testing.assert_allclose(ts.t.cpu().numpy()[same], tvo[same], rtol=rt, atol=at)
    assert 0.5 * C < got.sum() < 0.95 * C

    # the last three chains on their own, at the chain offset the second chunk gives them
    t3, g3 = pl.log_target_grad(torch.tensor(th0[cap:], device=DEV))
    assert _equal_bits(t3, tk[cap:]) and _equal_bits(g3, gk[cap:])
    a = [torch.tensor(th0[cap:], device=DEV), tk[cap:].clone(), gk[cap:].clone()]
    o3 = pl.hmc_step(*a, step, LSTEPS, seed=seed, it=1, chain_offset=cap)
    assert _equal_bits(a[0], ths.t[cap:]) and _equal_bits(a[1], ts.t[cap:]) and _equal_bits(a[2], gs.t[cap:])
    for k in o:
        assert _equal_bits(o3[k], o[k].t[cap:]), k
    assert not torch.equal(_bits(a[0]), _bits(torch.tensor(th0[cap:], device=DEV))) or int(o3["accepted"].sum()) == 0
