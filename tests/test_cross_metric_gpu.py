"""HMC under a metric (k_hmc_metric, k_hmc_metric_warmup of eeyore_amd/csrc/ey_generic.hip), NUTS (k_nuts, ey_nuts.hip) and
elliptical slice sampling (k_eslice, k_eslice_ell, ey_eslice.hip) under every prior family, every likelihood and every
evaluation path of eval_target, on the cases of tests/cross_metric_cases.py against the f64 restatements on the CPU, and
against themselves.  tests/test_cross_metric_host.py holds the table to the conditions relied on here.  Plans are built
by tests/test_cross_gpu.py's _plan, _set_prior and _case_plan.

A draw is a chain of discontinuous decisions, so a comparison follows the restatement's margins (the rule is stated in
the host file): the outcomes -- accepted; depth, n_leapfrog and divergent for NUTS; n_evals for elliptical slice sampling
-- must be equal wherever the draw is not set aside, and the count of pairs set aside stays within the host file's caps.

f64: the whole three-draw trajectory, a chain followed up to its first set-aside draw (tests/test_nuts_gpu.py's _compare);
theta and target at TRACE (rtol 1e-8 / atol 1e-9), grad, accept_stat, energy, h_cur - h_prop and ell at 1e-10 relative to
the largest entry of the vector compared (tests/test_nuts_gpu.py).  f32: every draw restated from the state the device
itself holds before it (tests/test_cross_gpu.py's test_steps_of_every_sampler), so no chain is lost after a decision that
fell the other way; where the outcomes agree, elliptical slice sampling keeps F32_STATE (1e-5) on theta and the value
tolerance 2e-4 / 2e-4 on target and ell, hmc_metric and NUTS keep tests/test_hmc_metric_gpu.py's f32 bounds: state,
gradient and target at rtol = atol = 2e-2, h_cur - h_prop and NUTS's energy at rtol 2e-4 / atol 2e-3, and accept_stat, a
mean of rates min(1, exp(dH)), at the rate's bound 2e-4 max(1, |dH|) + 2e-3 at |dH| = 1 (beyond it the rate's error falls
with exp(-|dH|)): 2.2e-3.  h_cur - h_prop is compared where the restated |dH| is at most 20: no f32 uniform lies below
2^-24 = exp(-16.6), so a draw beyond it is decided whatever the error of dH is (and its decision is asserted all the same),
while a trajectory that far off has met targets of the order of 1e3 and more, where the bound on dH has no meaning.
Chains that did not move keep their bits.

A BCE case of dtype 'f32' is restated with what f32 makes of the naive BCE sum near a saturated sigmoid
(cross_metric_cases.Saturation): NaN where the f32 sigmoid is exactly 1, and a draw set aside where 1 - o is too small
for a decision to be held to it."""

import numpy as np
import pytest
import torch

from oracle import philox_oracle as po
from tests import cross_metric_cases as cm
from tests import cross_restatement as cr
from tests import eslice_restatement as er
from tests import nuts_restatement as nr
from tests.test_cross_gpu import DEV, DT, F32, F32_STATE, F64, RUN_SETTINGS, TRACE, _case_plan, _np, _t, _tol

pytestmark = pytest.mark.gpu

RTOL = 1e-10                                       # tests/test_nuts_gpu.py's, relative to the vector's largest entry
F32_TOL10 = dict(rtol=2e-2, atol=2e-2)             # tests/test_hmc_metric_gpu.py: state, gradient, target
F32_DH = dict(rtol=2e-4, atol=2e-3)                # ... h_cur - h_prop; here also NUTS's energy
F32_DH_RANGE = 20.0                                # ... compared where a uniform could still decide (the module docstring)
F32_ACCEPT_STAT = 2.2e-3                           # ... the rate's bound at |dH| = 1 (the module docstring)
SEED, IT0, OFF = 21, 5, 7
OUT_KEYS = {"hmc_metric": ("accepted", "rate", "h_cur", "h_prop"),
            "nuts": ("accepted", "depth", "n_leapfrog", "divergent", "accept_stat", "energy"),
            "eslice": ("accepted", "n_evals")}


class _Chains:
    """The device state of the chains ``sel`` of a case and its sampler's calls."""

    def __init__(self, pl, d, dtype, sel=slice(None)):
        self.pl, self.d, self.dtype, self.kind = pl, d, dtype, d["kind"]
        self.temp = None if d["temps"] is None else _t(d["temps"][sel], dtype)
        self.th = _t(d["th0"][sel], dtype)
        self.C = self.th.shape[0]
        if self.kind == "eslice":
            self.base = dict(base_loc=None, base_scale=None)
            if d["base"] is not None:
                self.base = dict(base_loc=_t(d["base"][0], dtype), base_scale=_t(d["base"][1], dtype))
            ell, tv = pl.eslice_ell(self.th, temp=self.temp, **self.base)
            self.tv, self.ell = tv.contiguous(), ell.contiguous()
            return
        tv, gr = pl.log_target_grad(self.th, temp=self.temp)
        self.tv, self.gr = tv.contiguous(), gr.contiguous()
        table, layout = d["table"], d["layout"]
        self.M = _t(table[0] if layout == "shared" else table[sel] if layout == "per_chain" else table, dtype)
        self.index = None if layout != "indexed" else torch.tensor(d["index"][sel], dtype=torch.int32, device=DEV)
        self.steps = _t(d["steps"][sel], dtype)

    def tensors(self):
        return (self.th, self.tv, self.ell) if self.kind == "eslice" else (self.th, self.tv, self.gr)

    def state(self):
        """The state as cm.advance takes it, in f64 numpy."""
        third = "ell" if self.kind == "eslice" else "grad"
        return {k: _np(t) for k, t in zip(("theta", "target", third), self.tensors())}

    def _common(self, kw):
        d = self.d
        if self.kind == "eslice":
            return dict(kw, max_shrinks=d["max_shrinks"], temp=self.temp, **self.base)
        return dict(kw, index=self.index, step_vec=self.steps, temp=self.temp)

    def _lead(self):
        d = self.d
        if self.kind == "eslice":
            return self.tensors()
        return self.tensors() + (0.0, d["max_depth"] if self.kind == "nuts" else d["num_steps"], self.M, d["form"])

    def step(self, z=None, u=None, **kw):
        """One draw; z [C, P] and u as the case holds them (numpy) or tensors, or neither: the in-kernel streams."""
        if z is not None:
            z, u = (a if torch.is_tensor(a) else _t(a, self.dtype) for a in (z, u))
            kw.update({"z" if self.kind == "eslice" else "v0": z, "u": u})
        fn = dict(hmc_metric=self.pl.hmc_metric_step, nuts=self.pl.nuts_step, eslice=self.pl.eslice_step)[self.kind]
        if self.kind == "hmc_metric":   # (its step is taken from step_vec; the scalar must still be positive)
            lead = self._lead()
            return fn(*lead[:3], 1.0, *lead[4:], **self._common(kw))
        return fn(*self._lead(), **self._common(kw))

    def run(self, K, rec, warmup=False, **kw):
        pl = self.pl
        if self.kind == "eslice":
            return pl.eslice_run(*self._lead(), K, **self._common(kw), **rec)
        fn = {("hmc_metric", False): pl.hmc_metric_run, ("hmc_metric", True): pl.hmc_metric_warmup,
              ("nuts", False): pl.nuts_run, ("nuts", True): pl.nuts_warmup}[self.kind, warmup]
        lead = self._lead()
        if self.kind == "hmc_metric":
            lead = lead[:3] + (1.0,) + lead[4:]
        return fn(*lead, K, **self._common(kw), **rec)


def _same(x, y):
    """Bit for bit (a NaN rate of a trajectory that left the finite numbers equals itself)."""
    if x.is_floating_point():
        bits = torch.int64 if x.dtype == F64 else torch.int32
        return torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))
    return torch.equal(x, y)


def _records(kind, K, C, P, dtype):
    rec = dict(samples=torch.empty(K, C, P, dtype=dtype, device=DEV), targets=torch.empty(K, C, dtype=dtype, device=DEV),
               accepted_rec=torch.empty(K, C, dtype=torch.uint8, device=DEV),
               accept_count=torch.zeros(C, dtype=torch.int32, device=DEV))
    if kind == "nuts":
        rec.update(depth_rec=torch.empty(K, C, dtype=torch.int32, device=DEV),
                   divergent_rec=torch.empty(K, C, dtype=torch.uint8, device=DEV))
    if kind == "eslice":
        rec.update(n_evals_rec=torch.empty(K, C, dtype=torch.int32, device=DEV))
    return rec


def _rel(got, want):
    """The largest error of got against want relative to want's largest entry (per row of a matrix)."""
    if want.size == 0:
        return 0.0
    scale = np.abs(want).max(axis=-1, keepdims=True) if want.ndim == 2 else np.abs(want).max()
    return float((np.abs(got - want) / np.maximum(scale, 1e-300)).max())


def _err(got, want):
    return float(np.abs(got - want).max()) if want.size else 0.0


def _device_values(kind, ch, out):
    """What the device reports beside the state, in f64 numpy, under the restatement's names."""
    if kind == "hmc_metric":
        return dict(dh=_np(out["h_cur"]) - _np(out["h_prop"]))
    if kind == "nuts":
        return dict(accept_stat=_np(out["accept_stat"]), energy=_np(out["energy"]))
    return {}


def _check_steps(case, variant=None):
    """The three draws of a case from its given randoms (module docstring).  Returns the largest errors seen."""
    dtype, f64 = DT[case[4]], case[4] == "f64"
    d = cm.build(case)
    kind = d["kind"]
    pl = _case_plan(d, dtype)
    if variant is not None:
        pl.set_variant(variant)
    ch = _Chains(pl, d, dtype)
    third = "ell" if kind == "eslice" else "grad"
    st0 = ch.state()
    want0 = cm.start(d)   # the start itself, at the value tolerances of tests/test_cross_gpu.py
    np.testing.assert_allclose(st0["target"], want0["target"], **_tol(dtype, True))
    np.testing.assert_allclose(st0[third], want0[third], **(_tol(dtype, True) if kind == "eslice" else _tol(dtype)))
    ref = cm.restate(d, st=st0) if f64 else None
    live = np.ones(d["C"], bool)
    aside, worst = 0, {}

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), v)

    for k in range(d["draws"]):
        before = ch.state()
        o = ref[k] if f64 else cm.advance(d, before, d["z"][k], d["u"][k])
        out = ch.step(d["z"][k], d["u"][k])
        after = ch.state()
        got = {key: out[key].cpu().numpy().astype(int) for key in cm.OUTCOME[kind]}
        vals = _device_values(kind, ch, out)
        clear = ~cm.set_aside(d, o)
        aside += int((~clear).sum())
        if f64:
            live &= clear
            for key in cm.OUTCOME[kind]:
                assert np.array_equal(got[key][live], o[key][live]), (k, key, got[key], o[key], o["margin"])
            for key in ("theta", "target"):
                note(key, _err(after[key][live], o[key][live]))
                np.testing.assert_allclose(after[key][live], o[key][live], **TRACE)
            rel = {third: (after[third][live], o[third][live])}
            for key, v in vals.items():
                fin = live & np.isfinite(o[key])
                rel[key] = (v[fin], o[key][fin])
            for key, (g, w) in rel.items():
                note(key, _rel(g, w))
                assert _rel(g, w) <= RTOL, (k, key, _rel(g, w))
            continue
        for key in cm.OUTCOME[kind]:
            assert np.array_equal(got[key][clear], o[key][clear]), (k, key, got[key], o[key], o["margin"])
        same = np.all([got[key] == o[key] for key in cm.OUTCOME[kind]], axis=0)
        if kind == "eslice":
            bounds = dict(theta=F32_STATE, target=_tol(F32, True), ell=_tol(F32, True))
        else:
            bounds = dict(theta=F32_TOL10, target=F32_TOL10, grad=F32_TOL10)
        for key, tol in bounds.items():
            note(key, _err(after[key][same], o[key][same]))
            np.testing.assert_allclose(after[key][same], o[key][same], **tol, err_msg=f"draw {k} {key}")
        if kind == "hmc_metric":
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(o["dh"]) & (np.abs(o["dh"]) <= F32_DH_RANGE)
            note("dh", _err(vals["dh"][fin], o["dh"][fin]))
            np.testing.assert_allclose(vals["dh"][fin], o["dh"][fin], **F32_DH)
        if kind == "nuts":
            note("energy", _err(vals["energy"][same], o["energy"][same]))
            note("accept_stat", _err(vals["accept_stat"][same], o["accept_stat"][same]))
            np.testing.assert_allclose(vals["energy"][same], o["energy"][same], **F32_DH)
            np.testing.assert_allclose(vals["accept_stat"][same], o["accept_stat"][same], rtol=0, atol=F32_ACCEPT_STAT)
        stay = got["accepted"] == 0   # chains that did not move keep their bits
        for key in before:
            assert np.array_equal(after[key][stay], before[key][stay]), (k, key)
    print(cm.case_id(case), "variant", variant, "set aside", aside, "of", d["C"] * d["draws"], "ERR",
          " ".join(f"{key}={v:.3e}" for key, v in sorted(worst.items())))
    assert aside <= cm.cap(d), aside
    return worst


# ------------------------------------------------------------------------------------------------ a. steps from given randoms
@pytest.mark.parametrize("case", cm.CASES, ids=cm.case_id)
def test_steps_from_given_randoms(case):
    _check_steps(case)


# ------------------------------------------------------------------------------------------------ b. the LDS tile loop
def _tile_loop_cases():
    """For every register-resident shape, the first case of every sampler and dtype."""
    seen, out = set(), []
    for c in cm.CASES:
        key = (c[0], c[3], c[4])
        if cr.SHAPES[c[3]]["tiny"] and key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _tile_loop_cases(), ids=cm.case_id)
def test_the_lds_tile_loop_under_the_same_numbers(case):
    """Variant bit 8 sends the plan of a register-resident shape through the LDS tile loop: the same restatement, the same
    tolerances."""
    sh = cr.SHAPES[case[3]]
    assert cr.tiny_kind(sh["dims"], sh["N"], sh["variant"]) != 0 and cr.tiny_kind(sh["dims"], sh["N"], 256) == 0
    _check_steps(case, variant=256)


# ------------------------------------------------------------------------------------------------ c. run equals steps
def _run_case(sampler, setting, C=3):
    family, loss, shape, dt = RUN_SETTINGS[setting]
    extra = dict(n=0, layout="indexed" if dt == "f32" else "per_chain", own_base=True,
                 max_shrinks=2 if dt == "f32" else er.MAX_SHRINKS)
    return cm.build((sampler, family, loss, shape, dt, True), C=C, draws=1, extra=extra)


@pytest.mark.parametrize("setting", list(RUN_SETTINGS))
@pytest.mark.parametrize("sampler", cm.SAMPLERS)
def test_run_equals_steps_bit_for_bit(sampler, setting):
    dtype = DT[RUN_SETTINGS[setting][3]]
    C, K = 3, 6
    d = _run_case(sampler, setting, C)
    kind = d["kind"]
    pl = _case_plan(d, dtype)
    a, b = _Chains(pl, d, dtype), _Chains(pl, d, dtype)
    rec = _records(kind, K, C, pl.P, dtype)
    oa = a.run(K, rec, seed=SEED, it=IT0, chain_offset=OFF)
    outs = []
    for k in range(K):
        ob = b.step(seed=SEED, it=IT0 + k, chain_offset=OFF)
        outs.append({key: v.clone() for key, v in ob.items()})
        assert _same(rec["samples"][k], b.th) and _same(rec["targets"][k], b.tv), k
        assert _same(rec["accepted_rec"][k], ob["accepted"]), k
        if kind == "nuts":
            assert _same(rec["depth_rec"][k], ob["depth"]) and _same(rec["divergent_rec"][k], ob["divergent"]), k
        if kind == "eslice":
            assert _same(rec["n_evals_rec"][k], ob["n_evals"]), k
    for x, y in zip(a.tensors(), b.tensors()):   # the carried state: theta, target, and grad or ell
        assert _same(x, y)
    for key in oa:
        assert _same(oa[key], ob[key]), key
    assert _same(rec["accept_count"], rec["accepted_rec"].int().sum(0))
    assert torch.isfinite(rec["samples"]).all() and torch.isfinite(rec["targets"]).all()
    assert int(rec["accepted_rec"].sum()) > 0
    if kind != "eslice":   # the warm-up form with nothing attached is the run
        w = _Chains(pl, d, dtype)
        rw = _records(kind, K, C, pl.P, dtype)
        ow = w.run(K, rw, warmup=True, seed=SEED, it=IT0, chain_offset=OFF)
        for x, y in list(zip(a.tensors(), w.tensors())) + [(rec[key], rw[key]) for key in rec] + [(oa[key], ow[key]) for key in oa]:
            assert _same(x, y)
    for c in (0, C - 1):   # chain c alone, at chain_offset + c, is the chain of the batch
        one = _Chains(pl, d, dtype, slice(c, c + 1))
        for x, y in zip(one.tensors(), _Chains(pl, d, dtype).tensors()):
            assert _same(x[0], y[c])
        for k in range(K):
            o1 = one.step(seed=SEED, it=IT0 + k, chain_offset=OFF + c)
            assert _same(one.th[0], rec["samples"][k, c]) and _same(one.tv[0], rec["targets"][k, c]), (c, k)
            for key in o1:
                assert _same(o1[key][0], outs[k][key][c]), (c, k, key)


# ------------------------------------------------------------------------------------------------ d. one wave by construction
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("sampler", cm.SAMPLERS)
def test_row_waves_change_no_bit(sampler, dt):
    """These kernels have no row-wave form: on the 150-row 'waves' shape the plan's row_waves option changes nothing."""
    case = next(c for c in cm.CASES if c[0] == sampler and c[3] == "waves" and c[4] == dt)
    d = cm.build(case)
    start, res = None, {}
    for mode in ("off", "on"):
        pl = _case_plan(d, DT[dt])
        pl.row_waves = mode
        ch = _Chains(pl, d, DT[dt])
        if start is None:   # (log_target_grad has a row-wave form of its own: both modes start from the same bits)
            start = [t.clone() for t in ch.tensors()]
        for t, s0 in zip(ch.tensors(), start):
            t.copy_(s0)
        outs = []
        for k in range(d["draws"]):
            out = ch.step(d["z"][k], d["u"][k])
            outs += [out[key].clone() for key in OUT_KEYS[d["kind"]]] + [t.clone() for t in ch.tensors()]
        res[mode] = outs
    assert len(res["on"]) == len(res["off"]) and all(_same(x, y) for x, y in zip(res["on"], res["off"]))
    assert any(bool(x.any()) for x in res["on"][::len(OUT_KEYS[d["kind"]]) + 3])   # (some chain moved)


# ------------------------------------------------------------------------------------------------ e. the streams
def _stream_case(sampler, dt):
    """The first case of a sampler and dtype on a shape of the LDS tile loop with more than one row tile."""
    return next(c for c in cm.CASES if c[0] == sampler and c[3] == "lds3" and c[4] == dt)


def _words(d):
    return nr.words(d["max_depth"]) if d["kind"] == "nuts" else er.words()


@pytest.mark.parametrize("sampler", cm.SAMPLERS)
def test_the_in_kernel_streams_in_f64_are_the_oracle_s(sampler):
    """v0 / z = u = NULL in f64 against the same call given the Philox oracle's normals and uniforms (block words for NUTS
    and elliptical slice sampling, as tests/test_nuts_gpu.py and tests/test_eslice_gpu.py lay them out): with part a., parity
    of the draw on the streams with the restatement.  Equal outcomes; values at the f64 tolerances of part a."""
    d = cm.build(_stream_case(sampler, "f64"))
    kind, C, P = d["kind"], d["C"], d["P"]
    pl = _case_plan(d, F64)
    a, b = _Chains(pl, d, F64), _Chains(pl, d, F64)
    for k in range(2):
        z = po.normal(C, P, SEED, IT0 + k, chain_offset=OFF, dtype=np.float64)
        if kind == "hmc_metric":
            u = po.uniform(C, SEED, IT0 + k, chain_offset=OFF, dtype=np.float64)
        else:
            u = po.uniform_blocks(np.arange(C) + OFF, _words(d), SEED, IT0 + k, dtype=np.float64)
        oa = a.step(seed=SEED, it=IT0 + k, chain_offset=OFF)
        ob = b.step(z, u)
        for key in cm.OUTCOME[kind]:
            assert _same(oa[key], ob[key]), (k, key)
        sa, sb = a.state(), b.state()
        for key in ("theta", "target"):
            np.testing.assert_allclose(sa[key], sb[key], **TRACE)
        third = "ell" if kind == "eslice" else "grad"
        assert _rel(sa[third], sb[third]) <= RTOL
        va, vb = _device_values(kind, a, oa), _device_values(kind, b, ob)
        for key in va:
            fin = np.isfinite(vb[key])
            assert _rel(va[key][fin], vb[key][fin]) <= RTOL, (k, key)
    assert not _same(a.th, _t(d["th0"], F64))


@pytest.mark.parametrize("sampler", cm.SAMPLERS)
def test_the_in_kernel_streams_in_f32_are_the_library_s_bit_for_bit(sampler):
    """v0 / z = u = NULL in f32 against the same call fed Plan.philox_normal and Plan.philox_uniform (philox_uniform_blocks
    for the samplers that read block words)."""
    d = cm.build(_stream_case(sampler, "f32"))
    kind, C = d["kind"], d["C"]
    pl = _case_plan(d, F32)
    a, b = _Chains(pl, d, F32), _Chains(pl, d, F32)
    for k in range(2):
        z = pl.philox_normal(C, SEED, IT0 + k, OFF)
        u = pl.philox_uniform(C, SEED, IT0 + k, OFF) if kind == "hmc_metric" else \
            pl.philox_uniform_blocks(C, _words(d), SEED, IT0 + k, OFF)
        oa = a.step(seed=SEED, it=IT0 + k, chain_offset=OFF)
        ob = b.step(z, u)
        for key in OUT_KEYS[kind]:
            assert _same(oa[key], ob[key]), (k, key)
        for x, y in zip(a.tensors(), b.tensors()):
            assert _same(x, y), k
    assert not _same(a.th, _t(d["th0"], F32))


# ------------------------------------------------------------------------------------------------ the defect these cases found
@pytest.mark.parametrize("entry", ["step", "run", "warmup"])
@pytest.mark.parametrize("sampler", cm.GRADIENT_SAMPLERS)
def test_the_gradient_a_draw_leaves_is_the_gradient_at_the_state(sampler, entry):
    """The narrowest case of what part a. found: k_hmc_metric<float, TinyDyn, EY_METRIC_DIAG> stored, for a chain that
    accepted, a gradient read from the wrong LDS address (the register holding the image's offset was copied under an empty
    EXEC mask; eeyore_amd/csrc/ey_generic.hip, EY_METRIC_EACH), while theta, the target and H were right.  On the TinyDyn
    shape in f32, after every entry point of the four gradient samplers, the carried gradient is the gradient
    Plan.log_target_grad gives at the carried state, at the f32 value tolerance, for the chains that moved and the others."""
    case = next(c for c in cm.CASES if c[0] == sampler and c[3] == "dyn" and c[4] == "f32")
    d = cm.build(case)
    pl = _case_plan(d, F32)
    ch = _Chains(pl, d, F32)
    if entry == "step":
        moved = int(ch.step(d["z"][0], d["u"][0])["accepted"].sum())
    else:
        if sampler.startswith("hmc_metric"):
            ch.steps = _t(d["steps"][0] * np.ones(d["C"]), F32)   # (every chain at the smallest step: most draws accept)
        rec = _records(d["kind"], 2, d["C"], pl.P, F32)
        ch.run(2, rec, warmup=entry == "warmup", seed=SEED, it=IT0)
        moved = int(rec["accepted_rec"].sum())
    tv, gr = pl.log_target_grad(ch.th, temp=ch.temp)
    assert moved >= 3
    np.testing.assert_allclose(_np(ch.gr), _np(gr), **_tol(F32))
    np.testing.assert_allclose(_np(ch.tv), _np(tv), **_tol(F32, True))
