"""Every prior family with every likelihood, evaluation path and sampler of the generic kernels (eval_target and tiny_rows
of eeyore_amd/csrc/ey_generic.hip, the eight sampler kernels around them) and the layerwise path under the regression
likelihoods (ey_large.hip), against the reference's recorded values and traces (g21_cross_traces.npz) and against the f64
restatements on the CPU (tests/cross_restatement.py).

Tolerances are the project's own.  f64: values and gradients rtol 1e-10 / atol 1e-11 (atol 1e-10 for the sums), states and
targets after a step rtol 1e-8 / atol 1e-9 (tests/test_prior_gpu.py, tests/test_regression_gpu.py).  f32, against the
restatement on the inputs the device holds: values 2e-4 / 2e-4, states 1e-5, log rate rtol 2e-4 / atol 2e-3, decisions
compared where the margin exceeds F32_DECISION_TOL max(1, |log rate|) (tests/test_ram_gpu.py, tests/test_gpu_parity.py).
The layerwise path: tests/test_regression_gpu.py's _bgemm_close and tests/test_gpu_parity.py's
test_bgemm_path_mala_mh_leapfrog_rows_vs_oracle.

An f32 step is restated from the state the device itself is in before the step (as tests/test_ram_gpu.py does): the
rounding of earlier steps is not what a step's comparison is about, and a decision inside the margin that falls the other
way does not end the comparison of the steps after it."""
import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import cross_restatement as cr
from tests import prior_restatement as pr
from tests.ram_restatement import adapt_h, alpha_of, refactorised

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
DT = {"f64": F64, "f32": F32}
TRACE = dict(rtol=1e-8, atol=1e-9)
F32_STATE = dict(rtol=1e-5, atol=1e-5)
F32_RATE = dict(rtol=2e-4, atol=2e-3)
F32_DECISION_TOL = 2e-3  # as tests/test_gpu_parity.py
FAMILY = {"normal": L.EY_PRIOR_NORMAL, "laplace": L.EY_PRIOR_LAPLACE, "studentt": L.EY_PRIOR_STUDENT_T,
          "cauchy": L.EY_PRIOR_STUDENT_T}


# ------------------------------------------------------------------------------------------------ the step cases
def _step_cases():
    """(sampler, family, loss, shape, dtype, tempered): every sampler on every shape it runs on in both dtypes, three cases
    per cell, the family, the likelihood and the tempering cycled with periods that share no factor.
    test_the_step_cases_cover_the_product holds the result to the covering properties."""
    out = []
    for si, s in enumerate(cr.SAMPLERS):
        n = 0
        for shape, sh in cr.SHAPES.items():
            if shape == "waves" and s not in cr.WAVE_SAMPLERS:
                continue
            for dt in ("f64", "f32"):
                for _ in range(2 if shape == "bce" else 3):
                    fam = cr.FAMILIES[(n + si) % 4]
                    loss = sh["losses"][(n + n // 4 + si) % len(sh["losses"])]
                    out.append((s, fam, loss, shape, dt, bool((n + n // 4 + n // 20) % 2)))
                    n += 1
    return out


STEP_CASES = _step_cases()


def case_id(case):
    s, fam, loss, shape, dt, temp = case
    return f"{s}-{fam}-{loss}-{shape}-{dt}-{'temp' if temp else 'plain'}"


# the seed of a case's inputs where 0 does not meet the conditions tests/test_cross_host.py states (both decisions at least
# five times, at most 1 margin below 1e-9 in f64 and at most 3 below the f32 tolerance)
SEEDS = {
}


def build_case(case, **kw):
    s, fam, loss, shape, dt, temp = case
    return cr.cross_case(s, fam, loss, shape, temp=temp, seed=SEEDS.get(case_id(case), 0),
                         round_to=np.float32 if dt == "f32" else None, **kw)


def test_the_step_cases_cover_the_product():
    cases = STEP_CASES
    assert len(cases) == len(set(cases)) and 200 <= len(cases) <= 400
    for s in cr.SAMPLERS:
        mine = [c for c in cases if c[0] == s]
        assert {c[1] for c in mine} == set(cr.FAMILIES) and {c[2] for c in mine} == set(cr.LOSSES), s
        shapes = set(cr.SHAPES) - (set() if s in cr.WAVE_SAMPLERS else {"waves"})
        assert {(c[3], c[4]) for c in mine} == {(sh, dt) for sh in shapes for dt in DT}, s
        assert {c[5] for c in mine} == {False, True}, s
    pairs = {(f, lo) for f in cr.FAMILIES for lo in cr.LOSSES}
    assert {(c[1], c[2]) for c in cases if c[0] in cr.GRADIENT_SAMPLERS} == pairs
    assert {(c[1], c[2]) for c in cases if c[0] not in cr.GRADIENT_SAMPLERS} == pairs
    for shape, sh in cr.SHAPES.items():
        assert {c[2] for c in cases if c[3] == shape} == set(sh["losses"]), shape
        for dt in DT:
            assert {c[1] for c in cases if c[3] == shape and c[4] == dt} == set(cr.FAMILIES) or shape == "bce", (shape, dt)
    tempered = sum(c[5] for c in cases)
    assert abs(2 * tempered - len(cases)) <= len(cases) // 10  # half of them, to a tenth
    assert set(SEEDS) <= {case_id(c) for c in cases}


# ------------------------------------------------------------------------------------------------ helpers
def _tol(dtype, sums=False):
    return dict(rtol=1e-10, atol=1e-10 if sums else 1e-11) if dtype == F64 else dict(rtol=2e-4, atol=2e-4)


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().double().cpu().numpy().copy()


def _plan(shape, loss, x, y, dtype, variant=None):
    """A plan of one of cr.SHAPES under a likelihood, set up to reach the shape's evaluation path."""
    from eeyore_amd.plan import Plan
    sh = cr.SHAPES[shape]
    pl = Plan(sh["dims"], [1] * (len(sh["dims"]) - 1), sh["acts"], cr.LIK_CODE[loss], dtype, DEV)
    if x is not None:
        pl.set_data(_t(x, dtype), _t(y, dtype))
    if loss in ("gauss", "laplace"):
        pl.set_lik_scale(cr.LIK_SCALE[loss])
    pl.row_waves = sh["waves"]
    pl.set_variant(sh["variant"] if variant is None else variant)
    assert pl.P == cr.num_params(sh["dims"])
    return pl


def _set_prior(pl, family, loc, scale, df, fused=False):
    """Uploads the family's tables; returns them as the device holds them (f32: rounded), in f64 numpy.  ``fused``: a cell
    of cr.FUSED, whose Normal-prior plan the fused 16x16x4 kernels serve unless a call passes EY_FORCE_GENERIC."""
    lo, sc = _t(loc, pl.dtype), _t(scale, pl.dtype)
    if family == "normal":
        pl.set_prior(lo, sc)
        d = None
    else:
        d = None if family == "laplace" else torch.ones_like(sc) if family == "cauchy" else _t(df, pl.dtype)
        pl.set_prior_family(FAMILY[family], lo, sc, d)
    assert pl.prior_family == FAMILY[family]
    assert pl.kernel == ("fused16" if fused and family == "normal" else "generic")
    return _np(lo), _np(sc), None if family != "studentt" else _np(d)


def _want(tgt, th):
    want = [tgt.parts(t) for t in th]
    return tuple(np.array([w[i] for w in want]) for i in range(4))


G21 = cr.load_g21()


def _g21_plan(rec, dtype):
    from eeyore_amd.plan import Plan
    pl = Plan(rec["dims"], [1, 1], rec["acts"], cr.LIK_CODE[rec["loss"]], dtype, DEV)
    pl.set_data(_t(rec["x"], dtype), _t(rec["y"], dtype))
    if rec["loss"] != "poisson":
        pl.set_lik_scale(rec["lik_scale"])
    _set_prior(pl, rec["family"], rec["loc"], rec["scale"], rec["df"])
    return pl


# ------------------------------------------------------------------------------------------------ 1. values and gradients
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("key", sorted(k for k in G21 if k.startswith("values/")))
def test_values_against_the_reference(key, dtype):
    rec = G21[key]
    pl = _g21_plan(rec, dtype)
    th = _t(rec["theta"], dtype)
    lik, prior = pl.log_target(th)
    tv, gr = pl.log_target_grad(th)
    parts = rec["parts"]
    print(key, "errors: lik", np.abs(_np(lik) - parts[:, 0]).max(), "prior", np.abs(_np(prior) - parts[:, 1]).max(),
          "target", np.abs(_np(tv) - parts[:, 2]).max(), "grad", np.abs(_np(gr) - rec["grad"]).max())
    np.testing.assert_allclose(_np(lik), parts[:, 0], **_tol(dtype, True))
    np.testing.assert_allclose(_np(prior), parts[:, 1], **_tol(dtype, True))
    np.testing.assert_allclose(_np(tv), parts[:, 2], **_tol(dtype, True))
    np.testing.assert_allclose(_np(gr), rec["grad"], **_tol(dtype))


def _value_cases():
    for shape, sh in cr.SHAPES.items():
        for loss in sh["losses"]:
            for family in cr.FAMILIES:
                if not (family == "normal" and (shape, loss) in cr.FUSED):  # that plan is the fused kernels', not eval_target's
                    yield shape, loss, family


@pytest.mark.parametrize("C", [1, 11])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,loss,family", list(_value_cases()))
def test_values_against_torch(shape, loss, family, dtype, C):
    sh = cr.SHAPES[shape]
    dims, acts, N = sh["dims"], sh["acts"], sh["N"]
    assert cr.tiny_kind(dims, N, sh["variant"]) == sh["tiny"]  # the path the shape is in the table for
    x, y = cr.rows_for(dims, loss, N, seed=len(shape))
    pl = _plan(shape, loss, x, y, dtype)
    P = pl.P
    loc, scale, df = _set_prior(pl, family, *pr.distinct_tables(P, P))
    rng = np.random.default_rng(10 * P + C)
    th = _t(0.5 * rng.standard_normal((C, P)), dtype)
    temps = _t(0.2 + 0.8 * rng.random(C), dtype)
    tgt = cr.make_target(dims, acts, loss, _np(_t(x, dtype)), _np(_t(y, dtype)), pr.make_prior(family, loc, scale, df))
    w_lik, w_pri, w_tv, w_gr = _want(tgt, _np(th))
    tt = _np(temps)

    def check(label):
        lik, prior = pl.log_target(th)
        tv, gr = pl.log_target_grad(th)
        print(shape, loss, family, label, "errors: lik", np.abs(_np(lik) - w_lik).max(), "prior",
              np.abs(_np(prior) - w_pri).max(), "target", np.abs(_np(tv) - w_tv).max(), "grad", np.abs(_np(gr) - w_gr).max())
        np.testing.assert_allclose(_np(lik), w_lik, **_tol(dtype, True))
        np.testing.assert_allclose(_np(prior), w_pri, **_tol(dtype, True))
        np.testing.assert_allclose(_np(tv), w_tv, **_tol(dtype, True))
        np.testing.assert_allclose(_np(gr), w_gr, **_tol(dtype))
        # a per-chain temperature multiplies everything
        tl, tp = pl.log_target(th, temp=temps)
        ttv, tgr = pl.log_target_grad(th, temp=temps)
        np.testing.assert_allclose(_np(tl), tt * w_lik, **_tol(dtype, True))
        np.testing.assert_allclose(_np(tp), tt * w_pri, **_tol(dtype, True))
        np.testing.assert_allclose(_np(ttv), tt * w_tv, **_tol(dtype, True))
        np.testing.assert_allclose(_np(tgr), tt[:, None] * w_gr, **_tol(dtype))
        if loss in cr.REGRESSION:
            rows = pl.log_lik_rows(th)
            want_rows = np.array([tgt.rows(t) for t in _np(th)])
            np.testing.assert_allclose(_np(rows), want_rows, **_tol(dtype))
            np.testing.assert_allclose(_np(pl.log_lik_rows(th, temp=temps)), tt[:, None] * want_rows, **_tol(dtype))
        return lik, prior, tp, tv, gr

    lik, prior, tp, tv, gr = check("as set up")
    if sh["tiny"]:  # a register path: variant bit 8 sends the same plan through the LDS tile loop, held to the same numbers
        pl.set_variant(256)
        lik_l, _, _, tv_l, gr_l = check("LDS tile loop")
        np.testing.assert_allclose(_np(lik_l), _np(lik), **_tol(dtype, True))
        np.testing.assert_allclose(_np(tv_l), _np(tv), **_tol(dtype, True))
        np.testing.assert_allclose(_np(gr_l), _np(gr), **_tol(dtype))
    # the prior alone, on a plan that has no data
    bare = _plan(shape, loss, None, None, dtype)
    _set_prior(bare, family, loc, scale, df)
    assert torch.equal(bare.log_target(th, prior_only=True)[1], prior)
    assert torch.equal(bare.log_target(th, temp=temps, prior_only=True)[1], tp)


# ------------------------------------------------------------------------------------------------ 2. steps of every sampler
class _Chains:
    """The device state of C chains of one sampler on a plan, stepped from given z and u."""

    def __init__(self, pl, d, dtype, temps=None):
        self.pl, self.d, self.dtype, self.sampler, self.par = pl, d, dtype, d["sampler"], d["par"]
        C, P = d["th0"].shape
        self.temp = None if temps is None else _t(temps, dtype)
        self.th = _t(d["th0"], dtype)
        tv, gr = pl.log_target_grad(self.th, temp=self.temp)
        self.tv, self.gr = tv.contiguous(), gr.contiguous()
        par = self.par
        if self.sampler == "ram":
            self.chol = _t(np.stack([par["chol0"] * np.eye(P)] * C), dtype)
        elif self.sampler == "am":
            self.mean = torch.zeros(C, P, dtype=dtype, device=DEV)
            self.cs = torch.zeros(C, P, P, dtype=dtype, device=DEV)
            self.c0 = _t(par["cov0"] * np.eye(P), dtype)
            self.cov = self.c0[None].repeat(C, 1, 1).contiguous()
            self.nacc, self.bd = (torch.zeros(C, dtype=torch.int32, device=DEV) for _ in range(2))
        elif self.sampler == "gibbs":
            self.tb = pl.gibbs_table(d["blocks"], [par["scale"]] * len(d["blocks"]))
        elif self.sampler in ("mh_tril", "mala_tril"):
            self.tril = _t(d["L"], dtype)

    def state(self):
        """The state as cr.advance takes it, in f64 numpy."""
        st = dict(theta=_np(self.th), target=_np(self.tv), grad=_np(self.gr))
        if self.sampler == "ram":
            st["chol"] = _np(self.chol)
        if self.sampler == "am":
            mean, cs, cov, nacc = _np(self.mean), _np(self.cs), _np(self.cov), self.nacc.cpu().numpy()
            st["am"] = [dict(mean=mean[c], cov_sum=cs[c], cov=cov[c], num_accepted=int(nacc[c])) for c in range(len(mean))]
        return st

    def step(self, idx, z=None, u=None, u_mix=None, **kw):
        pl, par, s, dt = self.pl, self.par, self.sampler, self.dtype
        if z is not None:
            kw.update(z=_t(z, dt), u=_t(u, dt))
        kw["temp"] = self.temp
        if s in cr.WAVE_SAMPLERS:
            kw["flags"] = L.EY_FORCE_GENERIC  # the generic kernel also where a fused family would serve the plan
        if s == "hmc":
            if "z" in kw:
                kw["p0"] = kw.pop("z")
            out = pl.hmc_step(self.th, self.tv, self.gr, par["step"], par["L"], **kw)
            out["log_rate"] = out["h_cur"] - out["h_prop"]
            return out
        if s == "mala":
            return pl.mala_step(self.th, self.tv, self.gr, par["step"], **kw)
        if s == "mh":
            return pl.mh_step(self.th, self.tv, par["scale"], **kw)
        if s == "ram":
            return pl.ram_step(self.th, self.tv, self.chol, idx + 1, a=par["a"], g=par["g"], **kw)
        if s == "am":
            if u_mix is not None:
                kw["u_mix"] = _t(u_mix, dt)
            return pl.am_step(self.th, self.tv, self.mean, self.cs, self.cov, self.nacc, self.c0, idx, l=par["l"], b=par["b"],
                              c=par["c"], eps=par["eps"], t0=par["t0"], offset=0, breakdowns=self.bd, **kw)
        if s == "gibbs":
            return pl.gibbs_step(self.th, self.tv, self.tb, mode="intended", **kw)
        if s == "mh_tril":
            return pl.mh_tril_step(self.th, self.tv, self.tril, **kw)
        return pl.mala_tril_step(self.th, self.tv, self.gr, par["step"], self.tril, **kw)


def _case_plan(d, dtype):
    pl = _plan(d["shape"], d["loss"], d["x"], d["y"], dtype)
    _set_prior(pl, d["family"], d["loc"], d["scale"], d["df"], fused=(d["shape"], d["loss"]) in cr.FUSED)
    return pl


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_steps_of_every_sampler(case):
    """One to five steps from given z and u.  f64: the whole trajectory of the restatement; at most 1 decision of the case
    inside 1e-9.  f32: every step restated from the device's own state before it; at most 3 decisions inside the f32
    margin; RAM's factor from the device's own log rate, as tests/test_ram_gpu.py takes it."""
    sampler, dtype = case[0], DT[case[4]]
    d = build_case(case)
    pl = _case_plan(d, dtype)
    ch = _Chains(pl, d, dtype, d["temps"])
    steps, C, P = d["z"].shape
    left_out = 0
    for it in range(steps):
        if dtype == F32:
            st = ch.state()
            chol0 = None if sampler != "ram" else st["chol"].copy()
            acc_w, margin, rate, branch = cr.advance(sampler, d["targets"], d["par"], st, it, d["z"][it], d["u"][it],
                                                     d["u_mix"][it], blocks=d["blocks"], L=d.get("L"))
            th_before, tv_before = _np(ch.th), _np(ch.tv)
        else:
            acc_w, margin, rate, branch = d["accepted"][it], d["margin"][it], d["log_rate"][it], d["branch"][it]
        out = ch.step(it, d["z"][it], d["u"][it], d["u_mix"][it])
        acc = out["accepted"].cpu().numpy()
        if sampler == "am":
            assert np.array_equal(out["branch"].cpu().numpy(), branch), it
        if dtype == F64:
            clear = margin > 1e-9
            left_out += int((~clear).sum())
            assert np.array_equal(acc[clear], acc_w[clear]), (it, acc, acc_w)
            np.testing.assert_allclose(_np(ch.th), d["theta"][it], **TRACE)
            np.testing.assert_allclose(_np(ch.tv), d["target"][it], **TRACE)
            continue
        lr_dev = _np(out["log_rate"])
        with np.errstate(invalid="ignore"):
            finite = np.isfinite(rate)
            tol = np.where(finite, F32_DECISION_TOL * np.maximum(1.0, np.abs(rate)), 0.0)
        np.testing.assert_allclose(lr_dev[finite], rate[finite], **F32_RATE)
        clear = margin > tol
        left_out += int((~clear).sum())
        assert np.array_equal(acc[clear], acc_w[clear]), (it, acc, acc_w)
        # the state: where the device decided as the restatement did it is the restatement's, elsewhere it is the start
        same = (acc == acc_w) if sampler != "gibbs" else (acc == acc_w).all(1)
        np.testing.assert_allclose(_np(ch.th)[same], st["theta"][same], **F32_STATE)
        np.testing.assert_allclose(_np(ch.tv)[same], st["target"][same], **_tol(F32, True))
        if sampler != "gibbs":
            rej = acc == 0
            assert np.array_equal(_np(ch.th)[rej], th_before[rej]) and np.array_equal(_np(ch.tv)[rej], tv_before[rej])
        if sampler == "ram":
            S1 = _np(ch.chol)
            for c in range(C):
                beta = adapt_h(P, it + 1, d["par"]["g"]) * (alpha_of(np.float32(lr_dev[c])) - d["par"]["a"])
                want = refactorised(chol0[c], d["z"][it][c], beta)
                assert np.linalg.norm(np.tril(S1[c]) - want) / np.linalg.norm(want) <= 1e-5, (it, c)
    assert left_out <= (1 if dtype == F64 else 3)
    if sampler == "am":
        assert int(ch.bd.sum()) == 0


# ------------------------------------------------------------------------------------------------ 3. the reference's traces
@pytest.mark.parametrize("key", sorted(k for k in G21 if k.startswith("trace/")))
def test_fixture_replay(key):
    rec = G21[key]
    pl = _g21_plan(rec, F64)
    th = _t(rec["theta0"], F64)[None].clone()
    tv = _t([rec["init_target"]], F64)
    gr = _t(rec["init_grad"], F64)[None].clone()
    kind = rec["sampler"]
    t0, g0 = pl.log_target_grad(th)  # the start is the reference's own
    np.testing.assert_allclose(_np(t0), _np(tv), **_tol(F64, True))
    if kind != "mh":
        np.testing.assert_allclose(_np(g0), _np(gr), **_tol(F64))
    for it in range(rec["z"].shape[0]):
        z, u = _t(rec["z"][it], F64)[None], _t([rec["u"][it]], F64)
        if kind == "hmc":
            out = pl.hmc_step(th, tv, gr, float(rec["par"]), int(rec["L"]), p0=z, u=u)
        elif kind == "mala":
            out = pl.mala_step(th, tv, gr, float(rec["par"]), z=z, u=u)
        else:
            out = pl.mh_step(th, tv, float(rec["par"]), z=z, u=u)
        assert int(out["accepted"].item()) == int(rec["accepted"][it]), it
        np.testing.assert_allclose(_np(th)[0], rec["sample"][it], **TRACE)
        np.testing.assert_allclose(tv.item(), rec["target_val"][it], **TRACE)
    assert 0 < rec["accepted"].sum() < len(rec["accepted"])


# ------------------------------------------------------------------------------------------------ 4. run equals steps
RUN_SETTINGS = {"cauchy-poisson-fix-f32": ("cauchy", "poisson", "fix", "f32"),
                "laplace-laplace-lds3-f64": ("laplace", "laplace", "lds3", "f64")}


def _run(ch, K, rec, **kw):
    """K iterations of the chains' sampler in one launch."""
    pl, par, s = ch.pl, ch.par, ch.sampler
    kw = dict(kw, temp=ch.temp, samples=rec[0], targets=rec[1], accepted_rec=rec[2])
    if s in cr.WAVE_SAMPLERS:
        kw["flags"] = L.EY_FORCE_GENERIC
    if s == "hmc":
        return pl.hmc_run(ch.th, ch.tv, ch.gr, par["step"], par["L"], K, **kw)
    if s == "mala":
        return pl.mala_run(ch.th, ch.tv, ch.gr, par["step"], K, **kw)
    if s == "mh":
        return pl.mh_run(ch.th, ch.tv, par["scale"], K, **kw)
    if s == "ram":
        return pl.ram_run(ch.th, ch.tv, ch.chol, 1, K, a=par["a"], g=par["g"], **kw)
    if s == "am":
        return pl.am_run(ch.th, ch.tv, ch.mean, ch.cs, ch.cov, ch.nacc, ch.c0, 0, K, l=par["l"], b=par["b"], c=par["c"],
                         eps=par["eps"], t0=par["t0"], offset=0, breakdowns=ch.bd, **kw)
    if s == "gibbs":
        return pl.gibbs_run(ch.th, ch.tv, ch.tb, K, mode="intended", **kw)
    if s == "mh_tril":
        return pl.mh_tril_run(ch.th, ch.tv, ch.tril, K, **kw)
    return pl.mala_tril_run(ch.th, ch.tv, ch.gr, par["step"], ch.tril, K, **kw)


def _extra(ch):
    """What a sampler carries besides theta and the target: the gradient, RAM's factor, AM's moments."""
    s = ch.sampler
    if s in cr.GRADIENT_SAMPLERS:
        return [ch.gr]
    return [ch.chol] if s == "ram" else [ch.mean, ch.cs, ch.cov, ch.nacc, ch.bd] if s == "am" else []


@pytest.mark.parametrize("setting", list(RUN_SETTINGS))
@pytest.mark.parametrize("sampler", cr.SAMPLERS)
def test_run_equals_steps_bit_for_bit(sampler, setting):
    family, loss, shape, dt = RUN_SETTINGS[setting]
    dtype = DT[dt]
    C, K, seed, it0, off = 3, 6, 21, 5, 7
    d = cr.cross_case(sampler, family, loss, shape, temp=True, C=C, steps=1, round_to=np.float32 if dt == "f32" else None)
    pl = _case_plan(d, dtype)
    a, b = _Chains(pl, d, dtype, d["temps"]), _Chains(pl, d, dtype, d["temps"])
    S = len(d["blocks"])
    rec = (torch.empty(K, C, pl.P, dtype=dtype, device=DEV), torch.empty(K, C, dtype=dtype, device=DEV),
           torch.empty((K, C, S) if sampler == "gibbs" else (K, C), dtype=torch.uint8, device=DEV))
    _run(a, K, rec, seed=seed, it=it0, chain_offset=off)
    accepted = []
    for k in range(K):
        out = b.step(k, seed=seed, it=it0 + k, chain_offset=off)
        accepted.append(out["accepted"].clone())
        assert torch.equal(rec[0][k], b.th) and torch.equal(rec[1][k], b.tv) and torch.equal(rec[2][k], out["accepted"]), k
    assert torch.equal(a.th, b.th) and torch.equal(a.tv, b.tv)
    assert all(torch.equal(x, y) for x, y in zip(_extra(a), _extra(b)))
    assert torch.isfinite(a.th).all() and torch.isfinite(a.tv).all()
    if sampler in cr.WAVE_SAMPLERS:  # chain c alone, at chain_offset + c, is the chain of the batch
        for c in (0, C - 1):
            dc = dict(d, th0=d["th0"][c:c + 1])
            one = _Chains(pl, dc, dtype, d["temps"][c:c + 1])
            assert torch.equal(one.tv, _Chains(pl, d, dtype, d["temps"]).tv[c:c + 1])
            for k in range(K):
                out = one.step(k, seed=seed, it=it0 + k, chain_offset=off + c)
                assert torch.equal(one.th[0], rec[0][k, c]) and torch.equal(one.tv[0], rec[1][k, c]), (c, k)
                assert torch.equal(out["accepted"][0], accepted[k][c]), (c, k)


# ------------------------------------------------------------------------------------------------ 5. row waves in the steps
@pytest.mark.parametrize("sampler", cr.WAVE_SAMPLERS)
def test_row_waves_in_the_step_kernels(sampler):
    """Student-t x Gaussian on the 150-row MLP(2-3-1), f64: several waves per chain against one.  The decisions are the
    same, the states agree to rtol 1e-12 (the order of the row sums differs), and both are the restatement's."""
    d = cr.cross_case(sampler, "studentt", "gauss", "waves")
    res = {}
    for mode in ("on", "off"):
        pl = _case_plan(d, F64)
        pl.row_waves = mode
        ch = _Chains(pl, d, F64)
        accs = []
        for it in range(d["z"].shape[0]):
            out = ch.step(it, d["z"][it], d["u"][it])
            accs.append(out["accepted"].cpu().numpy())
            clear = d["margin"][it] > 1e-9
            assert np.array_equal(accs[-1][clear], d["accepted"][it][clear]), (mode, it)
            np.testing.assert_allclose(_np(ch.th), d["theta"][it], **TRACE)
            np.testing.assert_allclose(_np(ch.tv), d["target"][it], **TRACE)
        res[mode] = (np.array(accs), _np(ch.th), _np(ch.tv))
    assert (d["margin"] > 1e-9).all() and 0 < d["accepted"].sum() < d["accepted"].size
    assert np.array_equal(res["on"][0], res["off"][0])
    np.testing.assert_allclose(res["on"][1], res["off"][1], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(res["on"][2], res["off"][2], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ 6. the layerwise path
BG_DIMS, BG_ACTS, BG_N, BG_C = [10, 64, 2], [2, 0], 70, 9
BG_PAR = dict(mala=0.002, mh=0.02, hmc=(0.01, 5))


def bgemm_case(loss):
    """MLP(10-64-2) tanh / none on 70 rows under a regression likelihood and a Normal prior, everything rounded to f32: the
    rows, tables, start, z, p0 and u of one MALA, MH and HMC draw of 9 chains, and the restated target."""
    from tests import regression_restatement as rr
    r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)  # noqa: E731
    x, y = (r32(a) for a in rr.synthetic(BG_DIMS, loss, BG_N, seed=5))
    P = cr.num_params(BG_DIMS)
    rng = np.random.default_rng(600 + cr.LIK_CODE[loss])
    mu, sigma = r32(0.1 * rng.standard_normal(P)), r32(0.5 + rng.random(P))
    tgt = rr.Target(BG_DIMS, BG_ACTS, loss, x, y, scale=cr.LIK_SCALE[loss], prior=pr.make_prior("normal", mu, sigma))
    return dict(x=x, y=y, mu=mu, sigma=sigma, target=tgt, P=P, th0=r32(0.3 * rng.standard_normal((BG_C, P))),
                z=r32(rng.standard_normal((BG_C, P))), p0=r32(rng.standard_normal((BG_C, P))), u=r32(rng.random(BG_C)))


def bgemm_draws(d, sampler, tv, gr):
    """The restated draw of every chain from the start and the device's own f32 target and gradient there:
    (theta, target, grad, accepted, log rate), per chain."""
    tgt, out = d["target"], []
    for c in range(BG_C):
        if sampler == "mala":
            out.append(pr.mala_draw(tgt.value_and_grad, d["th0"][c], tv[c], gr[c], d["z"][c], d["u"][c], BG_PAR["mala"]))
        elif sampler == "mh":
            th, t, a, lr = pr.mh_draw(tgt.log_target, d["th0"][c], tv[c], d["z"][c], d["u"][c], BG_PAR["mh"])
            out.append((th, t, None, a, lr))
        else:
            out.append(pr.hmc_draw(tgt.value_and_grad, d["th0"][c], tv[c], gr[c], d["p0"][c], d["u"][c], *BG_PAR["hmc"]))
    return out


def bgemm_undecided(draws, u, hmc=False):
    lr = np.array([w[4] for w in draws])
    tol = F32_DECISION_TOL * np.maximum(1.0, np.abs(lr))
    return np.abs(np.log(u) - (np.minimum(lr, 0.0) if hmc else lr)) <= tol, lr, tol


@pytest.mark.parametrize("products", ["bf16x3", "exact"])
@pytest.mark.parametrize("loss", ["gauss", "poisson"])
def test_bgemm_path_steps_under_regression(loss, products):
    from eeyore_amd.plan import Plan
    d = bgemm_case(loss)
    pl = Plan(BG_DIMS, [1, 1], BG_ACTS, cr.LIK_CODE[loss], F32, DEV)
    pl.set_data(_t(d["x"], F32), _t(d["y"], F32))
    pl.set_prior(_t(d["mu"], F32), _t(d["sigma"], F32))
    if loss == "gauss":
        pl.set_lik_scale(cr.LIK_SCALE[loss])
    pl.f32_products = products
    assert pl.kernel == "bgemm"
    th0 = _t(d["th0"], F32)
    t, g = pl.log_target_grad(th0)
    t0, g0 = _np(t), _np(g)
    for c in range(BG_C):  # the start against the restatement, at _bgemm_close's f32 tolerances
        w_tv, w_gr = d["target"].value_and_grad(d["th0"][c])
        np.testing.assert_allclose(t0[c], w_tv, rtol=2e-4, atol=2e-3)
        np.testing.assert_allclose(g0[c], w_gr, rtol=2e-3, atol=2e-4 * max(1.0, np.abs(w_gr).max()))
    z, p0, u = _t(d["z"], F32), _t(d["p0"], F32), _t(d["u"], F32)
    for sampler in ("mala", "mh", "hmc"):
        th, tv, gg = th0.clone(), t.clone(), g.clone()
        if sampler == "mala":
            out = pl.mala_step(th, tv, gg, BG_PAR["mala"], z=z, u=u)
            lr_dev = _np(out["log_rate"])
        elif sampler == "mh":
            out = pl.mh_step(th, tv, BG_PAR["mh"], z=z, u=u)
            lr_dev = _np(out["log_rate"])
        else:
            out = pl.hmc_step(th, tv, gg, *BG_PAR["hmc"], p0=p0, u=u)
            lr_dev = _np(out["h_cur"]) - _np(out["h_prop"])
        want = bgemm_draws(d, sampler, t0, g0)
        undecided, lr, tol = bgemm_undecided(want, d["u"], hmc=sampler == "hmc")
        print(loss, products, sampler, "largest log-rate error / tolerance", (np.abs(lr_dev - lr) / tol).max())
        assert (np.abs(lr_dev - lr) <= tol).all()
        assert undecided.sum() <= 1
        acc, acc_w = out["accepted"].cpu().numpy(), np.array([int(w[3]) for w in want])
        np.testing.assert_array_equal(acc[~undecided], acc_w[~undecided])
        same = acc == acc_w
        np.testing.assert_allclose(_np(th)[same], np.array([w[0] for w in want])[same], rtol=2e-3, atol=2e-4)
        if sampler != "mh":
            go = np.array([w[2] for w in want])
            np.testing.assert_allclose(_np(gg)[same], go[same], rtol=5e-3, atol=5e-3 * max(1.0, np.abs(go).max()))
        assert torch.equal(th[~out["accepted"].bool()], th0[~out["accepted"].bool()])
    # in-kernel Philox == streams passed in
    a, b = [th0.clone(), t.clone(), g.clone()], [th0.clone(), t.clone(), g.clone()]
    oa = pl.mala_step(*a, BG_PAR["mala"], seed=6, it=3, chain_offset=4)
    ob = pl.mala_step(*b, BG_PAR["mala"], z=pl.philox_normal(BG_C, 6, 3, 4), u=pl.philox_uniform(BG_C, 6, 3, 4))
    assert torch.equal(oa["accepted"], ob["accepted"]) and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    # HMC.leapfrog: L steps, L + 1 evaluations, momentum negated
    th, p = th0.clone(), p0.clone()
    step, nsteps = BG_PAR["hmc"]
    tl, gl = pl.leapfrog(th, p, step, nsteps)
    for c in (0, BG_C - 1):
        tho, po = d["th0"][c].copy(), d["p0"][c].copy()
        to, go = d["target"].value_and_grad(tho)
        po = po + 0.5 * step * go
        for k in range(nsteps):
            tho = tho + step * po
            to, go = d["target"].value_and_grad(tho)
            po = po + (step if k < nsteps - 1 else 0.5 * step) * go
        np.testing.assert_allclose(_np(th)[c], tho, rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(_np(p)[c], -po, rtol=5e-3, atol=5e-3)  # (HMC.leapfrog returns the momentum negated)
        np.testing.assert_allclose(tl[c].item(), to, rtol=2e-4, atol=2e-2)
        np.testing.assert_allclose(_np(gl)[c], go, rtol=5e-3, atol=5e-3 * max(1.0, np.abs(go).max()))


def test_bgemm_model_refuses_another_family_before_any_launch():
    from eeyore_amd.plan import Plan, _stream
    d = bgemm_case("gauss")
    dims = [10, 200, 2]  # beyond the generic kernels' LDS in f64: only the layerwise path holds it
    x = d["x"]
    pl = Plan(dims, [1, 1], [2, 1], cr.LIK_CODE["gauss"], F64, DEV)
    pl.set_data(_t(x, F64), _t(d["y"], F64))
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
    assert pl.kernel == "bgemm"
    pl.set_prior_family(L.EY_PRIOR_STUDENT_T, torch.zeros(pl.P), torch.ones(pl.P), torch.full((pl.P,), 3.0))
    assert pl.kernel == "generic"
    C = 2
    th = torch.zeros(C, pl.P, dtype=F64, device=DEV)
    tv = torch.full((C,), -7.0, dtype=F64, device=DEV)
    gr = torch.full((C, pl.P), 0.5, dtype=F64, device=DEV)
    rc = L.lib().ey_log_target_grad(pl.handle, L.ptr(th), None, C, L.ptr(tv), L.ptr(gr), _stream(pl.device))
    msg = L.lib().ey_last_error().decode()
    assert rc == -2 and "Student-t" in msg and "generic kernels" in msg, msg
    for call in (lambda: pl.log_target_grad(th), lambda: pl.log_target(th), lambda: pl.hmc_step(th, tv, gr, 0.01, 2),
                 lambda: pl.mala_step(th, tv, gr, 0.01), lambda: pl.mh_step(th, tv, 0.1)):
        with pytest.raises(RuntimeError, match="prior is served only for models the generic kernels can hold"):
            call()
    torch.cuda.synchronize()
    assert bool((tv == -7.0).all()) and bool((gr == 0.5).all()) and bool((th == 0).all())
    pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))  # a Normal prior again: the layerwise kernels serve it
    assert pl.kernel == "bgemm" and torch.isfinite(pl.log_target_grad(th)[0]).all()


# ------------------------------------------------------------------------------------------------ 7. the model surface
def test_hmc_run_of_a_model_under_a_student_t_prior_and_a_poisson_loss():
    from torch.distributions import StudentT
    from torch.utils.data import DataLoader

    from eeyore_amd.chains import ChainBuffer
    from eeyore_amd.constants import poisson_loss
    from eeyore_amd.datasets import XYDataset
    from eeyore_amd.models import mlp
    from eeyore_amd.samplers import HMC
    dims = [4, 3, 3]
    x, y = cr.rows_for(dims, "poisson", 40, seed=7)
    data = XYDataset(_t(x, F32), _t(y, F32))
    loader = DataLoader(data, batch_size=len(data), shuffle=False)
    m = mlp.MLP(loss=poisson_loss(), hparams=mlp.Hyperparameters(dims=dims, bias=2 * [True], activations=[torch.sigmoid, None]),
                dtype=F32, device=DEV)
    P = m.num_params()
    loc, scale, df = (_t(a, F32) for a in pr.distinct_tables(P, 5))
    m.prior = StudentT(df, loc, scale)
    C, K = 32, 30
    th0 = 0.1 * torch.randn(C, P, generator=torch.Generator().manual_seed(0)).to(DEV)
    s = HMC(m, theta0=th0, dataloader=loader, step=0.05, num_steps=5, seed=1,
            chain=ChainBuffer(keys=['sample', 'target_val', 'accepted']))
    s.run(num_epochs=K, num_burnin_epochs=0)
    plan = m._plan(data.x, data.y)
    assert plan.kernel == "generic" and plan.prior_family == L.EY_PRIOR_STUDENT_T and plan.lik_scale == 1.0
    chain = s.get_chain()
    smp, tvs = chain.get_samples(), chain.get_target_vals()
    assert smp.shape == (K, C, P) and torch.isfinite(smp).all()
    want = torch.stack([m.log_target(smp[i].contiguous(), data.x, data.y) for i in range(K)])
    np.testing.assert_allclose(_np(tvs), _np(want), **_tol(F32, True))
    rate = chain.get_accepted().float().mean().item()
    print("HMC under a Student-t prior and a Poisson loss: acceptance", rate)
    assert 0.0 < rate < 1.0
