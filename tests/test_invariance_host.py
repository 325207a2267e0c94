"""The harness of the invariance test (tests/invariance.py) on the CPU: its vectorised transitions against the per-chain
restatements, its targets against independent evaluations, and its calibration -- at C = 4096 chains, n = 8 iterations and
4 C reference draws every correct transition of the case table stays below ``threshold(K_TOTAL)`` with a mean acceptance in
[0.3, 0.97], and every mutant exceeds twice the threshold on the case it is attached to.  The factor 2 is a condition on
the power of the test, met by choosing the case's step and scale (never the threshold); no mutant had to be dropped.
Seeds are fixed: the file is deterministic."""
import functools

import numpy as np
import pytest

from tests import dist_restatement as dr
from tests import invariance as iv
from tests.gibbs_restatement import gibbs_draw
from tests.hmc_metric_restatement import DIAG, TRIL, hmc_metric_draw
from tests.mala_mvn_restatement import mala_mvn_draw
from tests.mh_mvn_restatement import mh_mvn_draw

C_HOST, N_HOST = 4096, 8
C8 = 8
THRESHOLD = iv.threshold(iv.K_TOTAL)
# every mutant switch of tests/invariance.py with the cases it is attached to ('untempered': a run at a temperature vector
# held against the law at t = 1)
MUTANTS = [
    ("mala/mix5_3/f64", "no_ratio"),
    ("mala_tril/mix5_3/f64/shared", "no_ratio"),
    ("mala_tril/mix5_3/f64/shared", "identity_ratio"),
    ("mala_tril/mix65_2/f32/indexed", "no_ratio"),
    ("mala_tril/mix65_2/f32/indexed", "identity_ratio"),
    ("hmc_metric/dense/mix5_3/f64/shared", "kinetic"),
    ("hmc_metric/dense/mix65_2/f32/indexed", "kinetic"),
    ("hmc_metric/diag/mix65_2/f64/per_chain", "kinetic"),
    ("ladder/mala/mix5_1/f64", "sign"),
    ("ladder/mala/mix5_1/f64", "no_rescale"),
    ("hmc/lin12/f32/temp", "untempered"),
    ("mala/lin3/f32/temp", "untempered"),
    ("mala_tril/mix5_1/f64/per_chain/temp", "untempered"),
]
NAMES = [c["name"] for c in iv.CASES]


# ------------------------------------------------------------------------------------------------ the table and the numbers
def test_k_total_is_the_sum_over_the_case_table():
    assert iv.K_TOTAL == sum(iv.n_statistics(c) for c in iv.CASES)
    assert iv.n_features(2) == 7 and iv.n_features(5) == 22 and iv.n_features(65) == 160
    for c in iv.CASES:
        P = iv.target_of(c["target"]).P
        assert iv.features(np.zeros((3, P)), np.zeros(3)).shape == (3, iv.n_features(P))
        assert iv.feature_name(P, iv.n_features(P) - 1) == "logp^2"


def test_the_threshold_is_the_bonferroni_quantile():
    assert abs(iv.threshold(1500) - 4.97) < 5e-3
    assert abs(iv.threshold(1) - 3.2905) < 1e-3          # the two-sided 1e-3 quantile of one normal
    assert 5.0 < THRESHOLD < 5.1


def test_the_case_table_holds_the_required_cases():
    """The minimum list, with one exchange: Gibbs runs on the linear-Gaussian plan of dims [3, 1] in f64, not on the
    mixture of P = 5, M = 3, because the library refuses Gibbs on a mixture plan by design (k_gibbs is not
    instantiated for it; tests/test_dist_gpu.py holds the refusal).  And one addition: the plan of dims [200, 1] in f64
    reports the layerwise family, so HMC runs on it as well."""
    want = {("hmc", "mix2_2", "f64"), ("hmc", "mix65_2", "f32"), ("hmc", "lin3", "f64"), ("hmc", "lin12", "f32"),
            ("mala", "mix5_3", "f64"), ("mala", "mix65_2", "f32"), ("mala", "lin3", "f32"), ("mh", "mix5_3", "f32"),
            ("mh", "lin12", "f64"), ("mh_tril", "mix5_3", "f64"), ("mh_tril", "mix65_2", "f32"),
            ("mala_tril", "mix5_3", "f64"), ("mala_tril", "mix65_2", "f32"), ("mala_tril", "mix5_1", "f64"),
            ("hmc_metric", "mix5_3", "f64"), ("hmc_metric", "mix65_2", "f32"), ("hmc_metric", "mix65_2", "f64"),
            ("hmc_metric", "lin12", "f32"), ("gibbs", "lin3", "f64"), ("gibbs", "lin12", "f32"), ("hmc", "lin200", "f64")}
    have = {(c["sampler"], c["target"], c["dtype"]) for c in iv.CASES if not c.get("ladder")}
    assert want <= have
    assert {(c["sampler"], c["target"], c["dtype"]) for c in iv.CASES if c.get("ladder")} == \
        {("mala", "mix5_1", "f64"), ("hmc", "mix64_1", "f32"), ("mh", "mix5_1", "f32")}
    assert len(set(NAMES)) == len(NAMES) and iv.C_GPU % (2 * len(iv.LADDER_T)) == 0
    q = iv.ladder_q()
    _, logq, cdf = iv.ladder_tables(iv.LADDER_T, q)
    off = ~np.eye(len(q), dtype=bool)
    assert (np.abs(logq.T - logq)[off] > 1e-3).all()   # no pair's proposal ratio vanishes
    np.testing.assert_allclose(cdf[:, -1], 1.0, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ the targets
@pytest.mark.parametrize("name", ["mix2_2", "mix5_3", "mix65_2", "mix5_1", "mix64_1", "lin3", "lin12", "lin200"])
def test_target_against_the_per_chain_restatement(name):
    tgt = iv.target_of(name)
    rng = np.random.default_rng(3)
    th = iv.exact_draws(tgt, C8, rng)
    temps = 0.2 + 0.8 * rng.random(C8)
    for tt in (None, temps):
        val, g = tgt.value_grad(th, tt)
        for c in range(C8):
            v, gg = dr.mix_value_grad(tgt.c, tgt.mean, tgt.prec, th[c], None if tt is None else tt[c])
            np.testing.assert_allclose(val[c], v, rtol=1e-12)
            np.testing.assert_allclose(g[c], gg, rtol=1e-12, atol=1e-12 * np.abs(gg).max())
        np.testing.assert_array_equal(tgt.value(th, tt), val)


@pytest.mark.parametrize("name", list(iv.LINEAR))
def test_linear_gaussian_target_is_the_log_posterior_with_its_constant(name):
    """log N(y | X theta, s^2) + log N(theta | 0, sigma^2) term by term, as the plan's likelihood and prior add it up."""
    D, N = iv.LINEAR[name]
    x, y, tgt = iv.linear_gaussian(D, N)
    s, sg = iv.LIK_SCALE, iv.PRIOR_SIGMA
    th = iv.exact_draws(tgt, C8, np.random.default_rng(1)) + 0.05
    for c in range(C8):
        out = x @ th[c, :D] + th[c, D]
        lik = np.sum(-0.5 * ((y[:, 0] - out) / s) ** 2 - np.log(s) - 0.5 * np.log(2 * np.pi))
        prior = np.sum(-0.5 * (th[c] / sg) ** 2 - np.log(sg) - 0.5 * np.log(2 * np.pi))
        np.testing.assert_allclose(tgt.value(th[c:c + 1])[0], lik + prior, rtol=1e-12)
    if name == "lin3":
        from tests.regression_restatement import linear_gaussian
        x0, y0, mean, cov = linear_gaussian()
        assert np.array_equal(x0, x) and np.array_equal(y0, y)
        np.testing.assert_allclose(tgt.means[0], mean, rtol=1e-13)
        np.testing.assert_allclose(tgt.covs[0], cov, rtol=1e-13, atol=1e-18)


def test_exact_draws_have_the_moments_of_their_law():
    rng = np.random.default_rng(0)
    tgt = iv.target_of("mix5_3")
    x = iv.exact_draws(tgt, 200000, rng)
    mean = tgt.probs @ tgt.means
    second = np.einsum("k,kij->ij", tgt.probs, tgt.covs + np.einsum("ki,kj->kij", tgt.means, tgt.means))
    se = x.std(0) / np.sqrt(len(x))
    assert (np.abs(x.mean(0) - mean) < 5 * se).all()
    np.testing.assert_allclose(x.T @ x / len(x), second, atol=0.1)
    g = iv.target_of("lin3")
    for t in (None, 0.5):
        y = iv.exact_draws((g.means[0], g.covs[0]), 200000, rng, t)
        np.testing.assert_allclose(np.cov(y.T), g.covs[0] / (t or 1.0), rtol=0.03, atol=1e-4)
    a = iv.exact_draws((tgt.probs, tgt.means, tgt.covs), 7, np.random.default_rng(4))
    assert np.array_equal(a, iv.exact_draws(tgt, 7, np.random.default_rng(4)))
    with pytest.raises(ValueError):
        iv.exact_draws(tgt, 4, rng, 0.5)


def test_z_scores_and_chunked_reference_moments():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((500, 3)) + 0.1, 2.0 * rng.standard_normal((900, 3))
    want = (a.mean(0) - b.mean(0)) / np.sqrt(a.var(0, ddof=1) / 500 + b.var(0, ddof=1) / 900)
    np.testing.assert_allclose(iv.z_scores(a, b), want, rtol=1e-13)
    np.testing.assert_allclose(iv.z_scores(iv.moments(a), b), want, rtol=1e-13)
    tgt = iv.target_of("mix65_2")
    n, m, v = iv.reference_moments(tgt, 3000, np.random.default_rng(5), chunk=1024)
    th = iv.exact_draws(tgt, 3000, np.random.default_rng(5))   # (one chunk draws other variates: compare the laws)
    f = iv.features(th, tgt.value(th))
    assert n == 3000 and (np.abs(iv.z_scores((n, m, v), f)) < 5).all()
    n1, m1, v1 = iv.reference_moments(tgt, 3000, np.random.default_rng(5), chunk=3000)
    np.testing.assert_allclose(m1, f.mean(0), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(v1, f.var(0, ddof=1), rtol=1e-9)


# ------------------------------------------------------------------------------------------------ the transcriptions
def _state(tgt, temps, seed):
    rng = np.random.default_rng(seed)
    th = iv.exact_draws(tgt, C8, rng) + 0.3 * rng.standard_normal((C8, tgt.P))
    t, g = tgt.value_grad(th, temps)
    return rng, th, t, g


def _fn(tgt, temps, c):
    return dr.mix_value_grad_fn(tgt.c, tgt.mean, tgt.prec, None if temps is None else float(temps[c]))


def _same(got, want, what):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=what)


TEMPS8 = 0.3 + 0.1 * np.arange(C8)
FORMS = ["shared", "per_chain", "indexed"]


def _table(form, P, rng, kind="dense"):
    G = dict(shared=1, per_chain=C8, indexed=2)[form]
    tab = 0.3 * (0.5 + rng.random((G, P))) if kind == "diag" else iv.factors(G, P, rng, 0.3)
    if kind == "dense":
        tab = tab + np.triu(rng.standard_normal(tab.shape), 1)   # the strict upper triangle is never read
    index = ((np.arange(C8) + 1) % 2).astype(np.int32) if form == "indexed" else None
    per_chain = [tab[0 if form == "shared" else c if form == "per_chain" else index[c]] for c in range(C8)]
    return (tab[0] if form == "shared" else tab), index, per_chain


@pytest.mark.parametrize("tempered", [False, True], ids=["plain", "tempered"])
@pytest.mark.parametrize("name", ["mix5_3", "lin12"])
def test_mh_mala_hmc_equal_their_restatements(name, tempered):
    tgt, temps = iv.target_of(name), TEMPS8 if tempered else None
    rng, th, t, g = _state(tgt, temps, 1)
    z, u = rng.standard_normal(th.shape), rng.random(C8)
    scale = 0.8 if name == "mix5_3" else 0.06
    steps = (1.0 if name == "mix5_3" else 0.012) * (0.2 + 3.0 * rng.random(C8))   # (eight chains accept and reject)
    a = iv.mh(tgt, th, t, z, u, scale, temps)
    b = iv.mala(tgt, th, t, g, z, u, steps, temps)
    hsteps = steps if name == "mix5_3" else 8 * steps
    c_ = iv.hmc(tgt, th, t, g, z, u, hsteps, 3, temps)
    for c in range(C8):
        vg = _fn(tgt, temps, c)
        w = dr.mh_draw(lambda x: vg(x)[0], th[c], t[c], z[c], u[c], scale)
        _same(a[0][c], w[0], "mh theta"), _same(a[1][c], w[1], "mh target")
        assert a[2][c] == w[2]
        w = dr.mala_draw(vg, th[c], t[c], g[c], z[c], u[c], steps[c])
        _same(b[0][c], w[0], "mala theta"), _same(b[1][c], w[1], "mala target"), _same(b[2][c], w[2], "mala grad")
        assert b[3][c] == w[3]
        w = dr.hmc_draw(vg, th[c], t[c], g[c], z[c], u[c], hsteps[c], 3)
        _same(c_[0][c], w[0], "hmc theta"), _same(c_[1][c], w[1], "hmc target"), _same(c_[2][c], w[2], "hmc grad")
        assert c_[3][c] == w[3]
    for out in (a, b, c_):
        assert 0 < out[-1].sum() < C8   # the eight chains mix accepts and rejects


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["mix5_3", "mix65_2"])
def test_factor_forms_equal_their_restatements(name, form):
    tgt = iv.target_of(name)
    temps = TEMPS8 if form == "per_chain" else None
    rng, th, t, g = _state(tgt, temps, 2)
    P = tgt.P
    z, u = rng.standard_normal(th.shape), rng.random(C8)
    size = 1.0 if P < 60 else 0.25
    L, index, Ls = _table(form, P, rng)
    L, Ls = size * L, [size * m for m in Ls]
    steps = (0.3 if P < 60 else 0.05) * (0.5 + rng.random(C8))
    a = iv.mh_tril(tgt, th, t, L, index, z, u, temps)
    b = iv.mala_tril(tgt, th, t, g, L, index, z, u, steps, temps)
    for c in range(C8):
        vg = _fn(tgt, temps, c)
        w = mh_mvn_draw(lambda x: vg(x)[0], th[c], t[c], Ls[c], z[c], u[c])
        _same(a[0][c], w[0], "mh_tril theta"), _same(a[1][c], w[1], "mh_tril target")
        assert a[2][c] == w[2]
        w = mala_mvn_draw(vg, th[c], t[c], g[c], Ls[c], z[c], u[c], steps[c])
        _same(b[0][c], w[0], "mala_tril theta"), _same(b[1][c], w[1], "mala_tril target"), _same(b[2][c], w[2], "grad")
        assert b[3][c] == w[3]
    assert 0 < a[2].sum() < C8 and 0 < b[3].sum() < C8


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["dense", "diag"])
@pytest.mark.parametrize("name", ["mix5_3", "mix65_2"])
def test_hmc_metric_equals_its_restatement(name, kind, form):
    tgt = iv.target_of(name)
    temps = TEMPS8 if form == "indexed" else None
    rng, th, t, g = _state(tgt, temps, 3)
    P = tgt.P
    v, u = rng.standard_normal(th.shape), rng.random(C8)
    tab, index, per_chain = _table(form, P, rng, kind)
    steps = (2.5 if P < 60 else 6.0 if kind == "dense" else 3.0) * (0.2 + 2.0 * rng.random(C8))
    a = iv.hmc_metric(tgt, th, t, g, kind, tab, index, v, u, steps, 3, temps)
    for c in range(C8):
        w = hmc_metric_draw(_fn(tgt, temps, c), th[c], t[c], g[c], DIAG if kind == "diag" else TRIL, per_chain[c], v[c], u[c],
                            steps[c], 3)
        _same(a[0][c], w[0], "theta"), _same(a[1][c], w[1], "target"), _same(a[2][c], w[2], "grad")
        assert a[3][c] == w[3]
    assert 0 < a[3].sum() < C8


@pytest.mark.parametrize("mode", ["intended", "reference"])
@pytest.mark.parametrize("name", ["gibbs/lin3/f64", "gibbs/lin12/f32"])
def test_gibbs_equals_its_restatement(name, mode):
    case = iv.CASE[name]
    tgt = iv.target_of(case["target"])
    temps = TEMPS8 if mode == "intended" else None
    rng, th, t, _ = _state(tgt, temps, 4)
    S = len(case["blocks"])
    z, u = rng.standard_normal(th.shape), rng.random((C8, S))
    a = iv.gibbs(tgt, th, t, case["blocks"], case["scales"], z, u, mode, temps)
    for c in range(C8):
        vg = _fn(tgt, temps, c)
        w = gibbs_draw(lambda x: vg(x)[0], th[c], t[c], case["blocks"], case["scales"], z[c], u[c], mode)
        _same(a[0][c], w[0], "theta"), _same(a[1][c], w[1], "target")
        assert np.array_equal(a[2][c], w[2].astype(bool))
    assert 0 < a[2].sum() < C8 * S


@pytest.mark.parametrize("grad", [True, False])
def test_between_equals_its_restatement(grad):
    from tests import pt_restatement as pr
    K, R = len(iv.LADDER_T), C8
    tgt = iv.target_of("mix5_1")
    rng = np.random.default_rng(6)
    temps = np.repeat(iv.LADDER_T, R)
    th = np.concatenate([iv.exact_draws(tgt, R, rng, t) for t in iv.LADDER_T])
    t, g = tgt.value_grad(th, temps)
    ld = pr.Ladder(iv.LADDER_T, iv.ladder_q(), np.float64)
    tl, logq, cdf = iv.ladder_tables(iv.LADDER_T, iv.ladder_q())
    assert np.array_equal(tl, ld.t) and np.array_equal(logq, ld.logq) and np.array_equal(cdf, ld.cdf)
    v, u = rng.random((K, R)), rng.random((K, R))
    partners = iv.draw_partners(cdf, v)
    assert np.array_equal(partners, np.stack([pr.draw_partners(ld.cdf[i], v[i], i) for i in range(K)]))
    a = iv.between(tl, logq, th, t, g if grad else None, partners, u)
    w = pr.between(ld, th, t, g if grad else None, partners=partners, u=u)
    _same(a[0], w["theta"], "theta"), _same(a[1], w["target"], "target")
    if grad:
        _same(a[2], w["grad"], "grad")
    assert np.array_equal(a[3], w["swap"].astype(bool)) and 0 < a[3].sum() < K * R
    # the exchanged targets are the tempered log-density of the rows they now belong to
    _same(a[1], tgt.value(a[0], temps), "target after the exchange")


# ------------------------------------------------------------------------------------------------ the calibration
@functools.lru_cache(maxsize=None)
def _host_run(name, mutant=None):
    """(largest |z|, its feature, mean acceptance, swap rate) of a case at the host sizes."""
    case = iv.CASE[name]
    rng = np.random.default_rng([NAMES.index(name), 77])
    out = iv.run_host(case, C_HOST, N_HOST, rng, mutant=None if mutant == "untempered" else mutant)
    z = iv.case_z(case, out["theta"], out["logp"], rng, n_ref=4 * C_HOST, untempered=mutant == "untempered")
    assert z.size == iv.n_statistics(case)
    w, where = iv.worst(z, iv.target_of(case["target"]).P)
    print(f"{name} {mutant or ''}: largest |z| {w:.2f} at {where}, acceptance {out['accept']:.3f}, exchanges "
          f"{out['swap']:.3f}, threshold {THRESHOLD:.2f}")
    return w, where, out["accept"], out["swap"]


@pytest.mark.parametrize("name", NAMES)
def test_correct_transition_stays_below_the_threshold(name):
    w, where, accept, swap = _host_run(name)
    assert w < THRESHOLD, (w, where)
    assert iv.ACCEPT_BAND[0] <= accept <= iv.ACCEPT_BAND[1], accept   # the chains move, and they also reject
    if iv.CASE[name].get("ladder"):
        assert 0.0 < swap < 1.0


@pytest.mark.parametrize("name,mutant", MUTANTS)
def test_mutant_exceeds_twice_the_threshold(name, mutant):
    w, where, _, _ = _host_run(name, mutant)
    assert w > 2 * THRESHOLD, (w, where)
    assert _host_run(name)[0] < THRESHOLD   # ... on a case whose correct transition passes
