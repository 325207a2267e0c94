"""The host side of tests/test_cross_gpu.py: the restatement (tests/cross_restatement.py) against the reference's recorded
values and traces (g21_cross_traces.npz), and the conditions on the inputs that the GPU tests rely on, for every case the
GPU module parametrizes.  Needs no GPU."""
import os

import numpy as np
import pytest

from tests import cross_restatement as cr
from tests import prior_restatement as pr
from tests import regression_restatement as rr
from tests import test_cross_gpu as gpu  # the very same case lists, seeds and builders

G21 = cr.load_g21()
F32_DECISION_TOL = 2e-3


def test_the_fixture_holds_what_it_should():
    assert sorted(G21) == sorted([f"values/{f}/{lo}" for f in pr.FAMILIES for lo in rr.LOSSES]
                                 + ["trace/hmc", "trace/mala", "trace/mh"])
    assert [(G21[f"trace/{k}"]["family"], G21[f"trace/{k}"]["loss"]) for k in ("hmc", "mala", "mh")] == \
        [("laplace", "poisson"), ("studentt", "gauss"), ("cauchy", "laplace")]
    for key, rec in G21.items():
        assert rec["dims"] == [2, 3, 1] and rec["acts"] == [2, 0] and rec["x"].shape == (40, 2)
        if key.startswith("values/"):
            assert rec["theta"].shape == (4, 13) and rec["parts"].shape == (4, 3) and rec["grad"].shape == (4, 13)
        else:
            assert rec["z"].shape == (60, 13) and 0 < rec["accepted"].sum() < 60
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_cross_traces.npz")
    assert os.path.getsize(path) < 100 * 1024


@pytest.mark.parametrize("key", sorted(k for k in G21 if k.startswith("values/")))
def test_restatement_reproduces_the_recorded_values(key):
    rec = G21[key]
    tgt = cr.g21_target(rec)
    for i, th in enumerate(rec["theta"]):
        ll, lp, lt, g = tgt.parts(th)
        np.testing.assert_allclose(ll, rec["parts"][i, 0], rtol=1e-12)
        np.testing.assert_allclose(lp, rec["parts"][i, 1], rtol=1e-12)
        np.testing.assert_allclose(lt, rec["parts"][i, 2], rtol=1e-12)
        np.testing.assert_allclose(g, rec["grad"][i], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(tgt.rows(th).sum(), rec["parts"][i, 0], rtol=1e-12)  # the row terms add up to it


@pytest.mark.parametrize("key", sorted(k for k in G21 if k.startswith("trace/")))
def test_restatement_replays_the_recorded_traces(key):
    rec = G21[key]
    out = pr.replay(rec, cr.g21_target(rec))
    assert np.array_equal(out["accepted"], rec["accepted"]) and out["margin"].min() > 1e-9
    np.testing.assert_allclose(out["sample"], rec["sample"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["target_val"], rec["target_val"], rtol=1e-12, atol=1e-12)


def test_the_shapes_reach_the_paths_they_are_named_for():
    for name, sh in cr.SHAPES.items():
        assert cr.tiny_kind(sh["dims"], sh["N"], sh["variant"]) == sh["tiny"], name
        assert cr.tiny_kind(sh["dims"], sh["N"], 256) == 0, name
    assert cr.tiny_kind([3, 4, 2], 40) == 0 and cr.tiny_kind([3, 4, 2], 127) == 0 and cr.tiny_kind([3, 4, 2], 128) == 1
    assert cr.num_params(cr.SHAPES["fix"]["dims"]) == 27 and cr.num_params(cr.SHAPES["dyn"]["dims"]) == 26
    assert cr.num_params(cr.SHAPES["lds3"]["dims"]) == 67  # the prior's lane pass has a second, 3-lane round
    assert cr.node_blocks(rr.S_DIMS) == rr.S_BLOCKS and cr.node_blocks(pr.OTHER_DIMS) == pr.OTHER_BLOCKS


def test_the_step_cases_cover_the_product():
    gpu.test_the_step_cases_cover_the_product()


@pytest.mark.parametrize("case", gpu.STEP_CASES, ids=gpu.case_id)
def test_the_step_cases_meet_the_conditions_the_gpu_test_relies_on(case):
    """Conditions on the inputs, not measurements: both decisions at least five times (Gibbs: its sub-steps); in f64 at
    most 1 decision within 1e-9 of the threshold, in f32-rounded form at most 3 within 2e-3 max(1, |log rate|)."""
    d = gpu.build_case(case)
    f32 = case[4] == "f32"
    accepts, rejects, undecided = cr.decision_stats(d, f32=f32)
    assert accepts >= 5 and rejects >= 5, (accepts, rejects)
    assert undecided <= (3 if f32 else 1), undecided
    assert np.isfinite(d["theta"]).all() and np.isfinite(d["target"]).all()
    if case[0] == "am":
        assert (d["branch"] != 2).all()


@pytest.mark.parametrize("sampler", cr.WAVE_SAMPLERS)
def test_the_row_wave_cases_stay_clear_of_the_margin(sampler):
    d = cr.cross_case(sampler, "studentt", "gauss", "waves")
    assert (d["margin"] > 1e-9).all() and cr.decision_stats(d)[0] >= 5 and cr.decision_stats(d)[1] >= 5


@pytest.mark.parametrize("loss", ["gauss", "poisson"])
def test_the_layerwise_cases_leave_at_most_one_decision_open(loss):
    d = gpu.bgemm_case(loss)
    start = [d["target"].value_and_grad(t) for t in d["th0"]]
    tv, gr = np.array([s[0] for s in start]), np.array([s[1] for s in start])
    total = 0
    for sampler in ("mala", "mh", "hmc"):
        undecided, lr, _ = gpu.bgemm_undecided(gpu.bgemm_draws(d, sampler, tv, gr), d["u"], hmc=sampler == "hmc")
        assert undecided.sum() <= 1 and np.isfinite(lr).all(), sampler
        acc = np.array([w[3] for w in gpu.bgemm_draws(d, sampler, tv, gr)])
        total += int(acc.sum())
    assert 0 < total < 3 * gpu.BG_C


def test_sampler_case_and_other_case_are_what_they_were():
    """The two older builders are calls of cr.run_case now.  Their arrays were compared with array_equal against the ones
    their own loops gave before the move (every sampler, every loss / family, two argument sets); what stays checkable
    here is that they return what their users read, and that the same call gives the same bits."""
    d, d2 = (rr.sampler_case("mala", loss="poisson", C=3, steps=2) for _ in range(2))
    assert d["theta"].shape == (2, 3, 13) and d["accepted"].shape == (2, 3) and d["margin"].shape == (2, 3)
    assert all(np.array_equal(d[k], d2[k]) for k in ("theta", "target", "accepted", "margin", "log_rate"))
    e = pr.other_case("mala_tril", "cauchy", C=3, steps=2)
    assert e["theta"].shape == (2, 3, 27) and e["df"] is None and np.isfinite(e["target"]).all()
    g = pr.other_case("gibbs", "laplace", C=2, steps=1)
    assert g["accepted"].shape == (1, 2, len(pr.OTHER_BLOCKS)) and g["margin"].shape == g["accepted"].shape
