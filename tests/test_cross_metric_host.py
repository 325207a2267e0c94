"""The host side of tests/test_cross_metric_gpu.py: the table of tests/cross_metric_cases.py held to the conditions the
device test relies on, from the restatements alone (f64 arithmetic; the cases of dtype 'f32' on their f32-rounded inputs).
Needs no GPU.

The conditions are not measurements.  A case that misses one gets another seed in cross_metric_cases.SEEDS; no cap is
raised.  The set-aside rule: in f64 a (chain, draw) pair is set aside when the restatement's margin is at most 1e-9; in
f32 when it is at most F32_DECISION_TOL (2e-3) times max(1, |log rate|) for hmc_metric, times 1 for NUTS (its margins are
relative already), and for elliptical slice sampling when the smallest |ell' - log y| is at most 2e-3 max(1, |log y|) or
the smallest angle whose sign was branched on is at most 2e-3.  (The angle is a number in [-1, 1] whose f32 error does
not grow with the target; were it scaled by |log y| too, which is 30 to 5000 on these targets, every draw that shrinks
its bracket once would be set aside and the device test would compare almost nothing.  The rule used sets aside a subset
of those draws.)  In a BCE case of dtype 'f32' a draw is also set aside where it evaluated the target at a point whose
sigmoid output is within 3e-5 of 1 without being 1 in f32 (cross_metric_cases.Saturation): these count against the cap
like any other."""
import functools

import numpy as np
import pytest

from tests import cross_metric_cases as cm
from tests import cross_restatement as cr
from tests import nuts_restatement as nr


@functools.lru_cache(maxsize=None)
def _restated(case):
    d = cm.build(case)
    return d, cm.restate(d)


def _of(sampler):
    return [c for c in cm.CASES if c[0].startswith(sampler)]


def test_the_table_covers_the_product():
    cases = cm.CASES
    assert len(cases) == len(set(cases)) == 200 and set(cm.EXTRA) == set(cases)
    for s in cm.SAMPLERS:
        mine = [c for c in cases if c[0] == s]
        assert {c[1] for c in mine} == set(cr.FAMILIES) and {c[2] for c in mine} == set(cr.LOSSES), s
        assert {(c[3], c[4]) for c in mine} == {(sh, dt) for sh in cr.SHAPES for dt in ("f64", "f32")}, s
        assert {c[5] for c in mine} == {False, True}, s
        if s != "eslice":
            assert {cm.EXTRA[c]["layout"] for c in mine} == set(cm.LAYOUTS), s
            for dt in ("f64", "f32"):
                assert {cm.EXTRA[c]["layout"] for c in mine if c[4] == dt} == set(cm.LAYOUTS), (s, dt)
    for shape, sh in cr.SHAPES.items():
        assert {c[2] for c in cases if c[3] == shape} == set(sh["losses"]), shape
        assert cr.tiny_kind(sh["dims"], sh["N"], sh["variant"]) == sh["tiny"], shape
        assert cr.tiny_kind(sh["dims"], sh["N"], 256) == 0, shape   # variant bit 8: the LDS tile loop
    tempered = sum(c[5] for c in cases)
    assert abs(2 * tempered - len(cases)) <= len(cases) // 10
    assert set(cm.SEEDS) <= {cm.case_id(c) for c in cases}
    # elliptical slice sampling: under a Normal prior both the plan's prior and tables of its own, under the other families
    # always a base; one case per shape with max_shrinks = 2, in both dtypes over the shapes
    es = [c for c in cases if c[0] == "eslice"]
    assert {cm.EXTRA[c]["own_base"] for c in es if c[1] == "normal"} == {False, True}
    assert all(cm.EXTRA[c]["own_base"] for c in es if c[1] != "normal")
    two = [c for c in es if cm.EXTRA[c]["max_shrinks"] == 2]
    assert sorted(c[3] for c in two) == sorted(cr.SHAPES) and {c[4] for c in two} == {"f64", "f32"}
    assert all(cm.EXTRA[c]["max_shrinks"] == 64 for c in es if c not in two)


def test_the_inputs_are_what_the_device_will_hold():
    """A case of dtype 'f32' has every number the device holds rounded to f32; the steps span what the module says."""
    r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)  # noqa: E731
    for case in (_of("nuts/dense")[4], _of("hmc_metric/diag")[3], _of("eslice")[3]):
        assert case[4] == "f32"
        d = cm.build(case)
        keys = ["x", "y", "loc", "scale", "th0", "z", "u"] + (["table", "steps"] if d["kind"] != "eslice" else [])
        for k in keys:
            assert np.array_equal(d[k], r32(d[k])), k
        if d["temps"] is not None:
            assert np.array_equal(d["temps"], r32(d["temps"]))
        if d["kind"] == "eslice" and d["base"] is not None:
            assert np.array_equal(d["base"][1], r32(d["base"][1]))
    assert cm.NUTS_FACTORS[0] == 0.25 and cm.NUTS_FACTORS[-1] == 30.0 and (np.diff(cm.NUTS_FACTORS) > 0).all()
    assert cm.HMC_FACTORS[0] == 0.5 and cm.HMC_FACTORS[-1] == 3.0 and len(cm.HMC_FACTORS) == len(cm.NUTS_FACTORS) == cm.C
    d = cm.build(_of("nuts/dense")[2])
    assert d["layout"] == "indexed" and d["table"].shape == (cm.G, d["P"], d["P"]) and d["index"].dtype == np.int32
    assert set(d["index"]) == set(range(cm.G)) and np.array_equal(d["table"], np.tril(d["table"]))
    small = cm.build(_of("nuts/diag")[0], C=3, draws=1)
    base = cr.par_of("hmc", small["shape"], small["loss"])["step"]
    assert np.allclose(small["steps"], base * cm.NUTS_FACTORS[[0, 5, 10]]) and small["th0"].shape == (3, small["P"])


@pytest.mark.parametrize("case", cm.CASES, ids=cm.case_id)
def test_the_case_meets_the_conditions_the_gpu_test_relies_on(case):
    d, outs = _restated(case)
    pairs = d["C"] * d["draws"]
    aside = sum(int(cm.set_aside(d, o).sum()) for o in outs)
    assert cm.cap(d) == (1 if d["dtype"] == "f64" else 6) and pairs == 33
    assert aside <= cm.cap(d), aside
    if d["kind"] == "nuts":
        stop, depth = np.stack([o["stop"] for o in outs]), np.stack([o["depth"] for o in outs])
        assert (stop == "max_depth").any() and (depth == d["max_depth"]).any()
        assert (np.isin(stop, ("tree", "subblock")) & (depth < d["max_depth"])).any()
        assert (stop == "divergent").any() and np.stack([o["divergent"] for o in outs]).any()
        assert all(np.isfinite(o["theta"]).all() and np.isfinite(o["target"]).all() for o in outs)
    elif d["kind"] == "hmc_metric":
        acc = sum(int(o["accepted"].sum()) for o in outs)
        assert acc >= 3 and pairs - acc >= 3, acc
    else:
        ne = np.stack([o["n_evals"] for o in outs])
        assert (ne >= 3).any() and (ne == 1).any()
        exhausted = sum(int(o["exhausted"].sum()) for o in outs)
        if d["max_shrinks"] == 2:
            assert 2 <= exhausted <= 9 and ne.max() == 3, exhausted
        else:
            assert exhausted == 0
        ells = np.concatenate([cm.start(d)["ell"]] + [o["ell"] for o in outs])
        assert np.isfinite(ells).all()
        if d["dtype"] == "f32":   # the states' values are numbers f32 holds (an exp beyond 88 is inf there)
            assert np.abs(ells).max() <= 1e30


@pytest.mark.parametrize("shape", list(cr.SHAPES))
def test_nuts_on_every_shape_holds_every_way_a_tree_ends(shape):
    """Over the NUTS cases of a shape: a draw that does not move, a divergent draw of depth 0, and both places the
    criterion can stop a tree (between the ends of the whole tree, inside the new subtree)."""
    stay = div0 = 0
    stops = set()
    for case in _of("nuts"):
        if case[3] == shape:
            _, outs = _restated(case)
            stay += sum(int((o["accepted"] == 0).sum()) for o in outs)
            div0 += sum(int(((o["divergent"] == 1) & (o["depth"] == 0)).sum()) for o in outs)
            stops |= set(np.concatenate([o["stop"] for o in outs]))
    assert stay >= 1 and div0 >= 1 and stops == {"max_depth", "tree", "subblock", "divergent"}, (stay, div0, stops)


@pytest.mark.parametrize("shape", list(cr.SHAPES))
def test_the_two_forms_of_the_restated_tree_agree_on_these_targets(shape):
    """nr.nuts_draw (the recursion) and nr.nuts_draw_iterative (the kernel's checkpoint loop) agree exactly on the first
    draw of one f64 case per shape."""
    case = next(c for c in _of("nuts") if c[3] == shape and c[4] == "f64")
    d = cm.build(case)
    st = cm.start(d)
    table = np.stack([cm.entry_of(d, c) for c in range(d["C"])])
    args = (d["fs"], st["theta"], st["target"], st["grad"], d["z"][0], d["u"][0], d["steps"], d["max_depth"],
            (d["form"], table))
    a, b = nr.run_chains(*args), nr.run_chains(*args, draw=nr.nuts_draw_iterative)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert len(set(a["depth"])) >= 3
