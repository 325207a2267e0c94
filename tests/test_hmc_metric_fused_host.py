"""HMC under a diagonal metric on the matrix cores, without a device: the surface of include/eeyore_amd_hmc_metric_fused.h, the
parity cases of tests/hmc_metric_fused_cases.py held to their margin and coverage conditions by the restatement alone, and the
sampler's ``metric_kernel='fused'`` on a stub plan."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import hmc_metric_fused_cases as hc
from tests import hmc_metric_restatement as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("eeyore_amd.h", "eeyore_amd_ext.h", "eeyore_amd_warmup.h", "eeyore_amd_nuts.h", "eeyore_amd_eslice.h",
                 "eeyore_amd_eslice_fused.h", "eeyore_amd_nuts_tree.h", "eeyore_amd_nuts_fused.h")


def test_header_binding_and_library_agree():
    """Fails on the parent commit: there is no such header, table or symbol."""
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_hmc_metric_fused.h")).read()
    declared = set(re.findall(r"^const char\* (ey_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.HMC_METRIC_FUSED_SYMBOLS) == {"ey_hmc_metric_kernel"}, declared
    for table in (L.SYMBOLS, L.EXT_SYMBOLS, L.WARMUP_SYMBOLS, L.NUTS_SYMBOLS, L.ESLICE_SYMBOLS, L.ESLICE_FUSED_SYMBOLS,
                  L.NUTS_TREE_SYMBOLS, L.NUTS_FUSED_SYMBOLS):
        assert not set(L.HMC_METRIC_FUSED_SYMBOLS) & set(table)
    for inc in OTHER_HEADERS:
        assert f'#include "{inc}"' in hdr
    assert "#define EY_HMC_METRIC_FUSED 32" in hdr and L.EY_HMC_METRIC_FUSED == 32
    # a bit of its own among the flags
    others = (L.EY_RECOMPUTE_INITIAL_GRAD, L.EY_FORCE_GENERIC, L.EY_GIBBS_CARRY, L.EY_NUTS_TREE_DEVICE, L.EY_NUTS_FUSED)
    assert sorted(others) == [1, 2, 4, 8, 16] and not any(L.EY_HMC_METRIC_FUSED & o for o in others)
    lib = L.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert " T ey_hmc_metric_kernel\n" in exported
    res, args = L.HMC_METRIC_FUSED_SYMBOLS["ey_hmc_metric_kernel"]
    assert lib.ey_hmc_metric_kernel.restype is res is ct.c_char_p and list(lib.ey_hmc_metric_kernel.argtypes) == list(args)
    # without a plan there is nothing to serve
    for flags in (0, L.EY_HMC_METRIC_FUSED, L.EY_HMC_METRIC_FUSED | L.EY_FORCE_GENERIC):
        assert lib.ey_hmc_metric_kernel(None, flags) == b"generic"
    # the headers of the entry points are as they were
    for name in ("eeyore_amd_ext.h", "eeyore_amd_warmup.h"):
        assert "FUSED" not in open(os.path.join(ROOT, "include", name)).read()


@pytest.mark.parametrize("name", list(hc.CASES))
def test_every_pair_clears_the_floor_and_the_cases_cover_both_decisions(name):
    """What tests/test_hmc_metric_fused_gpu.py relies on, by the restatement alone: every (draw, chain) pair above MARGIN_FLOOR
    -- a condition: no pair is left out of the device comparison --, an accepted and a rejected pair, the hundredfold step
    blown and rejected, and a gap between the blown pairs and the others."""
    d = hc.setup(name)
    v0, u, outs = hc.restate(name)
    margin = np.stack([o["margin"] for o in outs])
    acc = np.stack([o["accepted"] for o in outs]).astype(bool)
    bl = np.stack([hc.blown(o) for o in outs])
    hp = np.stack([o["h_prop"] for o in outs])
    tries = np.stack([o["tries"] for o in outs])
    print(f"{name}: L {d['L']}, smallest margin {margin.min():.3g}, accepted {int(acc.sum())} of {acc.size}, blown {int(bl.sum())}, "
          f"non-finite H_prop {int((~np.isfinite(hp)).sum())}, largest calm |H_prop| {np.abs(hp[~bl]).max():.4g}, "
          f"{tries.mean():.2f} attempts per pair (at most {tries.max()})")
    assert margin.shape == (hc.DRAWS, hc.C) and (hc.C, hc.DRAWS) == (11, 3)
    assert (margin > hc.MARGIN_FLOOR).all() and hc.MARGIN_FLOOR == 0.05
    assert tries.max() <= hc.MAX_TRIES
    assert acc.any() and not acc.all()
    # the longest step, a hundred times the prior's stability limit: blown, rejected; the others calm
    assert d["factors"].max() == 100.0 and d["factors"].min() == 0.02
    assert bl[:, -1].all() and not bl[:, :-1].any() and not acc[bl].any()
    assert np.abs(hp[~bl]).max() <= hc.CALM < hc.BLOWN
    # rejected pairs that are not blown, too: a finite H_prop uphill of H_cur is compared on the device
    assert (~acc & ~bl).any()
    # what the device is given holds f32 values, and the metric table lies in [0.5, 1.5]
    for a in (d["theta"], d["steps"], d["tables"], d["prior"][0], d["prior"][1], d["x"], v0, u):
        assert np.array_equal(a, hc.f32(a))
    assert d["tables"].min() >= 0.5 and d["tables"].max() <= 1.5 and (u > 0).all() and (u < 1).all()
    assert (d["temps"] is not None) == ("temp" in name) and (d["index"] is not None) == ("index" in name)
    if d["index"] is not None:
        assert d["tables"].shape[0] == 3 and set(d["index"].tolist()) == {0, 1, 2}
    # the restatement is deterministic on the stored tables: the second draw again, from its recorded start
    again = hc.restate_draw(name, outs[1]["start_theta"], outs[1]["start_target"], outs[1]["start_grad"], v0[1], u[1])
    for key in ("accepted", "margin", "h_prop"):
        assert np.array_equal(again[key], outs[1][key], equal_nan=key != "accepted"), key


def test_the_cases_are_the_ones_the_kernel_can_go_wrong_on():
    assert list(hc.CASES) == ["n33/L1", "n33", "n150", "n150/bce-tanh", "n33/exact", "n33/prior/temp", "n33/index", "n330"]
    assert hc.setup("n33/L1")["L"] == 1 and hc.setup("n150")["L"] == 8 and hc.setup("n330")["L"] == 3
    d = hc.setup("n330")
    assert d["x"].shape == (330, 4) and (330 + 31) // 32 > 10   # more row tiles than MF_TRD_TILES
    x150, lab150 = hc.rows_of(150)
    x330, lab330 = hc.rows_of(330)
    assert np.array_equal(x330[:150], x150) and np.array_equal(lab330[150:300], lab150) and np.array_equal(lab330[300:], lab150[:30])
    assert not np.array_equal(x330[150:300], x150) and np.abs(x330[150:300] - x150).max() < 0.5
    # some case has a NaN or infinite H_prop
    assert any(hc.coverage(name)[3] > 0 for name in hc.CASES)


def test_the_draw_equals_the_draw_in_the_momentum():
    name = "n33"
    d, fs = hc.setup(name), hc.chain_functions(name)
    v0, u, outs = hc.restate(name)
    o = outs[0]
    for c in (0, 3, 7):
        a = hc.one_draw(name, fs, c, o["start_theta"][c], o["start_target"][c], o["start_grad"][c], v0[0, c], u[0, c])
        b = hc.one_draw(name, fs, c, o["start_theta"][c], o["start_target"][c], o["start_grad"][c], v0[0, c], u[0, c],
                        draw=hr.hmc_metric_draw_momentum)
        assert a["accepted"] == b["accepted"] == o["accepted"][c]
        for key in ("h_cur", "h_prop", "rate", "target"):
            assert abs(a[key] - b[key]) <= 1e-9 * max(1.0, abs(a[key])), (c, key, a[key], b[key])
        np.testing.assert_allclose(a["theta"], b["theta"], rtol=0, atol=1e-11)
        np.testing.assert_allclose(a["grad"], b["grad"], rtol=0, atol=1e-9 * np.abs(a["grad"]).max())


def test_the_device_tolerances_follow_the_probes_figures_and_stay_below_the_floor():
    """TAU of tests/test_hmc_metric_fused_gpu.py is 8 x the figure the probe recorded on the parent's path, rounded up to one
    digit, and the TAUs of the quantities a decision is made on do not exceed MARGIN_FLOOR."""
    import math
    from tests import test_hmc_metric_fused_gpu as tg
    assert set(tg.E_PARENT) == set(tg.TAU) == set(hc.VALUES)
    for key, e in tg.E_PARENT.items():
        digit = 10.0 ** math.floor(math.log10(8 * e))
        assert math.isclose(tg.TAU[key], math.ceil(8 * e / digit - 1e-9) * digit, rel_tol=1e-9), key
    assert max(tg.TAU["target"], tg.TAU["h_cur"], tg.TAU["h_prop"]) <= hc.MARGIN_FLOOR


def test_identity_restatement_is_conditioned_too():
    for name in ("n33", "n150/bce-tanh"):
        u, ref = hc.restate_identity(name)
        assert (ref["margin"] > hc.MARGIN_FLOOR).all() and ref["accepted"].any() and not ref["accepted"].all()
        assert np.array_equal(u, hc.f32(u))


def _model():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['multiclass_classification'],
                   hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                               activations=[torch.sigmoid, torch.sigmoid, None]))


def test_metric_kernel_keyword_on_a_stub_plan(monkeypatch):
    """Fails on the parent commit: HMC has no metric_kernel there."""
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.samplers import HMC, NUTS, DenseMetric, DiagMetric
    dl = DataLoader(EmptyXYDataset())
    monkeypatch.setattr(HMC, "set_current", lambda self, theta, data=None: None)  # (no device here)
    model = _model()
    P, C = model.num_params(), 4
    assert P == 1315
    th0 = torch.zeros(C, P, dtype=model.dtype)
    with pytest.raises(ValueError, match="metric_kernel must be"):
        HMC(model, theta0=th0, dataloader=dl, metric='diag', metric_kernel='bogus')
    for metric in ('diag', DiagMetric(torch.full((P,), 0.5, dtype=model.dtype))):
        s = HMC(model, theta0=th0, dataloader=dl, metric=metric, metric_kernel='fused')
        assert s.metric_kernel == 'fused' and s._metric_form == 'diag' and tuple(s._metric.shape) == (P,)
    for metric in (None, 'dense', DenseMetric(torch.eye(5, dtype=model.dtype))):
        with pytest.raises(ValueError, match="diagonal metric only"):
            HMC(model, theta0=th0, dataloader=dl, metric=metric, metric_kernel='fused')
    with pytest.raises(ValueError, match="diagonal metric only"):
        s._set_metric(DenseMetric(torch.eye(5, dtype=model.dtype)))
    with pytest.raises(ValueError, match="diagonal metric only"):
        s._set_metric(None)

    class StubPlan:
        kernel = "mfma32"

        def __init__(self, serves):
            self.serves, self.asked = serves, []

        def hmc_metric_kernel(self, flags=0):
            self.asked.append(flags)
            return "mfma32" if self.serves and flags & L.EY_HMC_METRIC_FUSED else "generic"

    plan = StubPlan(True)
    assert s._metric_flags(plan) == L.EY_HMC_METRIC_FUSED and plan.asked == [L.EY_HMC_METRIC_FUSED]
    other = StubPlan(False)
    other.kernel = "fused16"
    with pytest.raises(ValueError, match="fused16"):
        s._metric_flags(other)
    # the default, and NUTS, pass what they passed: the plan is not even asked
    plain = HMC(model, theta0=th0, dataloader=dl, metric='diag')
    plan = StubPlan(True)
    assert plain.metric_kernel == 'generic' and plain._metric_flags(plan) == 0 and plan.asked == []
    assert HMC(model, theta0=th0, dataloader=dl)._metric_flags(plan) == 0
    nuts = NUTS(model, theta0=th0, dataloader=dl, tree='device', max_depth=4)
    assert nuts._metric_flags(plan) == 0 and plan.asked == []
