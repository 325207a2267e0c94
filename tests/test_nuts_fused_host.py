"""NUTS on the matrix cores, without a device: the surface of include/eeyore_amd_nuts_fused.h, the parity cases of
tests/nuts_fused_cases.py held to their margin and coverage conditions by the restatement alone, and the sampler's
``tree='fused'`` on a stub plan."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import nuts_fused_cases as nf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("eeyore_amd.h", "eeyore_amd_ext.h", "eeyore_amd_warmup.h", "eeyore_amd_nuts.h", "eeyore_amd_eslice.h",
                 "eeyore_amd_eslice_fused.h", "eeyore_amd_nuts_tree.h")


def test_header_binding_and_library_agree():
    """Fails on the parent commit: there is no such header, table or symbol."""
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_nuts_fused.h")).read()
    declared = set(re.findall(r"^const char\* (ey_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.NUTS_FUSED_SYMBOLS) == {"ey_nuts_kernel"}, declared
    for table in (L.SYMBOLS, L.EXT_SYMBOLS, L.WARMUP_SYMBOLS, L.NUTS_SYMBOLS, L.ESLICE_SYMBOLS, L.ESLICE_FUSED_SYMBOLS,
                  L.NUTS_TREE_SYMBOLS):
        assert not set(L.NUTS_FUSED_SYMBOLS) & set(table)
    for inc in OTHER_HEADERS:
        assert f'#include "{inc}"' in hdr
    assert "#define EY_NUTS_FUSED 16" in hdr and L.EY_NUTS_FUSED == 16
    # a bit of its own among the flags
    assert not L.EY_NUTS_FUSED & (L.EY_RECOMPUTE_INITIAL_GRAD | L.EY_FORCE_GENERIC | L.EY_GIBBS_CARRY | L.EY_NUTS_TREE_DEVICE)
    lib = L.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert " T ey_nuts_kernel\n" in exported
    res, args = L.NUTS_FUSED_SYMBOLS["ey_nuts_kernel"]
    assert lib.ey_nuts_kernel.restype is res is ct.c_char_p and list(lib.ey_nuts_kernel.argtypes) == list(args)
    # without a plan there is nothing to serve
    for flags in (0, L.EY_NUTS_FUSED, L.EY_NUTS_FUSED | L.EY_FORCE_GENERIC):
        assert lib.ey_nuts_kernel(None, flags) == b"generic"
    # the headers of the sampler and of the tree are as they were
    for name in ("eeyore_amd_nuts.h", "eeyore_amd_nuts_tree.h"):
        assert "FUSED" not in open(os.path.join(ROOT, "include", name)).read().replace("eeyore_amd_eslice_fused", "")


@pytest.mark.parametrize("name", list(nf.CASES))
def test_every_pair_clears_the_floor_and_the_cases_cover_every_outcome(name):
    """What tests/test_nuts_fused_gpu.py relies on, by the restatement alone: every (draw, chain) pair above MARGIN_FLOOR;
    every depth from 0 to max_depth; a draw stopping in each of the four ways; a moved and an unmoved draw."""
    d = nf.setup(name)
    v0, u, outs = nf.restate(name)
    margin = np.stack([o["margin"] for o in outs])
    depth = np.stack([o["depth"] for o in outs])
    stop = np.stack([o["stop"] for o in outs])
    acc = np.stack([o["accepted"] for o in outs])
    tries = np.stack([o["tries"] for o in outs])
    hist = np.bincount(depth.ravel(), minlength=nf.MAX_DEPTH + 1).tolist()
    print(f"{name}: smallest margin {margin.min():.3g}, depths {hist}, stops "
          f"{ {s: int((stop == s).sum()) for s in nf.STOPS} }, moved {int(acc.sum())} of {acc.size}, "
          f"{tries.mean():.2f} attempts per pair (at most {tries.max()})")
    assert margin.shape == (nf.DRAWS, nf.C) and (nf.C, nf.DRAWS, nf.MAX_DEPTH) == (11, 3, 3)
    assert (margin > nf.MARGIN_FLOOR).all() and nf.MARGIN_FLOOR == 0.05
    assert tries.max() <= nf.MAX_TRIES
    assert all(h > 0 for h in hist), hist
    for s in nf.STOPS:
        assert (stop == s).any(), (name, s)
    assert acc.any() and not acc.all()
    # a depth-0 divergent draw: the longest step, a hundred times the prior's stability limit
    assert d["factors"].max() == 100.0 and d["factors"].min() < 0.1
    assert ((depth == 0) & (stop == "divergent")).any()
    # what the device is given holds f32 values, and the metric table lies in [0.5, 1.5]
    for a in (d["theta"], d["steps"], d["tables"], d["prior"][0], d["prior"][1], d["x"], v0, u):
        assert np.array_equal(a, nf.f32(a))
    assert d["tables"].min() >= 0.5 and d["tables"].max() <= 1.5
    assert (d["temps"] is not None) == ("temp" in name) and (d["index"] is not None) == ("index" in name)
    if d["index"] is not None:
        assert d["tables"].shape[0] == 3 and set(d["index"].tolist()) == {0, 1, 2}
    # the restatement is deterministic on the stored tables: the second draw again, from its recorded start
    again = nf.restate_draw(name, outs[1]["start_theta"], outs[1]["start_target"], outs[1]["start_grad"], v0[1], u[1])
    for key in ("depth", "n_leapfrog", "accepted", "margin"):
        assert np.array_equal(again[key], outs[1][key]), key


def _model():
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['multiclass_classification'],
                   hparams=mlp.Hyperparameters(dims=[4, 32, 32, 3], bias=3 * [True],
                                               activations=[torch.sigmoid, torch.sigmoid, None]))


def test_fused_keyword_on_a_stub_plan(monkeypatch):
    """Fails on the parent commit: tree='fused' is refused there."""
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.samplers import NUTS, DenseMetric, DiagMetric, HMC
    dl = DataLoader(EmptyXYDataset())
    monkeypatch.setattr(HMC, "set_current", lambda self, theta, data=None: None)  # (no device here)
    model = _model()
    P, C = model.num_params(), 4
    assert P == 1315
    th0 = torch.zeros(C, P, dtype=model.dtype)
    with pytest.raises(ValueError, match="tree must be"):
        NUTS(model, theta0=th0, dataloader=dl, tree='bogus')
    for metric in (None, 'diag', DiagMetric(torch.full((P,), 0.5, dtype=model.dtype))):
        s = NUTS(model, theta0=th0, dataloader=dl, tree='fused', metric=metric, max_depth=6)
        assert s.tree == 'fused' and s._metric_form == 'diag' and tuple(s._metric.shape) == (P,) and s.max_depth == 6
    for metric in ('dense', DenseMetric(torch.eye(5, dtype=model.dtype))):
        with pytest.raises(ValueError, match="diagonal metric only"):
            NUTS(model, theta0=th0, dataloader=dl, tree='fused', metric=metric)
    with pytest.raises(ValueError, match="diagonal metric only"):
        s._set_metric(DenseMetric(torch.eye(5, dtype=model.dtype)))

    class StubPlan:
        kernel = "mfma32"

        def __init__(self, serves):
            self.serves, self.attached, self.asked = serves, [], []

        def nuts_kernel(self, flags=0):
            self.asked.append(flags)
            return "mfma32" if self.serves and flags & L.EY_NUTS_FUSED else "generic"

        def attach_nuts_tree(self, C, max_depth):
            self.attached.append((C, max_depth))

    # the flags of a launch: the plan it is about to run on is asked, then gets the workspace
    s = NUTS(model, theta0=th0, dataloader=dl, tree='fused', max_depth=6, recompute_initial_grad=True)
    plan = StubPlan(True)
    assert s._flags(plan) == L.EY_NUTS_FUSED | L.EY_RECOMPUTE_INITIAL_GRAD
    assert plan.attached == [(C, 6)] and plan.asked == [L.EY_NUTS_FUSED]
    # a plan that is not served: a ValueError that names plan.kernel, nothing attached
    other = StubPlan(False)
    other.kernel = "fused16"
    with pytest.raises(ValueError, match="fused16"):
        s._flags(other)
    assert other.attached == []
    # 'device' and 'lds' pass what they passed
    dev = NUTS(model, theta0=th0, dataloader=dl, tree='device', max_depth=6)
    plan = StubPlan(True)
    assert dev._flags(plan) == L.EY_NUTS_TREE_DEVICE and plan.attached == [(C, 6)] and plan.asked == []


def test_plan_lifts_the_limit_of_128_parameters_for_the_fused_flag_and_the_diagonal_form():
    from eeyore_amd.plan import Plan

    class Stub:
        P = 1315
        _nuts_args = Plan._nuts_args

        def _theta(self, theta):
            return 3

        def _metric(self, metric, form, index, C):
            raise KeyError("reached the metric")

    with pytest.raises(ValueError, match="limited to 128 parameters"):
        Stub()._nuts_args(None, None, "dense", None, 5, None, L.EY_NUTS_FUSED)
    for flags in (L.EY_NUTS_FUSED, L.EY_NUTS_FUSED | L.EY_NUTS_TREE_DEVICE):
        with pytest.raises(KeyError, match="reached the metric"):
            Stub()._nuts_args(None, None, "diag", None, 5, None, flags)
