"""NUTS with its tree in device memory, without a device: the surface of include/eeyore_amd_nuts_tree.h, the parity inputs
of tests/nuts_tree_cases.py held to the coverage and margin rules by the restatement alone, the sampler's ``tree`` keyword
on a stub plan, and the workspace's size."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests import nuts_tree_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("eeyore_amd.h", "eeyore_amd_ext.h", "eeyore_amd_warmup.h", "eeyore_amd_nuts.h", "eeyore_amd_eslice.h",
                 "eeyore_amd_eslice_fused.h")


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_nuts_tree.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t) (ey_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.NUTS_TREE_SYMBOLS) == {"ey_nuts_tree_bytes", "ey_plan_attach_nuts_tree"}, declared
    for table in (L.SYMBOLS, L.EXT_SYMBOLS, L.WARMUP_SYMBOLS, L.NUTS_SYMBOLS, L.ESLICE_SYMBOLS, L.ESLICE_FUSED_SYMBOLS):
        assert not set(L.NUTS_TREE_SYMBOLS) & set(table)
    for inc in OTHER_HEADERS:
        assert f'#include "{inc}"' in hdr
    assert "#define EY_NUTS_TREE_DEVICE 8" in hdr and L.EY_NUTS_TREE_DEVICE == 8
    # a bit of its own among the flags
    assert not L.EY_NUTS_TREE_DEVICE & (L.EY_RECOMPUTE_INITIAL_GRAD | L.EY_FORCE_GENERIC | L.EY_GIBBS_CARRY)
    lib = L.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for name, (res, args) in L.NUTS_TREE_SYMBOLS.items():
        assert f" T {name}\n" in exported, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        proto = hdr[re.search(r"^(?:int|int64_t) " + name + r"\(", hdr, re.M).start():]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == len(args), name
    assert L.NUTS_TREE_SYMBOLS["ey_nuts_tree_bytes"][0] is ct.c_int64
    # the header of the sampler itself is as it was: three entry points
    nuts = open(os.path.join(ROOT, "include", "eeyore_amd_nuts.h")).read()
    assert "nuts_tree" not in nuts and "EY_NUTS_TREE_DEVICE" not in nuts


@pytest.mark.parametrize("name", list(tc.CASES))
def test_parity_inputs_cover_every_outcome_and_stay_clear_of_the_margin(name):
    """What tests/test_nuts_tree_gpu.py relies on, by the restatement alone: at most 5 % of the (chain, draw) pairs within
    the margin, a divergent draw, a draw of depth 0 and one at max_depth, and a tree ended by a U-turn between."""
    case = tc.CASES[name]
    assert tc.num_params(name) > 128
    outs = tc.restated(name)
    margin = np.stack([o["margin"] for o in outs])
    depth = np.stack([o["depth"] for o in outs])
    stop = np.stack([o["stop"] for o in outs])
    div = int(sum(o["divergent"].sum() for o in outs))
    hist = np.bincount(depth.ravel(), minlength=case["max_depth"] + 1).tolist()
    print(f"{name}: {(margin > tc.MARGIN).sum()} of {margin.size} above the margin, smallest {margin.min():.2g}, "
          f"depths {hist}, divergent {div}")
    assert margin.shape == (case["draws"], case["C"])
    assert (margin <= tc.MARGIN).mean() <= tc.MAX_UNDER, margin.min()
    assert div >= 1
    assert hist[0] > 0 and hist[case["max_depth"]] > 0, hist
    uturn = np.isin(stop, ("tree", "subblock")) & (depth > 0) & (depth < case["max_depth"])
    assert uturn.any(), (stop, depth)


def test_the_iris_case_has_a_u_turn_at_depth_three_with_seven_leaves():
    outs = tc.restated("iris4-32-32-3/diag")
    assert any(((o["stop"] == "tree") & (o["depth"] == 3) & (o["n_leapfrog"] == 7)).any() for o in outs)


def _model(dims):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=mlp.Hyperparameters(dims=list(dims)))


def test_tree_keyword_on_a_stub_plan(monkeypatch):
    from torch.utils.data import DataLoader
    from eeyore_amd.datasets import EmptyXYDataset
    from eeyore_amd.samplers import NUTS, DenseMetric, DiagMetric, HMC
    from eeyore_amd.tuners import WindowedAdaptation
    dl = DataLoader(EmptyXYDataset())
    monkeypatch.setattr(HMC, "set_current", lambda self, theta, data=None: None)  # (no device here)
    big = _model((8, 14, 1))
    P, C = big.num_params(), 4
    assert P == 141
    th0 = torch.zeros(C, P, dtype=big.dtype)
    # 'lds' is the sampler as it was, refusals included, named or not
    for kw in ({}, dict(tree='lds'), dict(tree='lds', metric='diag')):
        with pytest.raises(ValueError, match="limited to 128 parameters"):
            NUTS(big, theta0=th0, dataloader=dl, **kw)
    with pytest.raises(ValueError, match="'lds' or 'device'"):
        NUTS(big, theta0=th0, dataloader=dl, tree='global')
    # 'device' lifts the limit for a diagonal metric in each of its spellings
    for metric in (None, 'diag', DiagMetric(torch.full((P,), 0.5, dtype=big.dtype))):
        s = NUTS(big, theta0=th0, dataloader=dl, tree='device', metric=metric, max_depth=6)
        assert s.tree == 'device' and s._metric_form == 'diag' and tuple(s._metric.shape) == (P,) and s.max_depth == 6
    s = NUTS(big, theta0=th0, dataloader=dl, tree='device', tuner=WindowedAdaptation(num_steps=1))
    assert callable(s._warmup_launch)
    for metric in ('dense', DenseMetric(torch.eye(5, dtype=big.dtype))):
        with pytest.raises(ValueError, match="diagonal metric only"):
            NUTS(big, theta0=th0, dataloader=dl, tree='device', metric=metric)
    with pytest.raises(ValueError, match="diagonal metric only"):
        s._set_metric(DenseMetric(torch.eye(5, dtype=big.dtype)))
    # at a small model both are accepted, and the default is 'lds'
    small = _model((2, 2, 1))
    ths = torch.zeros(C, small.num_params(), dtype=small.dtype)
    assert NUTS(small, theta0=ths, dataloader=dl).tree == 'lds'
    assert NUTS(small, theta0=ths, dataloader=dl, tree='device').tree == 'device'

    # the flags of a launch: the plan it is about to run on gets the workspace first
    class StubPlan:
        attached = []

        def attach_nuts_tree(self, C, max_depth):
            self.attached.append((C, max_depth))

    s = NUTS(big, theta0=th0, dataloader=dl, tree='device', max_depth=6, recompute_initial_grad=True)
    plan = StubPlan()
    assert s._flags(plan) == L.EY_NUTS_TREE_DEVICE | L.EY_RECOMPUTE_INITIAL_GRAD and plan.attached == [(C, 6)]
    s = NUTS(small, theta0=ths, dataloader=dl)
    assert s._flags(plan) == 0 and plan.attached == [(C, 6)]


def test_plan_refuses_large_p_without_the_flag_and_the_diagonal_form():
    """Plan._nuts_args skips its P check only for the flag with 'diag' (on an object with the attributes it reads)."""
    from eeyore_amd.plan import Plan

    class Stub:
        P = 141
        _nuts_args = Plan._nuts_args

        def _theta(self, theta):
            return 3

        def _metric(self, metric, form, index, C):
            raise KeyError("reached the metric")

    for flags, form in ((0, "diag"), (L.EY_RECOMPUTE_INITIAL_GRAD, "diag"), (L.EY_NUTS_TREE_DEVICE, "dense")):
        with pytest.raises(ValueError, match="limited to 128 parameters"):
            Stub()._nuts_args(None, None, form, None, 5, None, flags)
    with pytest.raises(KeyError, match="reached the metric"):
        Stub()._nuts_args(None, None, "diag", None, 5, None, L.EY_NUTS_TREE_DEVICE | L.EY_RECOMPUTE_INITIAL_GRAD)


def test_tree_bytes_refuses_a_null_plan():
    assert L.lib().ey_nuts_tree_bytes(None, 4, 5) == -1
    assert b"null plan" in L.lib().ey_last_error()
    assert L.lib().ey_plan_attach_nuts_tree(None, None, 0) == -1
