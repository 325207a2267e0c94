"""Elliptical slice sampling on the matrix cores without a device: the sixth header, its binding table and the library
agree, and the committed inputs of tests/eslice_fused_cases.py meet the margin rules of tests/test_eslice_fused_gpu.py with
the f64 restatement alone."""
import os
import re
import subprocess

import numpy as np
import pytest

from eeyore_amd import _lib as L
from tests import eslice_fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("eeyore_amd.h", "eeyore_amd_ext.h", "eeyore_amd_warmup.h", "eeyore_amd_nuts.h", "eeyore_amd_eslice.h")


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd_eslice_fused.h")).read()
    declared = set(re.findall(r"^(?:const char\*|int) (ey_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.ESLICE_FUSED_SYMBOLS) == {"ey_eslice_kernel"}, declared
    for inc in OTHER_HEADERS:
        assert f'#include "{inc}"' in hdr
        assert "ey_eslice_kernel" not in open(os.path.join(ROOT, "include", inc)).read()
    for table in (L.SYMBOLS, L.EXT_SYMBOLS, L.WARMUP_SYMBOLS, L.NUTS_SYMBOLS, L.ESLICE_SYMBOLS):
        assert not set(L.ESLICE_FUSED_SYMBOLS) & set(table)
    lib = L.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    res, args = L.ESLICE_FUSED_SYMBOLS["ey_eslice_kernel"]
    assert " T ey_eslice_kernel\n" in exported
    fn = lib.ey_eslice_kernel
    assert fn.restype is res and list(fn.argtypes) == list(args)
    proto = hdr[hdr.index("const char* ey_eslice_kernel("):]
    assert proto[:proto.index(");")].count(",") + 1 == len(args) == 2
    assert fn(None, 0) == b"generic" and fn(None, L.EY_FORCE_GENERIC) == b"generic"   # no plan, no device
    from eeyore_amd.plan import Plan
    assert callable(Plan.eslice_kernel)


def test_cases_cover_what_the_kernel_serves():
    rows = {case["N"] for case in fc.CASES.values()}
    assert rows == {5, 33, 150}
    flags = {key for case in fc.CASES.values() for key in case}
    assert {"temp", "prior", "base", "max_shrinks", "model", "products"} <= flags
    assert fc.CASES["n33/shrinks2"]["max_shrinks"] == 2 and fc.CASES["n150/exact"]["products"] == "exact"
    assert fc.BCE_TANH == dict(dims=[4, 32, 32, 1], acts=[2, 2, 1], lik=0) and fc.C == 11 and fc.DRAWS == 4
    for name in fc.CASES:
        d = fc.inputs(name)
        for key in ("x", "theta", "z", "u"):   # what the device is given is what the restatement saw
            assert np.array_equal(d[key], d[key].astype(np.float32).astype(np.float64)), (name, key)
        if d["temps"] is not None:
            assert d["temps"].min() >= 0.4 and d["temps"].max() <= 1.0
        assert abs(d["x"].mean()) < 0.5 and len(np.unique(d["y"], axis=0)) >= 2 and d["theta"].shape == (fc.C, 1315 if d["y"].shape[1] == 3 else 1249)
    p = fc.inputs("n33/prior")["prior"]
    assert len(np.unique(p[0])) > 1000 and len(np.unique(p[1])) > 1000
    m, s = fc.inputs("n150/base")["base"]
    assert np.all(m != fc.inputs("n150/base")["prior"][0]) and np.all(s > fc.inputs("n150/base")["prior"][1])


@pytest.mark.parametrize("name", list(fc.CASES))
def test_committed_inputs_meet_the_margin_rule(name):
    """At an ell-margin of 2e-2 -- the largest tolerance the device test may use -- and an angle margin of 1e-5, at most
    10 % of a case's 44 pairs are set aside."""
    under, stayed, evals = fc.summary(name, fc.ELL_MARGIN_MAX)
    print(f"{name}: {under} of {fc.PAIRS} pairs under the margins, {stayed} stayed, {evals:.2f} evaluations per draw")
    assert under <= fc.MAX_UNDER * fc.PAIRS
    for o in fc.restate(name):
        assert np.isfinite(o["start_ell"]).all() and np.isfinite(o["ell"]).all() and (o["n_evals"] >= 1).all()
    if fc.inputs(name)["max_shrinks"] == 2:
        assert 1 <= stayed <= fc.PAIRS - 1 and max(int(o["n_evals"].max()) for o in fc.restate(name)) == 3
    else:
        assert stayed == 0 and evals > 2.0
