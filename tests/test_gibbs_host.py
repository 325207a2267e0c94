"""Gibbs without a GPU: the MLP blocking methods and chunk_evenly against tables recorded from the reference, the numpy
restatement against the reference's own traces (tests/golden/g12_gibbs_traces.npz), the two modes against each other,
and argument errors of the table, the C ABI and the sampler."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from eeyore_amd import _lib as L
from tests.gibbs_restatement import gibbs_draw, spec_target, table_of
from tests.helpers import load, subgroups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = list("abcd")


def _groups():
    z = load("g12_gibbs_traces.npz")
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in TRACES}


def _mlp(dims, bias=None):
    from eeyore_amd.constants import loss_functions
    from eeyore_amd.models import mlp
    n = len(dims) - 1
    hp = mlp.Hyperparameters(dims=list(dims), bias=[bool(b) for b in bias] if bias is not None else None,
                             activations=n * [torch.sigmoid])
    return mlp.MLP(loss=loss_functions['binary_classification'], hparams=hp)


def test_blocking_methods_equal_the_recorded_tables():
    tables = subgroups(load("g12_gibbs_traces.npz"), "blocking")
    assert {"m2_3_1", "m4_3_3", "m2_3_2_1"} <= set(tables) and len(tables) >= 6
    for name, t in tables.items():
        m = _mlp(t["dims"].tolist(), t["bias"].tolist())
        nb = m.num_par_blocks()
        assert nb == len(t["off"]) - 1 == sum(t["dims"][1:]), name
        for b in range(nb):
            idx, l, n = m.annotated_par_block_indices(b)
            assert idx == t["idx"][t["off"][b]:t["off"][b + 1]].tolist(), (name, b)
            assert [l, n] == t["layer_node"][b].tolist() == list(m.layer_and_node_from_par_block(b)), (name, b)
            assert m.par_block_indices(b) == idx
        assert m.starting_par_block_indices() == t["starts"].tolist(), name
        assert [m.starting_par_block_idx(l) for l in range(len(t["starts"]))] == t["starts"].tolist(), name


def test_intended_node_numbering_on_a_widening_model():
    # MLP(4-2-5-3): layer 2 is wider than the layers before it together; the reference's `b % nodes_before` maps two
    # blocks onto one node there, the subtraction gives ten distinct disjoint blocks that cover every parameter
    m = _mlp([4, 2, 5, 3])
    blocks = [m.par_block_indices(b) for b in range(m.num_par_blocks())]
    assert len(blocks) == 10 and len({tuple(b) for b in blocks}) == 10
    flat = [i for b in blocks for i in b]
    assert sorted(flat) == list(range(m.num_params())) and len(set(flat)) == len(flat)
    assert [m.layer_and_node_from_par_block(b) for b in range(10)] == \
        [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 0), (2, 1), (2, 2)]
    with pytest.raises(IndexError):
        m.layer_and_node_from_par_block(10)


def test_chunk_evenly_equals_the_recorded_pairs():
    from eeyore_amd.itertools import chunk_evenly
    table = load("g12_gibbs_traces.npz")["chunks/table"]
    assert len(table) == 12 * 6
    for row in table.tolist():
        length, n, count, sizes = row[0], row[1], row[2], row[3:]
        got = list(chunk_evenly(list(range(length)), n))
        assert [len(c) for c in got] == sizes[:count], (length, n)
        assert [i for c in got for i in c] == list(range(sum(sizes[:count]))), (length, n)
    assert list(chunk_evenly([5, 6, 7, 8], 3)) == [[5, 6, 7, 8]]  # the uneven case: ONE chunk of 4, not 3 + 1
    with pytest.raises(ValueError):
        list(chunk_evenly([1, 2], 0))


@pytest.mark.parametrize("name", TRACES)
def test_restatement_reproduces_reference_traces(name):
    rec = _groups()[name]
    assert float(rec["min_margin"]) >= 1e-6 and float(rec["margin"].min()) == float(rec["min_margin"])
    tf = spec_target(rec)
    blocks, scales = table_of(rec)
    th, tv = rec["theta0"].copy(), float(rec["init_target"])
    assert abs(tf(th) - tv) <= 1e-12 * max(1.0, abs(tv))
    for it in range(rec["z"].shape[0]):
        th, tv, acc, _, margin = gibbs_draw(tf, th, tv, blocks, scales, rec["z"][it], rec["u"][it], mode="reference")
        assert np.array_equal(acc, rec["accepted"][it]), it  # every decision, none left out
        np.testing.assert_allclose(margin, rec["margin"][it], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(th, rec["sample"][it], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(tv, rec["target_val"][it], rtol=1e-9)


def test_fixture_covers_what_it_claims():
    g = _groups()
    for name, rec in g.items():
        acc = rec["accepted"]
        assert 0 < acc.sum() < acc.size and acc.shape == rec["u"].shape, name
    assert np.diff(g["b"]["blk_off"]).tolist() == [3, 3, 3, 4, 2, 2, 3]  # 4 indices with size 3: one chunk of 4
    assert len(set(g["b"]["blk_scale"].tolist())) > 1
    assert g["c"]["bias"].tolist() == [0, 1] and g["d"]["dims"].tolist()[0] == 1
    # the carried rejections are visible: the reference's target_val is not the target of its sample after some draws
    tf = spec_target(g["a"])
    off = sum(abs(tf(s) - t) > 1e-9 for s, t in zip(g["a"]["sample"], g["a"]["target_val"]))
    assert off > 0


@pytest.mark.parametrize("name", TRACES)
def test_intended_mode_keeps_the_target_of_the_state(name):
    rec = _groups()[name]
    tf = spec_target(rec)
    blocks, scales = table_of(rec)
    th, tv = rec["theta0"].copy(), float(rec["init_target"])
    all_accepted = 0
    for it in range(rec["z"].shape[0]):
        ref = gibbs_draw(tf, th, tv, blocks, scales, rec["z"][it], rec["u"][it], mode="reference")
        # a draw whose sub-steps all accept never carries anything: feed uniforms that accept everything
        u_all = np.full(len(blocks), 1e-300)
        a = gibbs_draw(tf, th, tv, blocks, scales, rec["z"][it], u_all, mode="intended")
        b = gibbs_draw(tf, th, tv, blocks, scales, rec["z"][it], u_all, mode="reference")
        if a[2].all():
            all_accepted += 1
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(b[2], a[2])
        th, tv, acc, _, _ = gibbs_draw(tf, th, tv, blocks, scales, rec["z"][it], rec["u"][it], mode="intended")
        assert tv == tf(th), it  # the last accepted evaluation was of exactly this vector
        if ref[2].all():
            assert np.array_equal(ref[0], th)
    assert all_accepted >= rec["z"].shape[0] // 2


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "eeyore_amd.h")).read()
    declared = set(re.findall(r"\b(ey_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ey_gibbs_step", "ey_gibbs_run", "ey_gibbs_table_create", "ey_gibbs_table_destroy",
                 "ey_philox_uniform_blocks"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name), name
    assert "EY_GIBBS_CARRY = 4" in hdr and L.EY_GIBBS_CARRY == 4


def _create(P, blocks, scales, dtype=L.EY_F64):
    from eeyore_amd.plan import gibbs_table_arrays
    off, idx, scl = gibbs_table_arrays(blocks, scales)
    h = ct.c_void_p()
    rc = L.lib().ey_gibbs_table_create(ct.byref(h), P, len(blocks), off, idx, scl, dtype, 0)
    return rc, L.lib().ey_last_error().decode(), h


@pytest.mark.parametrize("blocks,scales,msg", [
    ([], [], "at least one block"),
    ([[0, 1], []], [1.0, 1.0], "empty"),
    ([[0, 1], [2, 5]], [1.0, 1.0], "outside"),
    ([[0, -1]], [1.0], "outside"),
    ([[0, 1], [1, 2]], [1.0, 1.0], "two blocks"),
    ([[0, 1, 2], [3, 4, 0]], [1.0, 1.0], "overlap"),
    ([[0, 1]], [0.0], "positive"),
    ([[0, 1]], [-1.0], "positive"),
    ([[0, 1]], [float("nan")], "positive"),
    ([[0, 1]], [float("inf")], "positive"),
])
def test_table_validation_fails_before_any_device_call(blocks, scales, msg):
    rc, err, h = _create(5, blocks, scales)
    assert rc == -1 and msg in err and not h.value, (rc, err)


def test_c_abi_argument_errors_without_gpu():
    lib = L.lib()
    p = ct.c_void_p(1)
    assert lib.ey_gibbs_step(None, p, p, p, None, None, None, 1, 0, 0, 0, 0, p, None, None) == -1
    assert b"null plan" in lib.ey_last_error()
    assert lib.ey_gibbs_run(None, p, p, p, None, 1, 0, 0, 0, 0, 8, None, None, None, None, p, None) == -1
    assert b"ey_gibbs_run" in lib.ey_last_error()
    assert lib.ey_gibbs_table_destroy(None) == 0
    assert lib.ey_philox_uniform_blocks(None, 1, 1, 0, 0, 0, L.EY_F32, None) == -1


def test_sampler_argument_errors_before_any_launch():
    from eeyore_amd.samplers import Gibbs
    m = _mlp([2, 3, 2, 1])
    assert m.num_par_blocks() == 6
    with pytest.raises(ValueError, match="mode"):
        Gibbs(m, mode="fast")
    with pytest.raises(ValueError, match="6 parameter blocks"):
        Gibbs(m, scales=[1.0, 2.0])
    with pytest.raises(ValueError, match="positive"):
        Gibbs(m, scales=[1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="node_subblock_size"):
        Gibbs(m, node_subblock_size=[None, 2])
    with pytest.raises(ValueError, match="positive integer"):
        Gibbs(m, node_subblock_size=[None, 0, None, None, None, None])
    with pytest.raises(ValueError, match="no sub-block"):
        Gibbs(m, node_subblock_size=[9] * 6)
    from eeyore_amd.datasets import DataCounter
    s = Gibbs(m, scales=0.5, node_subblock_size=[2, None, 3, 3, 2, None], counter=DataCounter(4, 4))
    assert [len(i) for per in s.get_blocks() for i in per] == [3, 3, 3, 4, 2, 2, 3] and s.num_substeps == 7
    assert s.scales.tolist() == [0.5] * 6


def test_save_blocks_writes_the_reference_json(tmp_path, monkeypatch):
    import json
    from eeyore_amd.samplers import Gibbs
    from eeyore_amd.datasets import DataCounter
    s = Gibbs(_mlp([2, 3, 1]), node_subblock_size=[None, 1, None, 2], counter=DataCounter(4, 4))
    monkeypatch.chdir(tmp_path)
    s.save_blocks()
    assert json.load(open(tmp_path / "gibbs_lbocks.txt")) == s.get_blocks()


def test_chain_buffer_holds_a_flag_per_substep():
    from eeyore_amd.chains import ChainBuffer
    buf = ChainBuffer()
    C, P, S = 3, 4, 5
    for it in range(6):
        buf.update(dict(sample=torch.full((C, P), float(it)), target_val=torch.zeros(C),
                        accepted=(torch.arange(C * S).reshape(C, S) % (it + 2) == 0).to(torch.uint8)))
    views = buf.block(2, dict(sample=torch.zeros(C, P), target_val=torch.zeros(C),
                              accepted=torch.zeros(C, S, dtype=torch.uint8)))
    assert views["accepted"].shape == (2, C, S)
    views["accepted"].fill_(1)
    buf.commit(2)
    assert buf.get_accepted().shape == (8, C, S) and buf.acceptance_rate().shape == (C, S)
    assert buf.acceptance_rate()[0, 0].item() == 1.0
    chain = buf.get_chain(1)
    assert len(chain.vals["accepted"]) == 8 and chain.vals["accepted"][0].shape == (S,)
    with pytest.raises(NotImplementedError, match="sub-step"):
        buf.to_chainfiles("unused")
