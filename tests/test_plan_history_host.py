"""The script generator and the configuration record of tests/plan_history.py, without a device: the scripts are
reproducible from their seed, every script holds the coverage the GPU test relies on, and the calls that build a fresh plan
carry every field of the record.  Also the index check of Plan._tril / Plan._metric on a stub plan: it must not be skipped
for a tensor that merely has the address and version counter of the one it saw before."""
import dataclasses

import pytest
import torch

from tests import plan_history as H

NAMES = [f.name for f in H.FAMILY_LIST]


def _walk(name, ops):
    """(record before, operation, record after) of every operation of a script."""
    cfg = H.start(H.FAMILY[name])
    for op in ops:
        new = H.after(cfg, op)
        yield cfg, op, new
        cfg = new


def test_families_are_the_rows_of_the_small_batch_suite():
    assert len(set(NAMES)) == len(NAMES) == 14
    for name, kernel, P in (("mfma32-bf16x3", "mfma32", 1315), ("fused16-f32", "fused16", 4676),
                            ("layerwise-784-f32", "bgemm", 101770), ("k_mid32", "bgemm", 3434), ("k_mid", "bgemm", 2110)):
        assert (H.FAMILY[name].kernel, H.FAMILY[name].P) == (kernel, P)
    assert H.FAMILY["layerwise-784-f32"].variant == 16 | 16384 and H.FAMILY["k_mid"].variant == 16 | 8192
    assert not any("rowwaves" in n for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_script_is_reproducible_from_its_seed(name):
    assert H.script(name) == H.script(name)
    assert H.script(name) != H.script(name, seed=H.SEED + 1)


@pytest.mark.parametrize("name", NAMES)
def test_script_meets_the_coverage_conditions(name):
    fam, ops = H.FAMILY[name], H.script(name)
    assert len(ops) >= H.SCRIPT_LEN
    steps = list(_walk(name, ops))
    for i, (cfg, op, _) in enumerate(steps):
        assert H.legal(cfg, op), (i, op, cfg)
    seen = {op[0] for op in ops}
    assert set(H.kinds(fam)) <= seen, set(H.kinds(fam)) - seen
    # every adjacent pair of the family's row counts, crossed by one data operation in each direction
    moves = {(cfg.n, new.n) for cfg, op, new in steps if op[0] == "data_n"}
    for a, b in zip(fam.ns, fam.ns[1:]):
        assert (a, b) in moves and (b, a) in moves, (a, b)
    # a refused call leaves the record as it was (and the runner probes behind every operation, refused ones included)
    for cfg, op, new in steps:
        if op[0] in H.REFUSALS:
            assert new == cfg, op
    if fam.kind == "mlp":
        assert {r for r in H.REFUSALS if r in seen} >= {"bad_sigma", "bad_df", "bad_cols", "bad_theta_dtype"}
        assert ("bad_lik_scale" in seen) == (fam.lik == 2)
    else:
        assert {"bad_index", "bad_theta_dtype"} <= seen
    if fam.priors:   # the other prior families are left for Normal again
        priors = [new.prior[0] for _, op, new in steps if op[0].startswith("prior_")]
        assert any(a in H.FAMILY_PRIORS and b in H.NORMAL_PRIORS for a, b in zip(priors, priors[1:])), priors
    # attachments: something is probed while attached and again after the detach
    assert any(cfg.moments is not None and new.moments is None for cfg, _, new in steps)
    if fam.fused:
        assert any(cfg.da is not None and new.da is None for cfg, _, new in steps)
        assert all(new.da is None or new.prior[0] in H.NORMAL_PRIORS for _, _, new in steps)


@pytest.mark.parametrize("name", NAMES)
def test_record_round_trips_through_the_calls_that_build_a_plan(name):
    k = 0
    for cfg, _, new in _walk(name, H.script(name)):
        k += 1
        new = H.after_probe(new, H.probe_hmc_iters(new, k))
        assert H.record_of(H.setup_calls(new)) == new
    fields = {f.name for f in dataclasses.fields(H.Config)} - {"family"}
    changed = {f for cfg, _, new in _walk(name, H.script(name)) for f in fields if getattr(cfg, f) != getattr(new, f)}
    if H.FAMILY[name].kind == "mlp":
        assert {"n", "data_seed", "bumps", "prior", "row_waves", "moments"} <= changed, changed


def test_attached_dual_averaging_counts_the_probes_draws():
    cfg = dataclasses.replace(H.start(H.FAMILY["fused16-f64"]), da=(3, 7, 0))
    assert H.probe_hmc_iters(cfg, 1) == 1 and H.probe_hmc_iters(cfg, 4) == 1 + H.RUN_ITERS
    assert H.after_probe(cfg, 4).da == (3, 7, 4) and H.probe_chains(cfg, 2) == 3
    assert H.after_probe(dataclasses.replace(cfg, da=None), 4).da is None


# ------------------------------------------------------------------------------------------- the index check, on a stub
def _stub(P=3):
    from eeyore_amd.plan import Plan
    pl = Plan.__new__(Plan)
    pl.device, pl.dtype, pl.P = torch.device("cpu"), torch.float64, P
    return pl


@pytest.mark.parametrize("through", ["_tril", "_metric"])
def test_index_check_is_not_skipped_for_another_tensor_at_the_same_address(through):
    """Two index tensors over one storage, both with version counter 1, the contents rewritten to G in between through a
    third: the second must be range-checked (an address-based key matched it and let G through to the kernel)."""
    G, C = 2, 4
    pl = _stub()
    storage = torch.zeros(C, dtype=torch.int32).untyped_storage()

    def alias():
        return torch.empty(0, dtype=torch.int32).set_(storage, 0, (C,))

    def check(index):
        if through == "_tril":
            return pl._tril(torch.zeros(G, pl.P, pl.P, dtype=pl.dtype), index, C)[1]
        return pl._metric(torch.ones(G, pl.P, dtype=pl.dtype), "diag", index, C)[2]

    first = alias()
    assert check(first) is first and check(first) is first
    alias().fill_(G)
    second = alias()
    assert second.data_ptr() == first.data_ptr() and second._version == first._version and second.tolist() == [G] * C
    with pytest.raises(ValueError, match=r"index must lie in \[0, 2\)"):
        check(second)
    second.zero_()                                                 # in place: the version counter moves, it is read again
    assert check(second) is second
    second.fill_(-1)
    with pytest.raises(ValueError, match=r"index must lie in \[0, 2\)"):
        check(second)
