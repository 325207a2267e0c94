"""A plan's results do not depend on what it served before ("A plan's history").

One plan per kernel family lives through a seeded script of reconfigurations (tests/plan_history.py): batches of other
sizes across the kernels' limits, the same batch objects unmodified and changed in place, other priors and prior families,
options, attached moments and dual averaging, a 1024-chain call, and calls that are refused.  After EVERY operation the
plan is probed beside a plan created at that moment directly in the configuration the record holds, and every output of the
two probes must have the same bits.  Then the two defects the issue names, each pinned on its own."""
import pytest
import torch

from tests import plan_history as H

pytestmark = pytest.mark.gpu

DEV = H.DEV


@pytest.mark.parametrize("name", [f.name for f in H.FAMILY_LIST])
def test_plan_answers_as_a_fresh_plan_after_every_operation(name):
    fam, ops = H.FAMILY[name], H.script(name)
    live = H.build(H.start(fam))
    assert live.plan.kernel == fam.kernel and live.plan.P == fam.P, (name, live.plan.kernel, live.plan.P)

    def check(k, what):
        twin = H.build(live.cfg, like=live)
        a, b = H.probe(live, k), H.probe(twin, k)
        torch.cuda.synchronize()
        diff = H.first_difference(a, b)
        assert diff is None, (f"{name}: after operation {k} {what}, {diff} differs from a fresh plan's in {live.cfg} "
                              f"(script of seed {H.SEED}, operations so far: {ops[:k]})")
        assert any(n.startswith("hmc_step") for n, _ in a) and len(a) > 20
        live.cfg = H.after_probe(live.cfg, H.probe_hmc_iters(live.cfg, k))

    check(0, "(the start)")
    for k, op in enumerate(ops, 1):
        raised = H.apply(live, op)
        if op[0] in H.REFUSALS:
            assert isinstance(raised, ValueError), f"{name}: operation {k} {op} was not refused"
        if op[0].startswith("prior_"):   # the other prior families live in the generic kernels, Normal gives the route back
            if live.cfg.prior[0] in H.FAMILY_PRIORS:
                assert live.plan.kernel == "generic", (name, k, op, live.plan.kernel)
            elif fam.fused:
                assert live.plan.kernel in ("mfma32", "fused16"), (name, k, op, live.plan.kernel)
        check(k, op)


# ------------------------------------------------------------------------------ a refused set_prior changes nothing
@pytest.mark.parametrize("name,n", [("generic-lds-f64", 5), ("mfma32-bf16x3", 33)])
def test_refused_set_prior_leaves_the_prior_it_had(name, n):
    """set_prior with a sigma that has one 0 entry raises, and the plan still answers as a fresh plan with the prior it
    had: ey_plan_set_prior used to copy the new mu into place before it looked at sigma (the kernels that read the prior
    per element then evaluated the new mu against the old 1/sigma^2)."""
    import dataclasses
    fam = H.FAMILY[name]
    cfg = dataclasses.replace(H.start(fam), n=n, prior=("elem", 1))
    live, fresh = H.build(cfg), H.build(cfg)
    assert live.plan.kernel == fam.kernel
    family = live.plan.prior_family
    mu_b, sigma_b, _ = H.prior_arrays(fam, "elem", 2)
    sigma_b[fam.P // 2] = 0.0
    with pytest.raises(ValueError, match="sigma must be positive"):
        live.plan.set_prior(mu_b + 1.0, sigma_b)
    assert live.plan.prior_family == family == fresh.plan.prior_family and live.plan.kernel == fam.kernel
    rng = torch.Generator().manual_seed(3)
    th = (0.2 * torch.randn(3, fam.P, generator=rng, dtype=torch.float64)).to(device=DEV, dtype=live.plan.dtype)
    for temp in (None, torch.tensor([1.0, 0.7, 0.4], dtype=live.plan.dtype, device=DEV)):
        (t, g), (tf, gf) = live.plan.log_target_grad(th, temp=temp), fresh.plan.log_target_grad(th, temp=temp)
        assert H.first_difference([("target", t), ("grad", g)], [("target", tf), ("grad", gf)]) is None
        assert torch.isfinite(t).all()


# ------------------------------------------------------------------------- the index check, through the entry points
@pytest.mark.parametrize("entry", ["mh_tril_step", "hmc_metric_step"])
def test_index_is_checked_again_for_another_tensor_at_the_same_address(entry):
    """Two index tensors over one storage with the same version counter, the contents rewritten to G in between: the
    second call must raise.  The factor table is the first G entries of an allocation of G + 1, so that even a build that
    let the index through would read inside it."""
    G, C = 2, 4
    pl = H.build(H.start(H.FAMILY["mixture"])).plan
    P, dt = pl.P, pl.dtype
    storage = torch.zeros(C, dtype=torch.int32, device=DEV).untyped_storage()

    def alias():
        return torch.empty(0, dtype=torch.int32, device=DEV).set_(storage, 0, (C,))

    th = torch.zeros(C, P, dtype=dt, device=DEV)
    t, g = pl.log_target_grad(th)

    def call(index):
        if entry == "mh_tril_step":
            big = (0.1 * torch.eye(P, dtype=dt, device=DEV)).repeat(G + 1, 1, 1)
            return pl.mh_tril_step(th.clone(), t.clone(), big[:G], index=index, seed=1, it=1)
        big = torch.ones(G + 1, P, dtype=dt, device=DEV)
        return pl.hmc_metric_step(th.clone(), t.clone(), g.clone(), H.STEP, H.LSTEPS, big[:G], "diag", index=index, seed=1,
                                  it=1)

    first = alias()
    call(first)
    alias().fill_(G)
    second = alias()
    assert second.data_ptr() == first.data_ptr() and second._version == first._version and second.tolist() == [G] * C
    with pytest.raises(ValueError, match=r"index must lie in \[0, 2\)"):
        call(second)
