"""Elliptical slice sampling on the device leaves a known target invariant: the recipe of tests/invariance.py and
tests/test_nuts_invariance_gpu.py, unchanged -- 16384 chains from exact draws of the target, 16 iterations in one
``eslice_run`` (in-kernel Philox, one launch), the final states held against 65536 exact draws by Welch's z per feature
under ``invariance.threshold`` for the z-scores this file asserts on; the carried target and ell must be those of the final
state.

Targets: the linear-Gaussian posteriors of dims [3, 1] (f64) and [12, 1] (f32, half the chains at temperature 0.5, each
half against its own law) under the plan's own prior, and the mixtures of P = 2 (f64) and P = 5 (f32) under a Gaussian base
whose scale tests/eslice_cases.py picks on the CPU from the restatement alone (``BASE_FACTOR``), for a mean of 1.5 to 8
evaluations per draw: asserted here.  Under the plan's own prior there is no scale to pick -- the mean evaluations per draw
is a property of the posterior against its N(0, 2^2) prior, 8.8 and 10.4 by the restatement, above that band -- so there the
kernel is held to the restatement's figure (``PRIOR_EVALS`` within ``EVALS_TOL``).  Every draw must move: moved > 0.99."""
import numpy as np
import pytest
import torch

from tests import eslice_cases as ec
from tests import invariance as iv
from tests.test_invariance_gpu import DEV, DT, _np, _plan, _t

pytestmark = pytest.mark.gpu

C, N, N_REF = iv.C_GPU, iv.N_ITERS, iv.N_REF
CASES = ec.INVARIANCE
THRESHOLD = iv.threshold(sum((2 if temp == "halves" else 1) * iv.n_features(iv.target_of(t).P) for t, _, temp, _ in CASES))
SEED0 = 6100


@pytest.mark.parametrize("target,dtype,temp,base", CASES, ids=["/".join(str(v) for v in c[:3]) for c in CASES])
def test_eslice_leaves_its_target_invariant(target, dtype, temp, base):
    seed = SEED0 + CASES.index((target, dtype, temp, base))
    tgt, dt = iv.target_of(target), DT[dtype]
    pl = _plan(target, dtype)
    rng = np.random.default_rng([seed, 1])
    groups = (1.0, 0.5) if temp == "halves" else (1.0,)
    R = C // len(groups)
    th = _t(np.concatenate([iv.exact_draws(tgt, R, rng, t) for t in groups]), dt)
    temps = None if temp is None else _t(np.repeat(groups, R), dt)
    kw = dict(base_loc=None, base_scale=None)
    if base:
        m, s = ec.mix_base(target)
        kw = dict(base_loc=_t(m, dt), base_scale=_t(s, dt))
    ell, tv = pl.eslice_ell(th, temp=temps, **kw)
    count = torch.zeros(C, dtype=torch.int32, device=DEV)
    evals_rec = torch.empty(N, C, dtype=torch.int32, device=DEV)
    pl.eslice_run(th, tv, ell, N, temp=temps, seed=seed, accept_count=count, n_evals_rec=evals_rec, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(th).all() and torch.isfinite(tv).all() and torch.isfinite(ell).all()
    logp = _np(tv) if temps is None else _np(tv) / _np(temps)
    z = np.stack([iv.z_scores(iv.features(_np(th)[k * R:(k + 1) * R], logp[k * R:(k + 1) * R]),
                              iv.reference_moments(tgt, N_REF, rng, t)) for k, t in enumerate(groups)])
    w, where = iv.worst(z, tgt.P)
    moved, evals = float(count.double().mean()) / N, float(evals_rec.double().mean())
    print(f"eslice/{target}/{dtype}/{temp}: largest |z| {w:.2f} ({where}), threshold {THRESHOLD:.2f}, moved {moved:.4f}, "
          f"evaluations per draw mean {evals:.2f} max {int(evals_rec.max())}")
    assert w < THRESHOLD, (w, where)
    assert moved > 0.99, moved
    if base:
        assert ec.EVALS_BAND[0] < evals < ec.EVALS_BAND[1], evals
    else:
        assert abs(evals - ec.PRIOR_EVALS[target]) < ec.EVALS_TOL, evals
    # the carried target and ell are those of the final state (tests.test_invariance_gpu._carried_state_is_fresh's bounds)
    f64 = dtype == "f64"
    lik, prior = pl.log_target(th.clone(), temp=temps)
    e1, t1 = pl.eslice_ell(th.clone(), temp=temps, **kw)
    rtol, atol = (1e-9, 1e-9) if f64 else (2e-4, 2e-3)
    np.testing.assert_allclose(_np(tv), _np(lik + prior), rtol=rtol, atol=atol)
    np.testing.assert_allclose(_np(tv), _np(t1), rtol=rtol, atol=atol)
    np.testing.assert_allclose(_np(ell), _np(e1), rtol=rtol, atol=atol)
