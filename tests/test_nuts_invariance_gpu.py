"""NUTS on the device leaves a known target invariant: the recipe of tests/invariance.py and tests/test_invariance_gpu.py,
unchanged -- 16384 chains from exact draws of the target, 16 iterations through ``nuts_run`` (in-kernel Philox, one launch,
max_depth 5), the final states held against 65536 exact draws by Welch's z per feature under ``invariance.threshold`` for
the z-scores this file asserts on; the carried target and gradient must be those of the final state.

Targets: the P = 2 mixture and the linear-Gaussian posterior of dims [3, 1]; f32 and f64; a diagonal and a dense metric
whose tables come from a generator of their own.  The steps were chosen on the CPU from tests/nuts_restatement.py alone
(300 chains, one draw) for a mean accept statistic of 0.8 to 0.96 with trees of several depths."""
import numpy as np
import pytest
import torch

from tests import invariance as iv
from tests.test_invariance_gpu import DEV, DT, _np, _plan, _t

pytestmark = pytest.mark.gpu

C, N, N_REF, MAX_DEPTH = iv.C_GPU, iv.N_ITERS, iv.N_REF, 5
STEPS = {("mix2_2", "diag"): 1.4, ("mix2_2", "dense"): 0.7, ("lin3", "diag"): 0.08, ("lin3", "dense"): 0.06}
CASES = [(t, k, d) for (t, k) in STEPS for d in ("f64", "f32")]
THRESHOLD = iv.threshold(sum(iv.n_features(iv.target_of(t).P) for t, _, _ in CASES))
SEED0 = 5200


def table(target, kind):
    P = iv.target_of(target).P
    rng = np.random.default_rng([P, kind == "dense", 41])
    return iv.factors(1, P, rng, 1.0)[0] if kind == "dense" else 0.5 + rng.random(P)


@pytest.mark.parametrize("target,kind,dtype", CASES, ids=["/".join(c) for c in CASES])
def test_nuts_leaves_its_target_invariant(target, kind, dtype):
    seed = SEED0 + CASES.index((target, kind, dtype))
    tgt, dt = iv.target_of(target), DT[dtype]
    pl = _plan(target, dtype)
    rng = np.random.default_rng([seed, 1])
    th = _t(iv.exact_draws(tgt, C, rng), dt)
    tv, gr = pl.log_target_grad(th)
    tv, gr = tv.contiguous(), gr.contiguous()
    count = torch.zeros(C, dtype=torch.int32, device=DEV)
    depth_rec = torch.empty(N, C, dtype=torch.int32, device=DEV)
    div_rec = torch.empty(N, C, dtype=torch.uint8, device=DEV)
    out = pl.nuts_run(th, tv, gr, STEPS[(target, kind)], MAX_DEPTH, _t(table(target, kind), dt), kind, N, seed=seed,
                      accept_count=count, depth_rec=depth_rec, divergent_rec=div_rec)
    torch.cuda.synchronize()
    assert torch.isfinite(th).all() and torch.isfinite(tv).all()
    z = iv.z_scores(iv.features(_np(th), _np(tv)), iv.reference_moments(tgt, N_REF, rng))
    w, where = iv.worst(z[None], tgt.P)
    depths = np.bincount(depth_rec.cpu().numpy().ravel(), minlength=MAX_DEPTH + 1)
    moved, stat = float(count.double().mean()) / N, float(out["accept_stat"].double().mean())
    print(f"nuts/{target}/{kind}/{dtype}: largest |z| {w:.2f} ({where}), threshold {THRESHOLD:.2f}, moved {moved:.3f}, "
          f"accept_stat of the last draw {stat:.3f}, depths {depths.tolist()}, divergent {int(div_rec.sum())}")
    assert w < THRESHOLD, (w, where)
    assert moved > 0.5 and 0.5 < stat < 0.995 and (depths[1:4] > 0).all() and int(div_rec.sum()) == 0
    f64 = dtype == "f64"
    t1, g1 = pl.log_target_grad(th.clone())
    rtol = 1e-9 if f64 else 2e-4
    np.testing.assert_allclose(_np(tv), _np(t1), rtol=rtol, atol=1e-9 if f64 else 2e-3)
    want = _np(g1)
    np.testing.assert_allclose(_np(gr), want, rtol=rtol, atol=rtol * np.abs(want).max())
