"""A numpy f64 restatement of one Gibbs.draw (eeyore/samplers/gibbs.py:67-102) over a table of index blocks, in both
modes: 'reference' carries a rejected block in the proposal vector for the rest of the draw, as the reference does;
'intended' restores it from the state (a valid Metropolis within Gibbs).  The kernel k_gibbs
(eeyore_amd/csrc/ey_generic.hip) implements exactly this loop."""
import numpy as np

from oracle import mlp_oracle as orc


def gibbs_draw(log_target, theta, target, blocks, scales, z, u, mode="intended"):
    """One draw from (theta [P], target) with normals z [P] (parameter i consumes z[i]) and uniforms u [S].
    ``blocks``: S index lists in visiting order; ``scales``: one scale per block.
    Returns (theta, target, accepted [S] uint8, log_rate [S], margin [S] = |log u - log_rate|)."""
    assert mode in ("intended", "reference")
    cur = np.array(theta, np.float64)
    prop = cur.copy()
    tv_cur = float(target)
    S = len(blocks)
    acc, lr, margin = np.zeros(S, np.uint8), np.zeros(S), np.zeros(S)
    for s, idx in enumerate(blocks):
        idx = np.asarray(idx, int)
        prop[idx] = prop[idx] + scales[s] * np.asarray(z)[idx]
        tv = log_target(prop)
        lr[s] = tv - tv_cur
        with np.errstate(divide="ignore"):
            lu = float(np.log(u[s]))
        margin[s] = abs(lu - lr[s])
        if lu < lr[s]:  # a NaN log-rate rejects
            cur[idx] = prop[idx]
            tv_cur = tv
            acc[s] = 1
        elif mode == "intended":
            prop[idx] = cur[idx]
    return cur, tv_cur, acc, lr, margin


def table_of(rec):
    """(blocks, scales) of a fixture group: blk_off [S+1], blk_idx, blk_scale [S]."""
    off, idx = rec["blk_off"], rec["blk_idx"]
    return [idx[off[s]:off[s + 1]].tolist() for s in range(len(off) - 1)], rec["blk_scale"].tolist()


def spec_of(rec, temperature=None):
    return orc.Spec(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), bias=rec["bias"].tolist(),
                    mu=rec["prior_mu"], sigma=rec["prior_sigma"], temperature=temperature)


def spec_target(rec, temperature=None):
    spec = spec_of(rec, temperature)
    x, y = np.asarray(rec["x"], np.float64), np.asarray(rec["y"], np.float64)
    return lambda th: float(orc.log_target(spec, np.asarray(th, np.float64), x, y))
