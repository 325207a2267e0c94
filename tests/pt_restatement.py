"""The between-chain move of PowerPosteriorSampler that k_pt_between (eeyore_amd/csrc/ey_pt.hip)
implements, restated in numpy: the ladder tables as ey_pt_ladder_create builds them, the Philox variates of the move
(through oracle/philox_oracle.py), the partner draw by inverse CDF, and the K sequential steps of one move for all
replicas.  Also a test double that gives tests/oracle_plan.VectorTempOraclePlan the ``pt_ladder`` / ``pt_between`` pair of
``eeyore_amd.plan.Plan``, so that ``PowerPosteriorSampler(between='device')`` runs on the CPU.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from oracle import philox_oracle as po
from tests.oracle_plan import VectorTempOraclePlan

STREAM_PT = 2
PT_WAVES, PT_KMAX = 4, 1024  # k_pt_between: replicas per workgroup, temperatures it serves


class Ladder:
    """t [K] and log_q [K, K] in ``dtype``, cdf [K, K] in double: row i holds the running sums of q[i, j] / sum_j q[i, j]
    over j != i in index order (the diagonal adds nothing), log_q the logs of the same quotients (diagonal 0)."""

    def __init__(self, t, q, dtype):
        t, q = np.asarray(t, np.float64), np.asarray(q, np.float64)
        self.K = K = len(t)
        self.dtype = np.dtype(dtype).type
        w = q.copy()
        np.fill_diagonal(w, 0.0)
        total = np.cumsum(w, axis=1)[:, -1]          # (cumsum adds in index order, as the library's loop does)
        p = w / total[:, None]
        cdf = np.cumsum(p, axis=1)
        with np.errstate(divide="ignore"):
            logq = np.log(p)
        np.fill_diagonal(logq, 0.0)
        self.t, self.logq, self.cdf = t.astype(dtype), logq.astype(dtype), cdf


def variates(K, R, seed, it, replica_offset=0, dtype=np.float64):
    """(v [K, R] double, u [K, R] dtype): Philox block i of the stream keyed (seed, replica_offset + r, it, STREAM_PT)
    gives step i of replica r its partner variate (words 0, 1: 53 bits) and its accept variate (words 2, 3, converted as
    the accept stream converts words 0, 1)."""
    chain = (np.arange(R, dtype=np.uint64) + np.uint64(replica_offset))[None, :]
    k0, k1, c1, c2, c3 = po._key_counter(seed, chain, it, STREAM_PT)
    o0, o1, o2, o3 = po.philox4x32_10(np.arange(K, dtype=np.uint32)[:, None], c1, c2, c3, k0, k1)

    def u53(hi, lo):
        return ((hi.astype(np.uint64) << np.uint64(21)) | (lo >> np.uint32(11)).astype(np.uint64)).astype(np.float64) * 2.0 ** -53

    v = u53(o0, o1)
    if np.dtype(dtype) == np.float32:
        return v, (o2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return v, u53(o2, o3)


def draw_partners(cdf_row, v, i):
    """The first index whose cumulative probability exceeds v; v beyond the rounded total goes to the last index != i."""
    K = len(cdf_row)
    j = np.searchsorted(cdf_row, v, side="right")
    return np.where(j < K, j, K - 2 if i == K - 1 else K - 1).astype(np.int32)


def between(ladder, theta, target, grad=None, partners=None, u=None, seed=0, it=0, replica_offset=0):
    """One between-chain move of every replica on COPIES of theta [K*R, P], target [K*R], grad [K*R, P] or None (row
    k * R + r = temperature k of replica r), all arithmetic in the ladder's dtype: for i = 0 .. K-1 in order, partner j,
    ell = target / t, log_rate = (log_q[j,i] - log_q[i,j]) + (t_i - t_j)(ell_j - ell_i), swap iff log(u) < log_rate; on a
    swap the theta rows trade places, target_i <- target_j (t_i / t_j), target_j <- target_i (t_j / t_i), the grad rows
    with the same factors.  A given partner out of [0, K) or equal to i exchanges nothing (log_rate NaN).
    Returns dict(theta, target, grad, partners, u, swap, log_rate, log_u); the last five [K, R]."""
    K, T = ladder.K, ladder.dtype
    t, logq = ladder.t, ladder.logq
    R = theta.shape[0] // K
    th = np.array(theta, dtype=T).reshape(K, R, -1)
    tg = np.array(target, dtype=T).reshape(K, R)
    g = None if grad is None else np.array(grad, dtype=T).reshape(K, R, -1)
    ar = np.arange(R)
    if partners is None:
        v, u = variates(K, R, seed, it, replica_offset, T)
        partners = np.stack([draw_partners(ladder.cdf[i], v[i], i) for i in range(K)])
    partners, u = np.asarray(partners, np.int32), np.asarray(u, T)
    swaps, rates = np.zeros((K, R), np.uint8), np.full((K, R), np.nan, T)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        log_u = np.log(u)
        for i in range(K):
            j = partners[i]
            valid = (j >= 0) & (j < K) & (j != i)
            jv = np.where(valid, j, i)
            ti, tj = t[i], t[jv]
            tgi, tgj = tg[i].copy(), tg[jv, ar]
            lr = (ti - tj) * (tgj / tj - tgi / ti)
            lr = lr + (logq[jv, i] - logq[i, jv])
            m = valid & (log_u[i] < lr)
            swaps[i], rates[i] = m, np.where(valid, lr, np.nan)
            fi, fj = (ti / tj)[m], (tj / ti)[m]
            rj, rr = jv[m], ar[m]
            a, b = th[i, rr].copy(), th[rj, rr].copy()
            th[i, rr], th[rj, rr] = b, a
            tg[i, rr], tg[rj, rr] = tgj[m] * fi, tgi[m] * fj
            if g is not None:
                a, b = g[i, rr].copy(), g[rj, rr].copy()
                g[i, rr], g[rj, rr] = b * fi[:, None], a * fj[:, None]
    return dict(theta=th.reshape(theta.shape), target=tg.reshape(-1), grad=None if g is None else g.reshape(grad.shape),
                partners=partners, u=u, swap=swaps, log_rate=rates, log_u=log_u)


def decided(out, margin=1e-3):
    """[K, R]: the steps whose decision has the margin |log u - log_rate| > margin * max(1, |log_rate|) (an invalid step,
    which exchanges nothing whatever the arithmetic, counts as decided)."""
    lr = out["log_rate"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.isnan(lr) | (np.abs(out["log_u"].astype(np.float64) - lr) > margin * np.maximum(1.0, np.abs(lr)))


class PtOraclePlan(VectorTempOraclePlan):
    """VectorTempOraclePlan with ``Plan.pt_ladder`` / ``Plan.pt_between`` on the restatement above."""

    def pt_ladder(self, t, q):
        return Ladder(t, q, self.np_dtype)

    def pt_between(self, ladder, theta, target, grad=None, partners=None, u=None, seed=0, it=0, replica_offset=0,
                   rec_theta=None, rec_target=None, outputs=True):
        out = between(ladder, theta.numpy(), target.numpy(), None if grad is None else grad.numpy(),
                      None if partners is None else partners.numpy(), None if u is None else u.numpy(), seed=seed, it=it,
                      replica_offset=replica_offset)
        moved = torch.as_tensor(out["swap"]).bool()
        theta.copy_(torch.as_tensor(out["theta"]))
        target.copy_(torch.as_tensor(out["target"]))
        if grad is not None:
            grad.copy_(torch.as_tensor(out["grad"]))
        if rec_theta is not None:
            rec_theta.copy_(theta)
        if rec_target is not None:
            rec_target.copy_(target)
        self.pt_calls = getattr(self, "pt_calls", []) + [dict(seed=seed, it=it, replica_offset=replica_offset, moved=moved)]
        if not outputs:
            return {}
        return dict(partners=torch.as_tensor(out["partners"]), u=torch.as_tensor(out["u"]),
                    swap=torch.as_tensor(out["swap"]), log_rate=torch.as_tensor(out["log_rate"]))


def attach_pt(model):
    """Give ``model`` (device='cpu') the oracle test double with the between-chain move."""
    object.__setattr__(model, "_hip_plan", PtOraclePlan.for_model(model))
    return model
