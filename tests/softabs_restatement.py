"""A numpy f64 restatement of the one-wave softabs of eeyore_amd/csrc/ey_generic.hip (softabs_fill, softabs_jacobi,
softabs_emit) in its pair and summation order, ``softabs_ref``, the reference's eigh formula with
f(0) = 1 / a, and ``am_draw_softabs``, tests/am_restatement.am_draw with that transform in place of the ridge."""
import numpy as np

from tests.am_restatement import am_draw, spec_target
from tests.dist_restatement import mix_target_fn, tables

MAX_SWEEPS = 80  # SOFTABS_MAX_SWEEPS
EPS = 2.0 ** -52


def f(x, a):
    """x / tanh(a x), f(0) = 1 / a."""
    x = np.asarray(x, np.float64)
    ax = a * x
    safe = np.where(ax == 0, 1.0, ax)
    return np.where(ax == 0, 1.0 / a, x / np.tanh(safe))


def softabs_ref(A, a=1000.0):
    """Q diag(f(lambda)) Q^T from numpy's eigh of the lower triangle."""
    lam, Q = np.linalg.eigh(np.asarray(A, np.float64), UPLO="L")
    return (Q * f(lam, a)) @ Q.T


def round_pairs(P, r):
    """The column pairs (p < q) of round r of the circle schedule, by lane: lane 0 holds (r, m1), lane k holds
    ((r + k) mod m1, (r - k) mod m1); player m1 = P is the bye of an odd P."""
    half = (P + 1) // 2
    m1 = 2 * half - 1
    out = []
    for k in range(half):
        p, q = (r, m1) if k == 0 else ((r + k) % m1, (r + m1 - k) % m1)
        if p > q:
            p, q = q, p
        if q < P:
            out.append((p, q))
    return out


def _dot(x, y):
    return np.cumsum(x * y)[-1]  # i ascending, one product added at a time (cumsum does not sum pairwise)


def softabs_jacobi(A, a=1000.0):
    """(S, sweeps): the kernel's result from the lower triangle of A, and the sweeps it took (0 for P = 1; -1 and the
    mirrored lower triangle for a matrix with an entry that is not finite)."""
    A = np.asarray(A, np.float64)
    P = A.shape[0]
    G = np.tril(A) + np.tril(A, -1).T
    if not np.isfinite(G).all():
        return G, -1
    m1 = 2 * ((P + 1) // 2) - 1
    sweeps, more, tol = 0, P > 1, (P + 6) * 2.0 ** -53
    with np.errstate(all="ignore"):
        while more and sweeps < MAX_SWEEPS:
            sweeps += 1
            more = False
            for r in range(m1):
                for p, q in round_pairs(P, r):  # disjoint columns: the lanes of a round do not see each other
                    x, y = G[:, p].copy(), G[:, q].copy()
                    al, be, ga = _dot(x, x), _dot(y, y), _dot(x, y)
                    if not abs(ga) > tol * (np.sqrt(al) * np.sqrt(be)):
                        continue
                    more = True
                    zeta = (be - al) / (2.0 * ga)
                    t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    G[:, p] = c * x - s * y
                    G[:, q] = s * x + c * y
        sig = np.array([np.sqrt(_dot(G[:, k], G[:, k])) for k in range(P)])
        tau = (P * EPS) * sig.max()
        ia = 1.0 / a
        keep = sig > tau
        sg = np.where(keep, sig, 1.0)
        coef = np.where(keep, ((sg / np.tanh(a * sg) - ia) / sg) / sg, 0.0)
        S = np.zeros((P, P))
        for k in range(P):  # k ascending, then the diagonal's 1 / a
            S = S + (coef[k] * G[:, k])[:, None] * G[:, k][None, :]
        S = S + ia * np.eye(P)
    S = np.tril(S)
    return S + np.tril(S, -1).T, sweeps


def am_draw_softabs(log_target, theta, target, mean, cov_sum, cov, num_accepted, cov0, z, u_mix, u, idx, offset, l, b, c,
                    t0, a, transform=None):
    """One AM.draw with the transform softabs(cov, a): am_draw with eps = 0, then what it recomputed (n >= t0, something
    accepted) passes through ``transform`` (default: the kernel's Jacobi)."""
    out = am_draw(log_target, theta, target, mean, cov_sum, cov, num_accepted, cov0, z, u_mix, u, idx, offset, l, b, c, t0,
                  0.0)
    out["raw_cov"] = out["cov"]
    out["transformed"] = bool(idx + 1 - offset >= t0 and out["num_accepted"] > 0)
    if out["transformed"]:
        out["cov"] = softabs_jacobi(out["cov"], a)[0] if transform is None else transform(out["cov"], a)
    return out


def fixture_target(rec):
    """The log-target of a g22 group: the mixture of group a, a network otherwise."""
    if "weights" in rec:
        return mix_target_fn(*tables(rec["weights"], rec["means"], rec["covs"], bool(rec["normalized"])))
    return spec_target(rec)


def unpacked(tri, P):
    """The symmetric [P, P] matrix of a lower triangle stored in np.tril_indices order."""
    out = np.zeros((P, P))
    out[np.tril_indices(P)] = tri
    return out + np.tril(out, -1).T


def recorded_state(rec, it):
    """The state after draw ``it`` (before the first: it = -1) as the fixture recorded it."""
    P = rec["theta0"].shape[0]
    if it < 0:
        return dict(theta=rec["theta0"].copy(), target=float(rec["init_target"]), mean=np.zeros(P),
                    cov_sum=np.zeros((P, P)), cov=rec["cov0"].copy(), num_accepted=0)
    return dict(theta=rec["sample"][it].copy(), target=float(rec["target_val"][it]), mean=rec["running_mean"][it].copy(),
                cov_sum=unpacked(rec["cov_sum"][it], P), cov=unpacked(rec["cov"][it], P),
                num_accepted=int(rec["num_accepted"][it]))


def replay(rec, transform=None):
    """(it, the restatement's draw from the recorded state before it, the recorded state after it) for every draw."""
    tf = fixture_target(rec)
    par = dict(l=float(rec["l"]), b=float(rec["b"]), c=float(rec["c"]), t0=int(rec["t0"]), a=float(rec["a"]))
    for it in range(rec["z"].shape[0]):
        st = recorded_state(rec, it - 1)
        got = am_draw_softabs(tf, st["theta"], st["target"], st["mean"], st["cov_sum"], st["cov"], st["num_accepted"],
                              rec["cov0"], rec["z"][it], rec["u_mix"][it], rec["u"][it], int(rec["idx"][it]),
                              int(rec["offset"]), transform=transform, **par)
        yield it, got, recorded_state(rec, it)
