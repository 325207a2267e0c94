"""Multinomial NUTS under a fixed metric, restated in numpy f64.  TEST INFRASTRUCTURE ONLY.

``nuts_draw`` is the transition of include/eeyore_amd_nuts.h for ONE chain, with the tree built RECURSIVELY: a subtree of
depth j is two subtrees of depth j - 1, its rho the sum of theirs, and it is valid iff both are and the U-turn criterion
holds between its first and last leaf.  That is the obviously-right form of the sub-block checks which the kernel makes
iteratively from checkpoints; ``nuts_draw_iterative`` transcribes the kernel's loop (an even leaf stores slot
popcount(k >> 1), an odd leaf checks one slot per trailing 1-bit) and must agree with the recursion.

Everything else is sequential in both: the whitened velocity v = L^T p (``mul`` x = L x, ``tmul`` x = L^T x), one leapfrog
step per leaf with half kicks at both ends, the leaf weights exp(H0 - H), reservoir sampling of the subtree's candidate
(u_leaf(n) < exp(delta - W')), the biased progressive move at the top (u_top(d) < exp(W' - W)), the energy error bound 1000.
The uniforms are one table ``u`` in the word layout of the header: 1 + 2d direction, 2 + 2d u_top, 21 + n u_leaf.

A draw reports, beside its outcome, the smallest MARGIN over every decision it took -- |v . rho| relative to |v| |rho|,
|u - p|, |-delta - 1000| / 1000 -- so that a comparison can set aside the draws a rounding error may legitimately flip.

Mutants (the host test shows that the invariance harness catches them): 'leaf_unweighted' draws the subtree's candidate
uniformly over its leaves, ignoring the weights; 'top_always' makes the top-level move with probability 1."""
import numpy as np

MAX_DEPTH = 10                      # EY_NUTS_MAX_DEPTH
LEAF_WORD = 1 + 2 * MAX_DEPTH       # u_leaf(n) is word LEAF_WORD + n
DELTA_MAX = 1000.0


def words(max_depth):
    """The number of uniform words a draw of that depth cap can read."""
    return LEAF_WORD + 2 ** max_depth


def metric_ops(kind, table):
    """(mul, tmul) for a diagonal metric (scales [P]) or a dense one (a factor [P, P], its lower triangle)."""
    if kind == "diag":
        s = np.asarray(table, np.float64)
        return (lambda x: s * x), (lambda x: s * x)
    F = np.tril(np.asarray(table, np.float64))
    return (lambda x: F @ x), (lambda x: F.T @ x)


def point_value_grad(tgt, temp=None):
    """value_grad of a tests.invariance.Target at ONE point [P] (the batched method on a batch of one)."""
    def f(th):
        val, g = tgt.value_grad(th[None], None if temp is None else np.asarray([temp], np.float64))
        return float(val[0]), g[0]
    return f


class _Draw:
    """What both forms share: the integrator's state, the counters, the reservoir of the subtree, the margins."""

    def __init__(self, value_grad, theta, t, g, v0, u, eps, mul, tmul, mutant):
        self.f, self.u, self.eps, self.mul, self.tmul, self.mutant = value_grad, np.asarray(u, np.float64), eps, mul, tmul, mutant
        self.H0 = -t + 0.5 * float(v0 @ v0)
        self.n, self.acc_sum, self.margin, self.divergent = 0, 0.0, np.inf, False
        self.dir_words = 0

    def note(self, m):
        if m < self.margin:
            self.margin = float(m)

    def uniform_below(self, word, p):
        """u[word] < p, with its margin (a NaN p decides 'no' with margin 0)."""
        uu = self.u[word]
        self.note(abs(uu - p) if p == p else 0.0)
        return bool(uu < p)

    def criterion(self, va, vb, rho):
        a, b = float(va @ rho), float(vb @ rho)
        nr = np.sqrt(float(rho @ rho))
        for x, w in ((a, va), (b, vb)):
            den = np.sqrt(float(w @ w)) * nr
            self.note(abs(x) / den if den > 0 else 0.0)
        return a > 0 and b > 0

    def start_subtree(self, state, fwd):
        self.th, self.v, self.g = (x.copy() for x in state)
        self.e = self.eps if fwd else -self.eps
        self.Wp, self.k, self.cand = -np.inf, 0, None

    def leaf(self):
        """One leapfrog step and the leaf's bookkeeping.  Returns the leaf's v, or None where the draw diverges."""
        e = self.e
        self.v = self.v + (0.5 * e) * self.tmul(self.g)
        self.th = self.th + e * self.mul(self.v)
        t, self.g = self.f(self.th)
        self.v = self.v + (0.5 * e) * self.tmul(self.g)
        H = -t + 0.5 * float(self.v @ self.v)
        delta = self.H0 - H
        if not delta == delta:
            delta = -np.inf
        self.note(abs(-delta - DELTA_MAX) / DELTA_MAX)
        if -delta > DELTA_MAX:
            self.divergent = True
            return None
        with np.errstate(over="ignore", invalid="ignore"):
            self.Wp = float(np.logaddexp(self.Wp, delta))
            if self.mutant == "leaf_unweighted":
                take = bool(self.u[LEAF_WORD + self.n] < 1.0 / (self.k + 1))
            else:
                take = self.uniform_below(LEAF_WORD + self.n, float(np.exp(delta - self.Wp)))
            if take:
                self.cand = (self.th.copy(), t, self.g.copy(), H)
            self.acc_sum += min(1.0, float(np.exp(delta)))
        self.n += 1
        self.k += 1
        return self.v.copy()

    def state(self):
        return self.th.copy(), self.v.copy(), self.g.copy()


def _recursive_subtree(dr, j):
    """(valid, v_first, v_last, rho) of the next 2^j leaves."""
    if j == 0:
        v = dr.leaf()
        return (False, None, None, None) if v is None else (True, v, v, v.copy())
    ok, a_first, _, a_rho = _recursive_subtree(dr, j - 1)
    if not ok:
        return False, None, None, None
    ok, _, b_last, b_rho = _recursive_subtree(dr, j - 1)
    if not ok:
        return False, None, None, None
    rho = a_rho + b_rho
    return dr.criterion(a_first, b_last, rho), a_first, b_last, rho


def _iterative_subtree(dr, d):
    """The kernel's loop over the 2^d leaves with its checkpoints: (valid, rho')."""
    P = len(dr.th)
    ckv, ckr = np.zeros((MAX_DEPTH, P)), np.zeros((MAX_DEPTH, P))
    rhop = np.zeros(P)
    for k in range(2 ** d):
        v = dr.leaf()
        if v is None:
            return False, None
        rhop = rhop + v
        slot = bin(k >> 1).count("1")
        if k % 2 == 0:
            ckv[slot], ckr[slot] = v, rhop
            continue
        kk = k
        while kk & 1:
            if not dr.criterion(ckv[slot], v, rhop - ckr[slot] + ckv[slot]):
                return False, None
            kk, slot = kk >> 1, slot - 1
    return True, rhop


def _draw(value_grad, theta, t, g, v0, u, eps, max_depth, mul, tmul, mutant, iterative):
    if not 1 <= max_depth <= MAX_DEPTH:
        raise ValueError("max_depth must lie in [1, 10]")
    theta, g, v0 = (np.asarray(x, np.float64) for x in (theta, g, v0))
    dr = _Draw(value_grad, theta, float(t), g, v0, u, float(eps), mul, tmul, mutant)
    left = right = (theta, v0, g)
    prop, moved = (theta, float(t), g, dr.H0), False
    W, rho, d, stop = 0.0, v0.copy(), 0, "max_depth"
    while d < max_depth:
        dr.dir_words += 1
        fwd = not dr.uniform_below(1 + 2 * d, 0.5)
        dr.start_subtree(right if fwd else left, fwd)
        if iterative:
            ok, rhop = _iterative_subtree(dr, d)
        else:
            ok, _, _, rhop = _recursive_subtree(dr, d)
        if not ok:
            stop = "divergent" if dr.divergent else "subblock"
            break
        with np.errstate(over="ignore", invalid="ignore"):
            if mutant == "top_always" or dr.uniform_below(2 + 2 * d, float(np.exp(dr.Wp - W))):
                prop, moved = dr.cand, True
            W = float(np.logaddexp(W, dr.Wp))
        rho = rho + rhop
        if fwd:
            right = dr.state()
        else:
            left = dr.state()
        d += 1
        if not dr.criterion(left[1], right[1], rho):
            stop = "tree"
            break
    return dict(theta=prop[0].copy(), target=prop[1], grad=prop[2].copy(), energy=prop[3], accepted=int(moved), depth=d,
                n_leapfrog=dr.n, divergent=int(dr.divergent), accept_stat=dr.acc_sum / dr.n if dr.n else 0.0,
                margin=dr.margin, stop=stop, dir_words=dr.dir_words)


def nuts_draw(value_grad, theta, t, g, v0, u, eps, max_depth, mul, tmul, mutant=None):
    """One draw from the state (theta [P], t, g [P]) with velocity v0 [P] and the uniform table u [>= words(max_depth)]:
    dict(theta, target, grad, energy, accepted, depth, n_leapfrog, divergent, accept_stat, margin, stop, dir_words) --
    ``stop`` is 'max_depth', 'divergent', 'subblock' (a check inside the new subtree, its own included) or 'tree'."""
    return _draw(value_grad, theta, t, g, v0, u, eps, max_depth, mul, tmul, mutant, iterative=False)


def nuts_draw_iterative(value_grad, theta, t, g, v0, u, eps, max_depth, mul, tmul, mutant=None):
    """``nuts_draw`` with the kernel's checkpoint loop in place of the recursion."""
    return _draw(value_grad, theta, t, g, v0, u, eps, max_depth, mul, tmul, mutant, iterative=True)


OUTCOME = ("depth", "n_leapfrog", "divergent", "accepted")
VALUES = ("theta", "target", "grad", "accept_stat", "energy")


def run_chains(value_grad, theta, t, g, v0, u, eps, max_depth, metric, mutant=None, draw=nuts_draw):
    """One draw of C chains: theta, g, v0 [C, P], t [C], u [C, S], eps a number or [C], ``metric`` (kind, table) with the
    table for all chains ([P] / [P, P]) or per chain.  Returns a dict of arrays with a leading chain axis."""
    C = len(theta)
    kind, table = metric
    table = np.asarray(table, np.float64)
    shared = table.ndim == (1 if kind == "diag" else 2)
    eps = np.broadcast_to(np.asarray(eps, np.float64), (C,))
    outs = []
    for c in range(C):
        mul, tmul = metric_ops(kind, table if shared else table[c])
        f = value_grad[c] if isinstance(value_grad, (list, tuple)) else value_grad
        outs.append(draw(f, theta[c], t[c], g[c], v0[c], u[c], eps[c], max_depth, mul, tmul, mutant))
    return {k: np.array([o[k] for o in outs]) for k in outs[0]}
