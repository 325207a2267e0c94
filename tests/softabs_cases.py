"""The matrices and the yardstick the softabs tests share (tests/test_softabs_host.py, tests/test_am_softabs_gpu.py)."""
import numpy as np

from tests.softabs_restatement import softabs_ref
from tests.test_am_gpu import CASES, F32_DECISION_TOL, LMIX, SCENARIOS, _data, _spd, _target_fn

SIZES = (1, 2, 3, 5, 27, 64, 65)
FACTOR = 8.0  # margin for Jacobi's constant differing from LAPACK's


def matrices(P, seed=0):
    """name -> symmetric [P, P]: SPD, rank 1, zero, 3 I, indefinite with eigenvalues +-logspace(-12, 3), and the
    covariance of three states (rank <= 2)."""
    rng = np.random.default_rng(1000 * P + seed)
    B = rng.standard_normal((P, P)) / np.sqrt(P)
    v = rng.standard_normal(P)
    Q = np.linalg.qr(rng.standard_normal((P, P)))[0]
    lam = np.logspace(-12, 3, P) * np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
    ind = (Q * lam) @ Q.T
    states = 0.1 * rng.standard_normal((3, P))
    return {
        "spd": B @ B.T + 0.5 * np.eye(P),
        "rank1": np.outer(v, v),
        "zero": np.zeros((P, P)),
        "3I": 3.0 * np.eye(P),
        "indefinite": 0.5 * (ind + ind.T),
        "cov3": np.cov(states.T).reshape(P, P),
    }


def yardstick(A, a, seed=0):
    """max(noise, floor): the eigh formula's own rounding noise, max over 8 random permutations Pi of
    |Pi^T ref(Pi A Pi^T) Pi - ref(A)|_F, and the floor P 2^-52 max(|A|_F, 1 / a) (f is Lipschitz-1, the solver backward
    stable).  A result S passes when |S - ref(A)|_F <= FACTOR * yardstick."""
    A = np.asarray(A, np.float64)
    P = A.shape[0]
    ref = softabs_ref(A, a)
    rng = np.random.default_rng(seed)
    noise = 0.0
    for _ in range(8):
        pi = rng.permutation(P)
        back = np.empty(P, int)
        back[pi] = np.arange(P)
        got = softabs_ref(A[np.ix_(pi, pi)], a)[np.ix_(back, back)]
        noise = max(noise, np.linalg.norm(got - ref))
    floor = P * 2.0 ** -52 * max(np.linalg.norm(A), 1.0 / a)
    return max(noise, floor)


# ------------------------------------------------------------------------------------- the one-step scenarios of AM
LIMIT = 160 * 1024


def softabs_lds_bytes(dims, esz):
    """The LDS of one chain in the softabs instantiation of k_am (ey_generic_am_lds): position and state, two packed
    triangles, mean, z, a slot per lane, then the larger of the evaluation's scratch and the f64 work matrix (P columns of
    leading dimension P | 1, P coefficients, a slot per lane)."""
    P = sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1))
    ppad = (P + 3) & ~3
    packed = (P * (P + 1) // 2 + 3) & ~3
    scratch = esz * (sum(dims) * 65 + 2 * max(dims) * 65)
    work = 8 * ((P | 1) * P + ppad + 64)
    return esz * (2 * ppad + 2 * packed + 2 * ppad + 64) + max(scratch, work)


def largest_lr(esz):
    """The widest logistic regression whose softabs instantiation fits (73 inputs in f64, 114 in f32)."""
    return max(d for d in range(1, 128) if softabs_lds_bytes([d, 1], esz) <= LIMIT)


def one_step_model(name, f64):
    """(dims, activations, likelihood, rows): the models of tests/test_am_gpu.py and the largest that fits the dtype."""
    if name == "largest":
        return [largest_lr(8 if f64 else 4), 1], [1], 0, 16
    return CASES[name]


ONE_STEP_MODELS = ("lr5", "mlp433", "lr65", "largest")
# the scenarios of tests/test_am_gpu.py and a rank-deficient cov_sum: two distinct states, the third draw (n = 3 >= t0 = 2)
ONE_STEP = SCENARIOS + [("rank-deficient cov_sum", 2, 0, 2, 1, None, False)]
# (P, chains) -> the seed at which no scenario puts a chain within twice F32_DECISION_TOL of a tie in the restatement on
# f32-rounded inputs (0 where absent); tests/test_softabs_host.py::test_one_step_seeds_leave_no_tie asserts it
SEEDS = {(27, 65): 3, (65, 65): 17, (74, 65): 13, (115, 65): 7}


def one_step_inputs(P, C, si):
    """The inputs of scenario ``si`` for C chains of P parameters as numpy f64 arrays (tests/test_am_gpu.py's recipe)."""
    label, idx, offset, t0, nacc0, mix, force = ONE_STEP[si]
    sc = 0.02 if P > 60 else 0.1
    rng = np.random.default_rng(1000 * si + C + P + 7919 * SEEDS.get((P, C), 0))
    n = idx + 1 - offset
    hist = sc * rng.standard_normal((max(n - 1, 1), C, P))
    below, above = np.nextafter(np.float32(LMIX), np.float32(0)), np.nextafter(np.float32(LMIX), np.float32(1))
    return dict(th=hist[-1].copy(), mean=hist.mean(0) if n > 1 else np.zeros((C, P)),
                cs=np.einsum("kci,kcj->cij", hist, hist) if n > 1 else np.zeros((C, P, P)),
                cov=_spd(C, P, rng, sc * sc), cov0=_spd(C, P, rng, sc * sc), z=rng.standard_normal((C, P)),
                u=np.full(C, 1e-30) if force else rng.random(C),
                um=np.where(np.arange(C) % 2 == 0, above, below).astype(np.float64) if mix else rng.random(C))


def one_step_margins(name, f64, C):
    """min over scenarios and chains of |log u - log_rate| / max(1, |log_rate|) in the restatement (the eigh form as the
    transform) on f32-rounded inputs: what the f32 decision band of the GPU test is compared with."""
    from tests.softabs_restatement import am_draw_softabs
    dims, acts, lik, N = one_step_model(name, f64)
    x, y = _data(dims, lik, N)
    tf = _target_fn(dims, acts, lik, x, y)
    P = sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1))
    b, c = 2.38 / np.sqrt(P), 0.05
    worst = np.inf
    for si, (label, idx, offset, t0, nacc0, mix, force) in enumerate(ONE_STEP):
        h = {k: v.astype(np.float32).astype(np.float64) for k, v in one_step_inputs(P, C, si).items()}
        for ch in range(C):
            want = am_draw_softabs(tf, h["th"][ch], tf(h["th"][ch]), h["mean"][ch], h["cs"][ch], h["cov"][ch], nacc0,
                                   h["cov0"][ch], h["z"][ch], h["um"][ch], h["u"][ch], idx, offset, LMIX, b, c, t0, 1000.0,
                                   transform=lambda m, a: m)  # the decision does not look at the new covariance
            lr = want["log_rate"]
            worst = min(worst, abs(np.log(h["u"][ch]) - lr) / max(1.0, abs(lr)))
    return worst, 2 * F32_DECISION_TOL
