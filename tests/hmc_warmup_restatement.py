"""A numpy f64 restatement of the windowed warm-up of HMC under a metric (ey_hmc_metric_warmup, ey_metric_from_moments,
tuners.WindowedAdaptation), independent of the product code: Welford's running moments, the metric they
give, Stan's window schedule, the dual-averaging recurrence, and a whole warm-up built from
tests/hmc_metric_restatement.hmc_metric_draw."""
import numpy as np

from tests.hmc_metric_restatement import DIAG, TRIL, hmc_metric_draw

REG, REG_N = 1e-3, 5.0          # Stan's shrinkage towards 1e-3 I with the weight of five draws
GAMMA, T0, KAPPA = 0.05, 10, 0.75  # dual averaging (Hoffman & Gelman 2014)


def welford(x_seq, form, mean=None, M2=None, count=0):
    """Running moments of the draws x_seq [n, P] of ONE chain, in the order given: with n the count including the draw and
    d = x - mean_old, mean += d / n and M2 += ((n - 1) / n) d d^T (DIAG: its diagonal).  ``mean``, ``M2``, ``count``
    continue earlier accumulators.  Returns (mean [P], M2 [P] or [P, P])."""
    x_seq = np.asarray(x_seq, np.float64)
    P = x_seq.shape[1]
    mean = np.zeros(P) if mean is None else np.array(mean, np.float64)
    M2 = (np.zeros(P) if form == DIAG else np.zeros((P, P))) if M2 is None else np.array(M2, np.float64)
    for k, x in enumerate(x_seq):
        n = float(count + k + 1)
        d = x - mean
        mean = mean + d / n
        M2 = M2 + ((n - 1.0) / n) * (d * d if form == DIAG else np.outer(d, d))
    return mean, M2


def welford_chains(draws, form):
    """``welford`` of every chain of draws [n, C, P]: (mean [C, P], M2 [C, P] or [C, P, P])."""
    draws = np.asarray(draws, np.float64)
    res = [welford(draws[:, c], form) for c in range(draws.shape[1])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _lower(M):
    """The symmetric matrix whose lower triangle M holds (the strict upper triangle of M is never read)."""
    low = np.tril(M)
    return low + np.tril(low, -1).T


def _estimate(total, N, form):
    if form == DIAG:
        return np.sqrt(N / (N + REG_N) * (total / (N - 1.0)) + REG * REG_N / (N + REG_N))
    P = total.shape[0]
    return np.linalg.cholesky(N / (N + REG_N) * (total / (N - 1.0)) + REG * REG_N / (N + REG_N) * np.eye(P))


def metric_from_moments(mean, M2, n, form, pooled):
    """The metric table of per-chain moments after n draws each: pooled, ONE estimate from the N = C n draws of all chains
    (total = sum_c M2_c + n sum_c (mean_c - gm)(mean_c - gm)^T with gm the mean of the chains' means); otherwise one per
    chain, N = n.  S = total / (N - 1) shrunk to N/(N+5) S + 1e-3 5/(N+5) I; DIAG: the square roots, TRIL: the Cholesky
    factor.  Returns [P] / [P, P], or [C, P] / [C, P, P]."""
    mean, M2 = np.asarray(mean, np.float64), np.asarray(M2, np.float64)
    C = mean.shape[0]
    if form == TRIL:
        M2 = np.stack([_lower(M2[c]) for c in range(C)])
    if not pooled:
        return np.stack([_estimate(M2[c], float(n), form) for c in range(C)])
    dm = mean - mean.sum(0) / C
    between = (dm * dm).sum(0) if form == DIAG else dm.T @ dm
    return _estimate(M2.sum(0) + n * between, float(C * n), form)


def windows(n, init_buffer=75, term_buffer=50, base_window=25):
    """Stan's metric windows [(start, end)] of a warm-up of n draws."""
    if n < 20:
        return []
    if init_buffer + base_window + term_buffer > n:
        init_buffer, term_buffer = int(0.15 * n), int(0.1 * n)
        base_window = n - init_buffer - term_buffer
    out, start, size = [], init_buffer, base_window
    while start < n - term_buffer:
        end = start + size
        if end + 2 * size > n - term_buffer:
            end = n - term_buffer
        out.append((start, end))
        start, size = end, 2 * size
    return out


def da_restart(step):
    """(barh, logbare, mu) from which dual averaging starts over at ``step``."""
    return np.array([0.0, 0.0, np.log(10.0 * step)])


def da_update(state, t, rate, d, logeub=None, averaged=False):
    """One update of the recurrence after the t-th adapting draw (t >= 1) with acceptance ``rate`` (NaN counts as 0):
    returns (state, the step of the next draw) -- the averaged step exp(logbare) when ``averaged``."""
    barh, logbare, mu = state
    rate = 0.0 if rate != rate else rate
    barh = barh + (1.0 / (t + T0)) * ((d - rate) - barh)
    loge = mu - (np.sqrt(t) / GAMMA) * barh
    if logeub is not None:
        loge = min(loge, logeub)
    logbare = logbare + t ** (-KAPPA) * (loge - logbare)
    return np.array([barh, logbare, mu]), float(np.exp(logbare if averaged else loge))


def start_step(value_grad, th, form, metric, v):
    """Hoffman & Gelman's heuristic for one chain: from step 1, double or halve until the acceptance ratio of one
    leapfrog step with velocity v crosses 1/2."""
    t0, g0 = value_grad(th)

    def ratio(step):
        o = hmc_metric_draw(value_grad, th, t0, g0, form, metric, v, 0.5, step, 1)
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.exp(o[4] - o[5])
        return 0.0 if r != r else float(r)

    step = 1.0
    r = ratio(step)
    a = 1.0 if r > 0.5 else -1.0
    for _ in range(60):
        if not (r > 0.5 if a > 0 else r < 0.5):  # r^a > 2^-a
            break
        step *= 2.0 ** a
        r = ratio(step)
    return step


def warm_up(value_grad, theta0, form, n, num_steps, d=0.8, seed=0, pooled=True):
    """A whole warm-up of the chains theta0 [C, P] from the identity metric of ``form``: the step of every chain by dual
    averaging (restarted at every window end from ``start_step``), the metric from the Welford moments of each window,
    pooled over the chains.  The random numbers are numpy's (``seed``).  Returns (theta [C, P], steps [C], metric, the
    mean acceptance rate of each draw [n])."""
    rng = np.random.default_rng(seed)
    th = np.array(theta0, np.float64)
    C, P = th.shape
    metric = np.ones(P) if form == DIAG else np.eye(P)
    tv, gr = zip(*[value_grad(th[c]) for c in range(C)])
    tv, gr = list(tv), list(gr)
    ends = {e: s for s, e in windows(n)}
    starts = {s for s, e in windows(n)}

    def restart():
        steps = [start_step(value_grad, th[c], form, metric, rng.standard_normal(P)) for c in range(C)]
        return steps, [da_restart(s) for s in steps], 1

    steps, states, t = restart()
    collecting, rates, seq = False, np.zeros(n), []
    for k in range(n):
        if k in starts:
            collecting, seq = True, []
        for c in range(C):
            o = hmc_metric_draw(value_grad, th[c], tv[c], gr[c], form, metric, rng.standard_normal(P), rng.random(),
                                steps[c], num_steps)
            th[c], tv[c], gr[c] = o[0], o[1], o[2]
            rates[k] += (0.0 if o[6] != o[6] else o[6]) / C
            states[c], steps[c] = da_update(states[c], t, o[6], d, averaged=k == n - 1)
        t += 1
        if collecting:
            seq.append(th.copy())
        if k + 1 in ends:
            mean, M2 = welford_chains(np.stack(seq), form)
            metric = metric_from_moments(mean, M2, len(seq), form, pooled)
            if not pooled:
                raise NotImplementedError("the restated warm-up pools the chains")
            collecting = False
            if k + 1 < n:
                steps, states, t = restart()
    return th, np.array(steps), metric, rates


def whitened_condition(Sigma, form, metric):
    """cond(L^-1 Sigma L^-T) for the metric's factor L."""
    L = np.diag(metric) if form == DIAG else np.tril(metric)
    Li = np.linalg.inv(L)
    return float(np.linalg.cond(Li @ Sigma @ Li.T))


def gaussian_case(form, P=8, cond=1e3, seed=0):
    """N(0, Sigma) with the spectrum 1e-2 .. 1e-2 cond: axis-aligned for DIAG, rotated for TRIL.  Returns (Sigma, the
    value-and-gradient function of its log-density up to a constant)."""
    rng = np.random.default_rng(1000 + seed)
    ev = 1e-2 * np.logspace(0, np.log10(cond), P)
    if form == DIAG:
        Sigma = np.diag(rng.permutation(ev))
    else:
        q, _ = np.linalg.qr(rng.standard_normal((P, P)))
        Sigma = (q * ev) @ q.T
        Sigma = (Sigma + Sigma.T) / 2
    prec = np.linalg.inv(Sigma)
    prec = (prec + prec.T) / 2
    return Sigma, lambda th: (-0.5 * float(th @ prec @ th), -(prec @ th))
