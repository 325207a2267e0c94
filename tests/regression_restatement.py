"""A torch f64 restatement of the three regression likelihoods (include/eeyore_amd.h: EY_LIK_GAUSS_SUM, _LAPLACE_SUM,
_POISSON_SUM) as the reference evaluates them: BayesianModel.log_lik = -loss(forward(x), y)
(eeyore/models/bayesian_model.py:30-35) with ``loss`` one of

    gauss     -Normal(out, s).log_prob(y).sum()
    laplace   -Laplace(out, s).log_prob(y).sum()
    poisson   nn.PoissonNLLLoss(log_input=True, full=False, reduction='sum')(out, y)

the gradient through autograd (eeyore/models/log_target_model.py:15-23), and the samplers' draws.  HMC.draw, MALA.draw and
the random-walk MetropolisHastings.draw are tests/prior_restatement.py's (they take any value_and_grad); RAM, AM and Gibbs
are the restatements of their own test suites.  Everything runs on the CPU.

The parameters are laid out as ``nn.Module.parameters()`` yields them; activation codes 0 none, 1 sigmoid, 2 tanh, 3 relu."""
import json

import numpy as np
import torch
from torch.distributions import Laplace, Normal

from tests import prior_restatement as pr
from tests.prior_restatement import hmc_draw, mala_draw, mh_draw  # noqa: F401  (the draws of the recorded traces)

F64 = torch.float64
LOSSES = ("gauss", "laplace", "poisson")
CODE = {"gauss": 2, "laplace": 3, "poisson": 4}
NAME = {v: k for k, v in CODE.items()}


def loss_fn(name, scale=1.0):
    """The reference-side callable of a loss name: what a user of the reference passes as ``loss``."""
    if name == "gauss":
        return lambda out, y: -Normal(out, scale).log_prob(y).sum()
    if name == "laplace":
        return lambda out, y: -Laplace(out, scale).log_prob(y).sum()
    if name == "poisson":
        return torch.nn.PoissonNLLLoss(log_input=True, full=False, reduction='sum')
    raise ValueError(name)


class Target(pr.Target):
    """tests/prior_restatement.py's Target with a regression likelihood: ``lik`` a code (2, 3, 4) or a name of LOSSES,
    ``scale`` the noise scale of the Gaussian and Laplace forms.  The prior defaults to N(0, sigma^2) on every parameter."""

    def __init__(self, dims, acts, lik, x, y, scale=1.0, prior=None, sigma=1.0, bias=None, temperature=None):
        code = CODE[lik] if isinstance(lik, str) else int(lik)
        super().__init__(dims, acts, code, x, y, prior, bias=bias, temperature=temperature)
        self.scale = float(scale)
        self.loss = loss_fn(NAME[code], self.scale)
        if prior is None:
            self.prior = Normal(torch.zeros(self.P, dtype=F64), torch.full((self.P,), float(sigma), dtype=F64))

    def log_lik_t(self, th):
        v = -self.loss(self.forward(th), self.y)
        return v if self.temperature is None else self.temperature * v

    def outputs(self, th):
        """forward(x) at th: [N, dK] as a numpy array."""
        with torch.no_grad():
            return self.forward(torch.as_tensor(np.asarray(th, np.float64), dtype=F64)).numpy().copy()

    def rows(self, th):
        """The N row terms of log_lik (untempered), as ey_log_lik_rows returns them."""
        with torch.no_grad():
            out = self.forward(torch.as_tensor(np.asarray(th, np.float64), dtype=F64))
            if self.lik == 2:
                r = Normal(out, self.scale).log_prob(self.y)
            elif self.lik == 3:
                r = Laplace(out, self.scale).log_prob(self.y)
            else:
                r = self.y * out - out.exp()
            return r.sum(1).numpy().copy()


def synthetic(dims, lik, N, seed=0):
    """N rows for a regression model: x ~ N(0, 1); y = a smooth function of x plus noise, or counts for the Poisson form."""
    name = NAME[lik] if not isinstance(lik, str) else lik
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, dims[0]))
    f = np.stack([np.sin(x @ rng.standard_normal(dims[0])) for _ in range(dims[-1])], 1)
    if name == "poisson":
        y = rng.poisson(np.exp(0.5 + 0.8 * f)).astype(np.float64)
    else:
        y = f + 0.3 * rng.standard_normal(f.shape)
    return x, y


# ------------------------------------------------------------------------------------------------ the fixture
def load_g19():
    """The groups of g19_regression_traces.npz, {'values/<loss>/<model>' or 'trace/<loss>': rec}, every rec completed with
    its model's spec and data (dims, acts, x, y), its loss name, likelihood code, scale and the prior's sigma; a values rec
    has theta, log_lik, log_prior, log_target, grad, a trace rec sampler, step / L or scale_mh, z, u, theta0, init_target,
    init_grad, sample, target_val, accepted."""
    from tests.helpers import load
    npz = load("g19_regression_traces.npz")
    meta = json.loads(str(npz["meta"]))
    grouped, out = {}, {}
    for k in npz.files:
        if k.startswith(("values/", "trace/")):
            g, f = k.rsplit("/", 1)
            grouped.setdefault(g, {})[f] = npz[k]
    for key, rec in grouped.items():
        loss = key.split("/")[1]
        tr = meta["traces"][loss] if key.startswith("trace/") else None
        mname = tr["model"] if tr else key.split("/")[2]
        model = meta["models"][mname]
        rec.update(dims=np.array(model["dims"]), acts=np.array(model["acts"]), x=npz[f"data/{mname}/x"],
                   y=npz[f"data/{mname}/{'counts' if loss == 'poisson' else 'y'}"], loss=loss, lik=CODE[loss],
                   lik_scale=meta["scales"][loss], sigma=meta["sigma"])
        if tr:
            rec["sampler"] = tr["sampler"]
            rec["scale_mh" if tr["sampler"] == "mh" else "step"] = tr["par"]
            rec["L"] = tr.get("L", 0)
        else:
            rec.update(log_lik=rec["parts"][:, 0], log_prior=rec["parts"][:, 1], log_target=rec["parts"][:, 2])
        out[key] = rec
    return out


def group_target(rec, temperature=None):
    """The Target of a group of load_g19()."""
    return Target(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"],
                  scale=float(rec["lik_scale"]), sigma=float(rec["sigma"]), temperature=temperature)


def replay(rec, tgt=None):
    """Replays a trace group of load_g19() from its recorded (z, u), as tests/prior_restatement.py's replay does."""
    return pr.replay(rec, tgt or group_target(rec))


# ------------------------------------------------------------------------------------------------ every sampler, C chains
SAMPLERS = ("hmc", "mala", "mh", "ram", "am", "gibbs")
S_DIMS, S_ACTS = [2, 3, 1], [2, 0]
S_BLOCKS = [[2 * n, 2 * n + 1, 6 + n] for n in range(3)] + [[9, 10, 11, 12]]  # the nodes of MLP(2-3-1)
S_PAR = dict(hmc=dict(step=0.05, L=4), mala=dict(step=0.01), mh=dict(scale=0.08), ram=dict(a=0.234, g=0.7, chol0=0.1),
             am=dict(l=0.3, b=0.5, c=0.1, eps=1e-2, t0=2, cov0=0.01), gibbs=dict(scale=0.25))


def sampler_case(sampler, loss="gauss", scale=0.5, seed=0, C=11, steps=5, N=40):
    """The inputs of ``steps`` draws of C chains of one of SAMPLERS on MLP(2-3-1) (tanh, identity) under a regression
    likelihood, and what the f64 restatements make of them: per step the states [C, P], targets [C], decisions and margins
    |log u - log rate| (Gibbs: per sub-step).  Needs no GPU."""
    from tests import cross_restatement as cr  # (it imports this module: the loop over steps and chains lives there)
    x, y = synthetic(S_DIMS, loss, N, seed=20 + seed)
    tgt = Target(S_DIMS, S_ACTS, loss, x, y, scale=scale, sigma=2.0)
    P = tgt.P
    par = S_PAR[sampler]
    rng = np.random.default_rng(9000 + 10 * seed + SAMPLERS.index(sampler))
    S = len(S_BLOCKS)
    d = dict(x=x, y=y, par=par, target=tgt, lik=CODE[loss], lik_scale=scale, sigma=2.0,
             th0=0.3 * rng.standard_normal((C, P)), z=rng.standard_normal((steps, C, P)),
             u=rng.random((steps, C, S) if sampler == "gibbs" else (steps, C)), u_mix=rng.random((steps, C)))
    return cr.run_case(sampler, tgt, par, d, blocks=S_BLOCKS)


# ------------------------------------------------------------------------------------------------ the closed form
def linear_gaussian(N=50, s=0.7, sigma=2.0, seed=3):
    """A one-layer plan (dims [3, 1], identity, bias) under a Gaussian likelihood of scale s and a N(0, sigma^2) prior: its
    posterior is Gaussian with precision X^T X / s^2 + I / sigma^2 (X with the ones column last, as theta = (w, b)) and
    mean precision^-1 X^T y / s^2.  Returns x, y, mean [4], cov [4, 4]."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, 3))
    y = x @ np.array([0.8, -0.5, 0.3]) + 0.2 + s * rng.standard_normal(N)
    X = np.concatenate([x, np.ones((N, 1))], 1)
    prec = X.T @ X / s ** 2 + np.eye(4) / sigma ** 2
    cov = np.linalg.inv(prec)
    return x, y[:, None], cov @ X.T @ y / s ** 2, cov


CLOSED_FORM_STEP, CLOSED_FORM_L = 0.1, 2  # the restated HMC accepts between 0.6 and 0.95 of its proposals (host test)


def hmc_acceptance(tgt, step, L, C=64, iters=30, seed=0):
    """The acceptance rate of the restated HMC.draw on a target from dispersed starts (after 10 draws of warm-up)."""
    rng = np.random.default_rng(seed)
    acc = []
    for c in range(C):
        th = 0.1 * rng.standard_normal(tgt.P)
        t, g = tgt.value_and_grad(th)
        for it in range(iters):
            th, t, g, a, _ = hmc_draw(tgt.value_and_grad, th, t, g, rng.standard_normal(tgt.P), rng.random(), step, L)
            if it >= 10:
                acc.append(a)
    return float(np.mean(acc))
