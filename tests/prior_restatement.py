"""A torch f64 restatement of the reference's BayesianModel.log_target (eeyore/models/bayesian_model.py:30-56) for an MLP or
a logistic regression under ANY elementwise ``torch.distributions`` prior, with the gradient through autograd as
LogTargetModel.upto_grad_log_target takes it (eeyore/models/log_target_model.py:15-23), and of the three draws whose traces
g18_prior_traces.npz records: HMC.draw (hmc.py:100-156), MALA.draw (mala.py:46-82) and the symmetric random-walk
MetropolisHastings.draw (metropolis_hastings.py:41-73).  Everything runs on the CPU.

The parameters are laid out as ``nn.Module.parameters()`` yields them: per layer the weight matrix [d_out, d_in] row-major,
then the bias.  Activation codes 0 none, 1 sigmoid, 2 tanh, 3 relu; likelihood 0 BCE-sum on probabilities
(eeyore/stats/loss.py:1-11, naive logs), 1 CE-sum on logits with the labels argmax(y, 1)."""
import numpy as np
import torch
from torch.distributions import Cauchy, Laplace, Normal, StudentT

F64 = torch.float64
_ACT = {0: lambda v: v, 1: torch.sigmoid, 2: torch.tanh, 3: torch.relu}
FAMILIES = ("laplace", "studentt", "cauchy")


def make_prior(family, loc, scale, df=None):
    """The torch.distributions object of a family name with per-parameter tables (f64 tensors or arrays)."""
    loc, scale = torch.as_tensor(loc, dtype=F64), torch.as_tensor(scale, dtype=F64)
    if family == "normal":
        return Normal(loc, scale)
    if family == "laplace":
        return Laplace(loc, scale)
    if family == "cauchy":
        return Cauchy(loc, scale)
    if family == "studentt":
        return StudentT(torch.as_tensor(df, dtype=F64), loc, scale)
    raise ValueError(family)


class Target:
    """log_lik / log_prior / log_target and the gradient of the log-target of one model on one batch."""

    def __init__(self, dims, acts, lik, x, y, prior, bias=None, temperature=None):
        self.dims, self.acts, self.lik = [int(d) for d in dims], [int(a) for a in acts], int(lik)
        self.bias = [True] * len(self.acts) if bias is None else [bool(b) for b in bias]
        self.x = None if x is None else torch.as_tensor(np.asarray(x), dtype=F64)
        self.y = None if y is None else torch.as_tensor(np.asarray(y), dtype=F64).reshape(self.x.shape[0], -1)
        self.prior, self.temperature = prior, temperature
        self.P = sum((self.dims[k] + (1 if self.bias[k] else 0)) * self.dims[k + 1] for k in range(len(self.acts)))

    def forward(self, th):
        h, off = self.x, 0
        for k, a in enumerate(self.acts):
            din, dout = self.dims[k], self.dims[k + 1]
            W = th[off:off + din * dout].view(dout, din)
            off += din * dout
            h = h @ W.t()
            if self.bias[k]:
                h = h + th[off:off + dout]
                off += dout
            h = _ACT[a](h)
        return h

    def log_lik_t(self, th):
        out = self.forward(th)
        if self.lik == 0:
            v = (out.log() * self.y + (1 - out).log() * (1 - self.y)).sum()
        else:
            v = -torch.nn.CrossEntropyLoss(reduction='sum')(out, torch.argmax(self.y, 1))
        return v if self.temperature is None else self.temperature * v

    def log_prior_t(self, th):
        v = torch.sum(self.prior.log_prob(th))
        return v if self.temperature is None else self.temperature * v

    def parts(self, th):
        """(log_lik, log_prior, log_target, grad of log_target) at th, as floats and a numpy array."""
        t = torch.as_tensor(np.asarray(th, np.float64), dtype=F64).clone().requires_grad_(True)
        ll, lp = self.log_lik_t(t), self.log_prior_t(t)
        tv = ll + lp
        g, = torch.autograd.grad(tv, t)
        return float(ll.detach()), float(lp.detach()), float(tv.detach()), g.numpy().copy()

    def log_prior(self, th):
        with torch.no_grad():
            return float(self.log_prior_t(torch.as_tensor(np.asarray(th, np.float64), dtype=F64)))

    def lik_grad(self, th):
        t = torch.as_tensor(np.asarray(th, np.float64), dtype=F64).clone().requires_grad_(True)
        g, = torch.autograd.grad(self.log_lik_t(t), t)
        return g.numpy().copy()

    def log_target(self, th):
        with torch.no_grad():
            t = torch.as_tensor(np.asarray(th, np.float64), dtype=F64)
            return float(self.log_lik_t(t) + self.log_prior_t(t))

    def value_and_grad(self, th):
        p = self.parts(th)
        return p[2], p[3]


def load_g18():
    """The groups of g18_prior_traces.npz, {'values/<family>/<model>' or 'trace/<family>': rec}, every rec completed with
    its model's spec and data (dims, acts, lik, x, y), its family and the prior's tables (loc, scale, and df for
    Student-t); a values rec has theta, log_lik, log_prior, log_target, grad, a trace rec sampler, step / L or scale, z, u,
    theta0, init_target, init_grad, sample, target_val, accepted."""
    import json

    from tests.helpers import load
    npz = load("g18_prior_traces.npz")
    meta = json.loads(str(npz["meta"]))
    ds = load("datasets.npz")
    data = {"iris": (ds["iris_x"], ds["iris_y"]), "xor": (ds["xor_x"], ds["xor_y"]), "lr": (npz["data/lr/x"], npz["data/lr/y"])}
    grouped, out = {}, {}
    for k in npz.files:
        if k.startswith(("values/", "trace/")):
            g, f = k.rsplit("/", 1)
            grouped.setdefault(g, {})[f] = npz[k]
    for key, rec in grouped.items():
        family = key.split("/")[1]
        tr = meta["traces"][family] if key.startswith("trace/") else None
        model = meta["models"][tr["model"] if tr else key.split("/")[2]]
        x, y = data[model["data"]]
        rec.update(dims=np.array(model["dims"]), acts=np.array(model["acts"]), lik=np.array(model["lik"]), x=x, y=y,
                   family=family, loc=rec["tables"][0], scale=rec["tables"][1])
        if family == "studentt":
            rec["df"] = rec["tables"][2]
        if tr:
            rec["sampler"] = tr["sampler"]
            rec["scale_mh" if tr["sampler"] == "mh" else "step"] = tr["par"]
            rec["L"] = tr.get("L", 0)
        else:
            rec.update(log_lik=rec["parts"][:, 0], log_prior=rec["parts"][:, 1], log_target=rec["parts"][:, 2])
        out[key] = rec
    return out


def group_target(rec, family=None, temperature=None):
    """The Target of a group of load_g18() (its model, data, family and tables)."""
    fam = str(rec["family"]) if family is None else family
    prior = make_prior(fam, rec["loc"], rec["scale"], rec["df"] if "df" in rec else None)
    return Target(rec["dims"].tolist(), rec["acts"].tolist(), int(rec["lik"]), rec["x"], rec["y"], prior,
                  temperature=temperature)


# ------------------------------------------------------------------------------------------------ the three draws
def hmc_draw(value_and_grad, theta, target, grad, z, u, step, L):
    """HMC.draw with the cached gradient at the start of the trajectory (the value hmc.py:104 recomputes).
    Returns (theta, target, grad, accepted, log of the unclipped rate)."""
    th, p = np.array(theta, np.float64), np.array(z, np.float64)
    h_cur = -target + 0.5 * np.sum(p ** 2)
    p = p + 0.5 * step * grad
    t, g = target, grad
    for k in range(L):
        th = th + step * p
        t, g = value_and_grad(th)
        p = p + (step if k < L - 1 else 0.5 * step) * g
    h_prop = -t + 0.5 * np.sum(p ** 2)
    log_rate = h_cur - h_prop
    with np.errstate(over="ignore"):
        acc = bool(u < min(np.exp(log_rate), 1.0))
    return (th, t, g, acc, log_rate) if acc else (np.asarray(theta), target, grad, acc, log_rate)


def _normal_log_prob(loc, sd, v):
    return float(torch.sum(Normal(torch.as_tensor(loc), torch.as_tensor(sd, dtype=F64)).log_prob(torch.as_tensor(v))))


def mala_draw(value_and_grad, theta, target, grad, z, u, step):
    """MALA.draw with its NormalKernel(theta + step/2 grad, sqrt(step)) proposal."""
    theta = np.asarray(theta, np.float64)
    sd = np.sqrt(step)
    loc = theta + 0.5 * step * grad
    prop = loc + sd * np.asarray(z, np.float64)
    tp, gp = value_and_grad(prop)
    log_rate = tp - target
    log_rate = log_rate - _normal_log_prob(loc, sd, prop)
    log_rate = log_rate + _normal_log_prob(prop + 0.5 * step * gp, sd, theta)
    acc = bool(np.log(u) < log_rate)
    return (prop, tp, gp, acc, log_rate) if acc else (theta, target, grad, acc, log_rate)


def mh_draw(log_target, theta, target, z, u, scale):
    """The symmetric random-walk MetropolisHastings.draw with a NormalKernel(theta, scale) proposal."""
    theta = np.asarray(theta, np.float64)
    prop = theta + scale * np.asarray(z, np.float64)
    tp = log_target(prop)
    log_rate = tp - target
    acc = bool(np.log(u) < log_rate)
    return (prop, tp, acc, log_rate) if acc else (theta, target, acc, log_rate)


def replay(rec, tgt=None):
    """Replays a trace group of load_g18() from its recorded (z, u): (samples [n, P], targets [n], accepted [n], margins [n]),
    margin = |log u - log rate|."""
    tgt = tgt or group_target(rec)
    kind = str(rec["sampler"])
    th, t = np.array(rec["theta0"], np.float64), float(rec["init_target"])
    g = np.array(rec["init_grad"], np.float64)
    out = dict(sample=[], target_val=[], accepted=[], margin=[])
    for it in range(rec["z"].shape[0]):
        z, u = rec["z"][it], float(rec["u"][it])
        if kind == "hmc":
            th, t, g, acc, lr = hmc_draw(tgt.value_and_grad, th, t, g, z, u, float(rec["step"]), int(rec["L"]))
        elif kind == "mala":
            th, t, g, acc, lr = mala_draw(tgt.value_and_grad, th, t, g, z, u, float(rec["step"]))
        else:
            th, t, acc, lr = mh_draw(tgt.log_target, th, t, z, u, float(rec["scale_mh"]))
        out["sample"].append(np.array(th)); out["target_val"].append(t); out["accepted"].append(int(acc))
        out["margin"].append(abs(np.log(u) - lr))
    return {k: np.array(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the other samplers
OTHER_SAMPLERS = ("ram", "am", "gibbs", "mh_tril", "mala_tril")
OTHER_DIMS, OTHER_ACTS, OTHER_LIK = [4, 3, 3], [1, 0], 1
OTHER_BLOCKS = [[4 * n + i for i in range(4)] + [12 + n] for n in range(3)] + [[15 + 3 * n + i for i in range(3)] + [24 + n]
                                                                               for n in range(3)]  # the nodes of MLP(4-3-3)
OTHER_PAR = dict(ram=dict(a=0.234, g=0.7, chol0=0.1), am=dict(l=0.3, b=0.5, c=0.1, eps=1e-2, t0=2, cov0=0.01),
                 gibbs=dict(scale=0.3), mh_tril=dict(scale=0.1), mala_tril=dict(scale=0.1, step=0.01))


def distinct_tables(P, seed):
    """loc, scale, df [P] with all entries different (shuffled grids)."""
    rng = np.random.default_rng(seed)
    return (rng.permutation(np.linspace(-0.4, 0.5, P)), rng.permutation(np.linspace(0.6, 2.2, P)),
            rng.permutation(np.linspace(1.5, 9.0, P)))


def dense_lower(P, scale, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((P, P)) / np.sqrt(P)
    return scale * np.linalg.cholesky(A @ A.T + 0.5 * np.eye(P))


def other_case(sampler, family, seed=0, C=11, steps=5):
    """The inputs of ``steps`` draws of C chains of one of OTHER_SAMPLERS on MLP(4-3-3) / iris under a Laplace or Student-t
    prior with distinct tables, and what the f64 restatements (ram / am / gibbs / mh_mvn / mala_mvn _restatement with this
    module's target) make of them: per step the states [C, P], targets [C], decisions and margins |log u - log rate|
    (Gibbs: per sub-step).  Needs no GPU."""
    from tests import cross_restatement as cr  # (it imports this module: the loop over steps and chains lives there)
    from tests.helpers import load
    ds = load("datasets.npz")
    x, y = ds["iris_x"], ds["iris_y"]
    P = 27
    loc, scale, df = distinct_tables(P, 100 + seed)
    tgt = Target(OTHER_DIMS, OTHER_ACTS, OTHER_LIK, x, y, make_prior(family, loc, scale, df))
    par = OTHER_PAR[sampler]
    rng = np.random.default_rng(7000 + 10 * seed + OTHER_SAMPLERS.index(sampler))
    S = len(OTHER_BLOCKS)
    d = dict(x=x, y=y, loc=loc, scale=scale, df=df if family == "studentt" else None, par=par, target=tgt,
             th0=0.3 * rng.standard_normal((C, P)), z=rng.standard_normal((steps, C, P)),
             u=rng.random((steps, C, S) if sampler == "gibbs" else (steps, C)), u_mix=rng.random((steps, C)))
    if sampler in ("mh_tril", "mala_tril"):
        d["L"] = dense_lower(P, par["scale"], 50 + seed)
    return cr.run_case(sampler, tgt, par, d, blocks=OTHER_BLOCKS)
