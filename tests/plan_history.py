"""What the plan-history tests share (tests/test_plan_history_gpu.py, tests/test_plan_history_host.py; DESIGN.md section 2,
"A plan's history"): the record of a plan's configuration with the function that builds a fresh plan in exactly that
configuration, the operations that change a live plan and its record together, the seeded script generator with its forced
coverage, and the probe.  Nothing here asserts: the probe returns named tensors and `first_difference` names the first
that differs.

The property: after ANY sequence of reconfigurations a long-lived plan gives the same bits as a plan created now, directly
in the current configuration.  Both run the same kernels on the same inputs with the same in-kernel Philox keys, so the
comparison is on bits and the reference is the fresh plan (which the rest of the suite holds to the f64 oracle)."""
import dataclasses
import itertools

import numpy as np
import torch

from tests.test_small_batches import FAMILIES as SMALL_BATCH_FAMILIES

DEV = "cuda:0"
CHAINS = (1, 3, 37)   # the probe's chain counts, in turn (an attachment fixes the count for as long as it lasts)
GROW = 1024           # the chain count of the 'big' operation
SCRIPT_LEN = 24       # operations of a script, where the forced coverage does not need more
STEP, LSTEPS, MALA_STEP, MH_SCALE = 0.01, 4, 1e-4, 1e-3
RUN_ITERS, RUN_EVERY = 3, 4
BUMP = 0.125          # what 'data_inplace' adds to x
DA_ROWS = 256         # rows of an attached dual-averaging table: more than a script's probes can use up
SEED = 20260

_TORCH = {"f32": torch.float32, "f64": torch.float64}
_NP = {"f32": np.float32, "f64": np.float64}

# the row counts a family's data operations move among: the limits of the kernels that serve it
N_MFMA32 = (1, 24, 25, 33, 320, 352, 512, 600, 768, 800)   # peeled tile, piece image, bf16x3 limit, fused16 and back
N_FUSED16 = (1, 16, 17, 100)
N_LAYERWISE = (1, 10, 13, 130)
N_GENERIC = (1, 5, 129)


@dataclasses.dataclass(frozen=True)
class Family:
    name: str
    kind: str                 # 'mlp', 'mixture' or 'tilt'
    dims: tuple = ()
    acts: tuple = ()
    bias: tuple = ()
    lik: int = 1
    tag: str = "f64"
    kernel: str = "generic"   # Plan.kernel of the starting configuration
    variant: int = 0          # the variant bits of the family's row: set_variant moves among their subsets
    products: str = ""        # the row's f32_products ('' on a row that names none)
    ns: tuple = ()
    priors: bool = False      # the generic kernels can hold the model: Laplace, Student-t and Cauchy priors are served
    fused: bool = False       # always served by mfma32 or fused16 under a Normal prior: dual averaging can be attached
    chunks: bool = False      # the layerwise rows: max_chunk_chains
    P: int = 0


def _row(name, fam, dims, tag, ns, **kw):
    """A Family from the row (fam, dims, tag) of tests/test_small_batches.py::FAMILIES: its tuples, variant bits and
    expected kernel name."""
    for f, d, acts, bias, lik, t, kern, opts, _, _ in SMALL_BATCH_FAMILIES:
        if (f, d, t) == (fam, list(dims), tag):
            bias = tuple(bias) if bias is not None else (1,) * (len(d) - 1)
            P = sum((d[l] + bias[l]) * d[l + 1] for l in range(len(d) - 1))
            return Family(name, "mlp", tuple(d), tuple(acts), bias, lik, t, kern, opts.get("variant", 0),
                          opts.get("products", ""), tuple(ns), P=P, **kw)
    raise KeyError((fam, dims, tag))


FAMILY_LIST = [
    _row("mfma32-bf16x3", "mfma32-bf16x3", [4, 32, 32, 3], "f32", N_MFMA32, priors=True, fused=True),
    _row("mfma32-exact", "mfma32-exact", [4, 32, 32, 3], "f32", N_MFMA32, priors=True, fused=True),
    _row("mfma32-kind2", "mfma32-kind2", [4, 32, 32, 1], "f32", N_MFMA32, priors=True, fused=True),
    _row("fused16-f64", "fused16", [6, 20, 24, 2], "f64", N_FUSED16, priors=True, fused=True),
    _row("fused16-f32", "fused16", [3, 64, 64, 4], "f32", N_FUSED16, priors=True, fused=True),
    _row("generic-regs-f32", "generic-regs", [2, 3, 2, 1], "f32", N_GENERIC, priors=True),
    _row("generic-lds-f64", "generic-lds", [4, 8, 8, 8, 3], "f64", N_GENERIC, priors=True),
    _row("layerwise-784-f32", "layerwise", [784, 128, 10], "f32", N_LAYERWISE, chunks=True),
    _row("layerwise-6-f64", "layerwise", [6, 16, 10], "f64", N_LAYERWISE, priors=True, chunks=True),
    _row("k_mid32", "k_mid32", [64, 32, 32, 10], "f32", N_LAYERWISE, priors=True),
    _row("k_mid", "k_mid", [10, 100, 10], "f32", N_LAYERWISE, priors=True),
    # a Gaussian likelihood (EY_LIK_GAUSS_SUM = 2) for set_lik_scale; the two densities on theta itself
    Family("regression", "mlp", (3, 4, 1), (2, 0), (1, 1), 2, "f64", "generic", ns=N_GENERIC, priors=True, P=21),
    Family("mixture", "mixture", tag="f64", kernel="dist", P=5),
    Family("exp_tilt", "tilt", tag="f64", kernel="dist", P=5),
]
FAMILY = {f.name: f for f in FAMILY_LIST}

NORMAL_PRIORS = ("uniform", "elem")
FAMILY_PRIORS = ("laplace", "student", "cauchy")
REFUSALS = ("bad_sigma", "bad_df", "bad_cols", "bad_theta_dtype", "bad_lik_scale", "bad_index")


# ------------------------------------------------------------------------------------------------------- the record
@dataclasses.dataclass(frozen=True)
class Config:
    """Everything a plan was told that its answers may depend on.  `bumps`: how often x was changed in place since it was
    drawn; `moments`: the chain count of the attached accumulators or None; `da`: (chain count, seed, rows of the table
    already used) of the attached dual averaging or None."""
    family: str
    n: int = 0
    data_seed: int = 0
    bumps: int = 0
    prior: tuple = ("uniform", 0)
    products: str = ""
    variant: int = 0
    row_waves: str = "off"
    max_chunk: int = 0
    lik_scale: float = 1.0
    moments: object = None
    da: object = None


def start(fam):
    """The configuration a family's script starts from: the row of tests/test_small_batches.py as it stands."""
    if fam.kind != "mlp":
        return Config(fam.name)
    return Config(fam.name, n=fam.ns[0], products=fam.products or ("bf16x3" if fam.tag == "f32" else ""),
                  variant=fam.variant)


def setup_calls(cfg):
    """The calls that put a new plan into `cfg`, in order: what `build` executes and `record_of` reads back."""
    fam = FAMILY[cfg.family]
    calls = [("create", cfg.family)]
    if fam.kind == "mlp":
        calls += [("variant", cfg.variant), ("products", cfg.products), ("row_waves", cfg.row_waves),
                  ("max_chunk", cfg.max_chunk), ("lik_scale", cfg.lik_scale),
                  ("data", cfg.n, cfg.data_seed, cfg.bumps), ("prior",) + tuple(cfg.prior)]
    if cfg.moments is not None:
        calls.append(("moments", cfg.moments))
    if cfg.da is not None:
        calls.append(("da",) + tuple(cfg.da))
    return calls


def record_of(calls):
    """The configuration that `calls` (of `setup_calls`) leave a new plan in."""
    cfg = None
    for c in calls:
        what, a = c[0], c[1:]
        if what == "create":
            cfg = Config(a[0])
        elif what == "data":
            cfg = dataclasses.replace(cfg, n=a[0], data_seed=a[1], bumps=a[2])
        elif what == "prior":
            cfg = dataclasses.replace(cfg, prior=tuple(a))
        elif what == "da":
            cfg = dataclasses.replace(cfg, da=tuple(a))
        else:
            cfg = dataclasses.replace(cfg, **{what: a[0]})
    return cfg


# ----------------------------------------------------------------------------------------------- what the calls hold
def data_arrays(fam, n, seed, cols=None):
    """(x [n, d0], y [n, dK]) of the family's dtype as host arrays; `cols` another column count for x."""
    rng = np.random.default_rng([SEED, 1, n, seed])
    d0, dK, npdt = fam.dims[0], fam.dims[-1], _NP[fam.tag]
    x = rng.standard_normal((n, cols or d0)).astype(npdt)
    if fam.lik == 1:
        y = np.eye(dK, dtype=npdt)[rng.integers(0, dK, n)]
    elif fam.lik == 0:
        y = (rng.random((n, dK)) < 0.5).astype(npdt)
    else:
        y = rng.standard_normal((n, dK)).astype(npdt)
    return x, y


def prior_arrays(fam, kind, seed):
    """(loc, scale, df or None) [P] of the family's dtype as host tensors: 'uniform' one pair for every parameter."""
    rng = np.random.default_rng([SEED, 2, NORMAL_PRIORS.index(kind) if kind in NORMAL_PRIORS else 9, seed])
    P, dt = fam.P, _TORCH[fam.tag]
    if kind == "uniform":
        loc, scale = np.full(P, 0.1 * rng.standard_normal()), np.full(P, 0.8 + rng.random())
    else:
        loc, scale = 0.1 * rng.standard_normal(P), 0.5 + rng.random(P)
    df = None
    if kind == "student":
        df = torch.tensor(2.0 + 4.0 * rng.random(P), dtype=dt)
    elif kind == "cauchy":
        df = torch.ones(P, dtype=dt)
    return torch.tensor(loc, dtype=dt), torch.tensor(scale, dtype=dt), df


def mixture_tables(P):
    rng = np.random.default_rng([SEED, 3])
    M = 3
    a = 0.3 * rng.standard_normal((M, P, P))
    prec = np.einsum("mij,mkj->mik", a, a) + np.eye(P)[None]
    return np.log(np.array([0.5, 0.3, 0.2])), 0.7 * rng.standard_normal((M, P)), prec


def tilt_tables(P):
    rng = np.random.default_rng([SEED, 4])
    return (0.1 * rng.standard_normal(P), 0.5 + rng.random(P), 0.5 + rng.random(P), 0.5 + 0.5 * rng.random(P))


def da_tensors(C, seed, dtype):
    """(state [C, 3], step_vec [C], table [DA_ROWS, 3]) of a dual averaging that has adapted nothing yet."""
    t = np.arange(1, DA_ROWS + 1, dtype=np.float64)
    table = np.stack([1.0 / (t + 10.0), np.sqrt(t) / 0.05, t ** -0.75], axis=1)
    state = np.zeros((C, 3))
    state[:, 2] = np.log(10 * STEP) + 0.01 * np.random.default_rng([SEED, 5, seed]).standard_normal(C)
    return (torch.tensor(state, device=DEV), torch.full((C,), STEP, dtype=dtype, device=DEV),
            torch.tensor(table, device=DEV))


# ------------------------------------------------------------------------------------------------------ a live plan
class Live:
    """A plan with the tensors it was handed that a later operation needs again (the batch objects, the attached buffers)
    and the record of its configuration."""

    def __init__(self, cfg):
        self.cfg, self.plan = cfg, None
        self.x = self.y = None
        self.mom = self.da = None   # (s1, s2, acc) / (state, step_vec, table)

    @property
    def fam(self):
        return FAMILY[self.cfg.family]


def _new_moments(C, P):
    return (torch.zeros(C, P, dtype=torch.float64, device=DEV), torch.zeros(C, P, dtype=torch.float64, device=DEV),
            torch.zeros(C, dtype=torch.float64, device=DEV))


def _attach_da(lv, C, seed, done, like=None):
    """Attach a dual averaging that has used `done` rows of its table: a new one, or `like`'s state and step as they are
    now, under the rows that are left (ey_api.hip, da_window: a launch reads the table from row da_done on)."""
    state, step, table = da_tensors(C, seed, lv.plan.dtype)
    if like is not None:
        state, step = like.da[0].clone(), like.da[1].clone()
    lv.da = (state, step, table)
    lv.plan.attach_da(state, step, table[done:], DA_ROWS - done, 0.8)


def _set_prior(plan, fam, kind, seed):
    from eeyore_amd import _lib as L
    loc, scale, df = prior_arrays(fam, kind, seed)
    if kind in NORMAL_PRIORS:
        plan.set_prior(loc, scale)
    elif kind == "laplace":
        plan.set_prior_family(L.EY_PRIOR_LAPLACE, loc, scale)
    else:
        plan.set_prior_family(L.EY_PRIOR_STUDENT_T, loc, scale, df)


def _set_data(lv, n, seed, bumps):
    x, y = data_arrays(lv.fam, n, seed)
    lv.x, lv.y = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    for _ in range(bumps):
        lv.x.add_(BUMP)
    lv.plan.set_data(lv.x, lv.y)


def build(cfg, like=None):
    """A new plan directly in `cfg` (the calls of `setup_calls`, nothing else); an attached dual averaging continues from
    `like`'s state."""
    from eeyore_amd.plan import Plan
    lv = Live(cfg)
    fam = lv.fam
    for c in setup_calls(cfg):
        what, a = c[0], c[1:]
        if what == "create":
            dt = _TORCH[fam.tag]
            if fam.kind == "mixture":
                lv.plan = Plan.mixture(*mixture_tables(fam.P), dt, DEV)
            elif fam.kind == "tilt":
                lv.plan = Plan.exp_tilt(*tilt_tables(fam.P), dt, DEV)
            else:
                lv.plan = Plan(list(fam.dims), list(fam.bias), list(fam.acts), fam.lik, dt, DEV)
        elif what == "variant":
            lv.plan.set_variant(a[0])
        elif what == "products":
            if a[0]:
                lv.plan.f32_products = a[0]
        elif what == "row_waves":
            lv.plan.row_waves = a[0]
        elif what == "max_chunk":
            lv.plan.max_chunk_chains = a[0]
        elif what == "lik_scale":
            if fam.lik == 2:
                lv.plan.set_lik_scale(a[0])
        elif what == "data":
            _set_data(lv, *a)
        elif what == "prior":
            _set_prior(lv.plan, fam, *a)
        elif what == "moments":
            lv.mom = _new_moments(a[0], fam.P)
            lv.plan.attach_moments(*lv.mom)
        elif what == "da":
            _attach_da(lv, *a, like=like)
    return lv


# --------------------------------------------------------------------------------------------------- the operations
# An operation is a tuple (kind, arguments...).  `legal` says whether it may follow a record, `after` what record it
# leaves, `apply` does it to a live plan; a refused call leaves the record as it was.
def kinds(fam):
    """Every operation kind the family's script must contain ('data_n' apart: the crossings of its row counts)."""
    if fam.kind != "mlp":
        return ["attach_moments", "detach_moments", "big", "bad_theta_dtype", "bad_index"]
    ks = ["data_content", "data_same", "data_inplace", "prior_uniform", "prior_elem", "row_waves", "attach_moments",
          "detach_moments", "big", "bad_sigma", "bad_df", "bad_cols", "bad_theta_dtype"]
    if fam.priors:
        ks += ["prior_" + k for k in FAMILY_PRIORS]
    if fam.tag == "f32":
        ks.append("products")
    if fam.variant:
        ks.append("variant")
    if fam.chunks:
        ks.append("max_chunk")
    if fam.lik == 2:
        ks += ["lik_scale", "bad_lik_scale"]
    if fam.fused:
        ks += ["attach_da", "detach_da"]
    return ks


def variant_choices(fam):
    bits = [1 << b for b in range(15) if fam.variant >> b & 1]
    return sorted({sum(s) for r in range(len(bits) + 1) for s in itertools.combinations(bits, r)})


def legal(cfg, op):
    kind = op[0]
    fam = FAMILY[cfg.family]
    if kind == "data_n":
        return fam.kind == "mlp" and op[1] != cfg.n
    if kind not in kinds(fam):
        return False
    if kind == "attach_moments":
        return cfg.moments is None
    if kind == "detach_moments":
        return cfg.moments is not None
    if kind == "attach_da":   # the generic kernels, which serve the other prior families, refuse to adapt in the kernel
        return cfg.da is None and cfg.prior[0] in NORMAL_PRIORS
    if kind == "detach_da":
        return cfg.da is not None
    if kind in ("prior_" + k for k in FAMILY_PRIORS):
        return cfg.da is None
    return True


def draw(cfg, kind, rng):
    """An operation of that kind with its arguments drawn for the record it is to follow."""
    fam = FAMILY[cfg.family]
    seed = int(rng.integers(1, 1 << 20))
    if kind in ("data_content", "bad_sigma", "bad_df", "bad_cols") or kind.startswith("prior_"):
        return (kind, seed)
    if kind == "data_n":
        return (kind, int(rng.choice([n for n in fam.ns if n != cfg.n])), seed)
    if kind == "variant":
        return (kind, int(rng.choice([v for v in variant_choices(fam) if v != cfg.variant])))
    if kind == "max_chunk":
        return (kind, int(rng.choice([k for k in (0, 1, 2) if k != cfg.max_chunk])))
    if kind == "lik_scale":
        return (kind, float(rng.choice([s for s in (0.5, 1.0, 1.75) if s != cfg.lik_scale])))
    if kind in ("attach_moments", "attach_da"):
        other = cfg.da[0] if cfg.da is not None else cfg.moments
        return (kind, int(other if other is not None else rng.choice(CHAINS)), seed)
    return (kind,)


def after(cfg, op):
    kind, a = op[0], op[1:]
    r = dataclasses.replace
    if kind == "data_content":
        return r(cfg, data_seed=a[0], bumps=0)
    if kind == "data_n":
        return r(cfg, n=a[0], data_seed=a[1], bumps=0)
    if kind == "data_inplace":
        return r(cfg, bumps=cfg.bumps + 1)
    if kind.startswith("prior_"):
        return r(cfg, prior=(kind[6:], a[0]))
    if kind == "products":
        return r(cfg, products="exact" if cfg.products == "bf16x3" else "bf16x3")
    if kind == "row_waves":
        return r(cfg, row_waves="on" if cfg.row_waves == "off" else "off")
    if kind in ("variant", "max_chunk", "lik_scale"):
        return r(cfg, **{kind: a[0]})
    if kind == "attach_moments":
        return r(cfg, moments=a[0])
    if kind == "detach_moments":
        return r(cfg, moments=None)
    if kind == "attach_da":
        return r(cfg, da=(a[0], a[1], 0))
    if kind == "detach_da":
        return r(cfg, da=None)
    return cfg   # data_same, big and every refused call


def after_probe(cfg, hmc_iters):
    """The record behind a probe: its HMC draws have used that many rows of an attached dual-averaging table."""
    if cfg.da is None:
        return cfg
    return dataclasses.replace(cfg, da=(cfg.da[0], cfg.da[1], min(DA_ROWS, cfg.da[2] + hmc_iters)))


def apply(lv, op):
    """Do `op` to the live plan and its record.  Returns the exception a refused call raised (None: it returned)."""
    from eeyore_amd import _lib as L
    kind, a = op[0], op[1:]
    pl, fam, cfg = lv.plan, lv.fam, lv.cfg
    new = after(cfg, op)
    raised = None
    try:
        if kind in ("data_content", "data_n"):
            _set_data(lv, new.n, new.data_seed, 0)
        elif kind == "data_same":
            pl.set_data(lv.x, lv.y)
        elif kind == "data_inplace":
            lv.x.add_(BUMP)
            pl.set_data(lv.x, lv.y)
        elif kind.startswith("prior_"):
            _set_prior(pl, fam, *new.prior)
        elif kind == "products":
            pl.f32_products = new.products
        elif kind == "row_waves":
            pl.row_waves = new.row_waves
        elif kind == "variant":
            pl.set_variant(new.variant)
        elif kind == "max_chunk":
            pl.max_chunk_chains = new.max_chunk
        elif kind == "lik_scale":
            pl.set_lik_scale(new.lik_scale)
        elif kind == "attach_moments":
            lv.mom = _new_moments(a[0], fam.P)
            pl.attach_moments(*lv.mom)
        elif kind == "detach_moments":
            pl.detach_moments()
            lv.mom = None
        elif kind == "attach_da":
            _attach_da(lv, a[0], a[1], 0)
        elif kind == "detach_da":
            pl.detach_da()
            lv.da = None
        elif kind == "big":
            th = (0.1 * pl.philox_normal(GROW, seed=99, it=0)).contiguous()
            pl.log_target_grad(th, temp=torch.full((GROW,), 0.8, dtype=pl.dtype, device=DEV))
        # ---- the refused calls: each is validated on the host before anything is launched or stored
        elif kind == "bad_sigma":      # ey_plan_set_prior validates sigma before it writes
            loc, scale, _ = prior_arrays(fam, "elem", a[0])
            scale[a[0] % fam.P] = 0.0
            pl.set_prior(loc, scale)
        elif kind == "bad_df":         # ey_plan_set_prior_family: "a refused call leaves the prior it had"
            loc, scale, df = prior_arrays(fam, "student", a[0])
            df[a[0] % fam.P] = 0.0
            pl.set_prior_family(L.EY_PRIOR_STUDENT_T, loc, scale, df)
        elif kind == "bad_cols":       # Plan.set_data checks the shape before ey_plan_set_data
            x, y = data_arrays(fam, cfg.n, a[0], cols=fam.dims[0] + 1)
            pl.set_data(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV))
        elif kind == "bad_theta_dtype":   # Plan._theta, the first line of every step
            other = torch.float32 if pl.dtype == torch.float64 else torch.float64
            pl.mh_step(torch.zeros(2, fam.P, dtype=other, device=DEV), torch.zeros(2, dtype=other, device=DEV), MH_SCALE)
        elif kind == "bad_lik_scale":  # ey_plan_set_lik_scale validates before set_lik_constants
            pl.set_lik_scale(-1.0)
        elif kind == "bad_index":      # Plan._tril range-checks the index before the launch
            G, C = 2, 3
            big = torch.eye(fam.P, dtype=pl.dtype, device=DEV).repeat(G + 1, 1, 1)   # an unchecked G stays inside it
            index = torch.tensor([0, G, 1], dtype=torch.int32, device=DEV)
            pl.mh_tril_step(torch.zeros(C, fam.P, dtype=pl.dtype, device=DEV), torch.zeros(C, dtype=pl.dtype, device=DEV),
                            big[:G], index=index)
        else:
            raise KeyError(kind)
    except ValueError as e:
        if kind not in REFUSALS:
            raise
        raised = e
    lv.cfg = new
    return raised


# ------------------------------------------------------------------------------------------------ the script generator
def crossings(fam):
    """The row counts to visit, in order, so that every adjacent pair of the family's limits is crossed both ways."""
    return list(fam.ns[1:]) + list(fam.ns[-2::-1])


def script(name, seed=SEED):
    """The operations of the family's script: every kind of `kinds` at least once, every adjacent pair of its row counts
    crossed in both directions, each operation legal behind the ones before it.  Ordered sub-sequences (the walk over the
    row counts; attach before detach; the other prior families, then back to Normal) are interleaved at random; a script
    shorter than SCRIPT_LEN is filled up with operations drawn among the legal ones.  The runner probes after EVERY
    operation, so every refused call is followed by a probe."""
    fam = FAMILY[name]
    rng = np.random.default_rng([seed, FAMILY_LIST.index(fam)])
    ks = kinds(fam)
    chains = [[("data_n", n) for n in crossings(fam)]] if fam.kind == "mlp" else []
    paired = {"attach_moments", "detach_moments", "attach_da", "detach_da", "prior_elem"} | {"prior_" + k for k in FAMILY_PRIORS}
    chains.append(["attach_moments", "detach_moments"])
    if "attach_da" in ks:
        chains.append(["attach_da", "detach_da"])
    if "prior_laplace" in ks:
        chains.append(["prior_" + k for k in rng.permutation(FAMILY_PRIORS)] + ["prior_elem"])
    elif "prior_elem" in ks:
        chains.append(["prior_elem"])
    chains += [[k] for k in ks if k not in paired]
    cfg, ops = start(fam), []

    def head(ch):
        h = ch[0]
        return ("data_n", h[1], int(rng.integers(1, 1 << 20))) if isinstance(h, tuple) else draw(cfg, h, rng)

    while any(chains):
        live = [ch for ch in chains if ch]
        ready = []
        for ch in live:
            kind = ch[0][0] if isinstance(ch[0], tuple) else ch[0]
            probe_op = ("data_n", ch[0][1], 0) if kind == "data_n" else (kind,)
            if legal(cfg, probe_op):
                ready.append(ch)
        w = np.array([len(ch) for ch in ready], dtype=np.float64)
        ch = ready[int(rng.choice(len(ready), p=w / w.sum()))]
        op = head(ch)
        ch.pop(0)
        ops.append(op)
        cfg = after(cfg, op)
    pool = ks + (["data_n"] if fam.kind == "mlp" else [])
    while len(ops) < SCRIPT_LEN:
        kind = pool[int(rng.integers(len(pool)))]
        if not legal(cfg, (kind, -1)):
            continue
        op = draw(cfg, kind, rng)
        ops.append(op)
        cfg = after(cfg, op)
    return ops


# --------------------------------------------------------------------------------------------------------- the probe
def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def first_difference(a, b):
    """The name of the first output of two probes that differs in name, shape, dtype or bits (NaN equals NaN), or None."""
    for (na, ta), (nb, tb) in itertools.zip_longest(a, b, fillvalue=("missing", None)):
        if na != nb or ta is None or tb is None:
            return f"{na} / {nb}"
        if isinstance(ta, str):
            if ta != tb:
                return f"{na}: {ta} / {tb}"
        elif ta.dtype != tb.dtype or ta.shape != tb.shape or not torch.equal(_bits(ta), _bits(tb)):
            return na
    return None


def probe_chains(cfg, k):
    att = cfg.da[0] if cfg.da is not None else cfg.moments
    return att if att is not None else CHAINS[k % len(CHAINS)]


def probe_hmc_iters(cfg, k):
    """HMC draws of probe number k on the plan's own HMC kernels (what an attached dual averaging counts)."""
    return 1 + (RUN_ITERS if k % RUN_EVERY == 0 else 0)


def _records(pl, C, n):
    return dict(samples=pl.empty(n, C, pl.P), targets=pl.empty(n, C), accepted_rec=pl.empty(n, C, dtype=torch.uint8),
                accept_count=torch.zeros(C, dtype=torch.int32, device=DEV))


def probe(lv, k):
    """Probe number k of the plan: a list of (name, tensor) (and ('kernel', name)).  Every sampler starts from clones of
    one state, on the in-kernel Philox streams keyed by k; attached accumulators are zeroed first and returned last."""
    pl, fam, cfg = lv.plan, lv.fam, lv.cfg
    C, P, dt = probe_chains(cfg, k), pl.P, pl.dtype
    rng = np.random.default_rng([SEED, 6, k])
    width = max(fam.dims) if fam.kind == "mlp" else 4
    th0 = torch.tensor(0.5 / np.sqrt(width) * rng.standard_normal((C, P)), dtype=dt, device=DEV)
    temp = torch.linspace(1.0, 0.4, C, dtype=dt, device=DEV) if C > 1 else torch.full((1,), 0.7, dtype=dt, device=DEV)
    key = dict(seed=1000 + k, it=k)
    run = k % RUN_EVERY == 0
    if lv.mom is not None:
        for t in lv.mom:
            t.zero_()
    out = [("kernel", pl.kernel)]

    def add(name, state, res=None, rec=None):
        out.extend((f"{name}.{i}", t) for i, t in enumerate(state))
        out.extend((f"{name}.{n}", t) for n, t in sorted((res or {}).items()))
        out.extend((f"{name}.{n}", t) for n, t in sorted((rec or {}).items()))

    t0, g0 = pl.log_target_grad(th0)
    add("log_target_grad", (t0, g0))
    add("log_target_grad[temp]", pl.log_target_grad(th0, temp=temp))

    def state(grad=True):
        return (th0.clone(), t0.clone(), g0.clone()) if grad else (th0.clone(), t0.clone())

    s = state()
    add("hmc_step", s, pl.hmc_step(*s, STEP, LSTEPS, temp=temp, **key))
    s = state()
    add("mala_step", s, pl.mala_step(*s, MALA_STEP, temp=temp, **key))
    s = state(False)
    add("mh_step", s, pl.mh_step(*s, MH_SCALE, temp=temp, **key))
    if run:
        s, rec = state(), _records(pl, C, RUN_ITERS)
        add("hmc_run", s, pl.hmc_run(*s, STEP, LSTEPS, RUN_ITERS, temp=temp, **key, **rec), rec)
        s, rec = state(), _records(pl, C, RUN_ITERS)
        add("mala_run", s, pl.mala_run(*s, MALA_STEP, RUN_ITERS, temp=temp, **key, **rec), rec)
        s, rec = state(False), _records(pl, C, RUN_ITERS)
        add("mh_run", s, pl.mh_run(*s, MH_SCALE, RUN_ITERS, temp=temp, **key, **rec), rec)

    if fam.kind != "mlp":   # the samplers with a factor: one for all chains, one per chain, indexed (a new index tensor)
        G = 2
        tril = torch.tensor(0.1 * np.tril(rng.standard_normal((max(C, G), P, P))) + 0.3 * np.eye(P), dtype=dt, device=DEV)
        diag = torch.tensor(0.2 + rng.random((max(C, G), P)), dtype=dt, device=DEV)
        index = torch.tensor((np.arange(C) + k) % G, dtype=torch.int32, device=DEV)
        forms = (("shared", tril[0].contiguous(), diag[0].contiguous(), None),
                 ("per-chain", tril[:C].contiguous(), diag[:C].contiguous(), None),
                 ("indexed", tril[:G].contiguous(), diag[:G].contiguous(), index))
        for tag, tr, dg, ix in forms:
            s = state(False)
            add(f"mh_tril_step[{tag}]", s, pl.mh_tril_step(*s, tr, index=ix, temp=temp, **key))
            s = state()
            add(f"mala_tril_step[{tag}]", s, pl.mala_tril_step(*s, MALA_STEP, tr, index=ix, temp=temp, **key))
            for form, m in (("dense", tr), ("diag", dg)):
                s = state()
                add(f"hmc_metric_step[{form},{tag}]", s,
                    pl.hmc_metric_step(*s, STEP, LSTEPS, m, form, index=ix, temp=temp, **key))
            if run:
                s, rec = state(False), _records(pl, C, RUN_ITERS)
                add(f"mh_tril_run[{tag}]", s, pl.mh_tril_run(*s, tr, RUN_ITERS, index=ix, temp=temp, **key, **rec), rec)
                s, rec = state(), _records(pl, C, RUN_ITERS)
                add(f"mala_tril_run[{tag}]", s,
                    pl.mala_tril_run(*s, MALA_STEP, tr, RUN_ITERS, index=ix, temp=temp, **key, **rec), rec)
                for form, m in (("dense", tr), ("diag", dg)):
                    s, rec = state(), _records(pl, C, RUN_ITERS)
                    add(f"hmc_metric_run[{form},{tag}]", s,
                        pl.hmc_metric_run(*s, STEP, LSTEPS, m, form, RUN_ITERS, index=ix, temp=temp, **key, **rec), rec)
    if lv.mom is not None:
        add("moments", lv.mom)
    if lv.da is not None:
        add("dual_averaging", lv.da[:2])
    return out
