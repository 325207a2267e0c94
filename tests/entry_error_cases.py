"""The error surface of the 18 sampler entry points ey_{hmc,mala,mh,ram,mh_tril,mala_tril,am,am_softabs,gibbs}_{step,run}
and of the Plan methods over them, as one table of calls that validation refuses before any launch (or, with C == 0,
answers OK on null buffers).

tests/golden/make_golden_entry_errors.py runs the table and records what each call answers; tests/test_entry_errors_gpu.py
runs it again and compares.  Nothing here says what a call must answer: the record does.  A case is a set of changes
to a call that would otherwise be served; the checks of an entry point are listed in the order the library makes them,
and every two neighbours of that list are also violated together (which of the two errors wins is part of the surface).
Only pointers the validation covers are passed: every optional buffer is null.

Two refusals need what one small plan on one device cannot give and have no case: a Gibbs table built on another device
(a second GPU) and a Gibbs table whose LDS image does not fit (a large model).
"""
import json
import os
import types
from collections import namedtuple

import torch

from eeyore_amd import _lib as L

NAN, INF = float("nan"), float("inf")
_DRAW = "temp C seed iter chain_offset flags"
_RECS = "n_iters samples targets accepted_rec accept_count accepted"
_REC = _RECS + " stream"
_AM = "running_mean cov_sum cov num_accepted cov0 cov0_per_chain l b c eps t0 idx offset"
ARGS = {k: v.split() for k, v in {
    "ey_hmc_step": f"pl theta target grad p0 u step step_vec L {_DRAW} accepted accept_rate H_cur H_prop stream",
    "ey_hmc_run": f"pl theta target grad step step_vec L {_DRAW} {_REC}",
    "ey_mala_step": f"pl theta target grad z u step step_vec {_DRAW} accepted log_rate stream",
    "ey_mala_run": f"pl theta target grad step step_vec {_DRAW} {_REC}",
    "ey_mh_step": f"pl theta target z u scale {_DRAW} accepted log_rate stream",
    "ey_mh_run": f"pl theta target scale {_DRAW} {_REC}",
    "ey_ram_step": f"pl theta target chol z u a g n {_DRAW} accepted log_rate stream",
    "ey_ram_run": f"pl theta target chol a g n {_DRAW} {_REC}",
    "ey_mh_tril_step": f"pl theta target tril G tril_index z u {_DRAW} accepted log_rate stream",
    "ey_mh_tril_run": f"pl theta target tril G tril_index {_DRAW} {_REC}",
    "ey_mala_tril_step": f"pl theta target grad tril G tril_index z u step step_vec {_DRAW} accepted log_rate stream",
    "ey_mala_tril_run": f"pl theta target grad tril G tril_index step step_vec {_DRAW} {_REC}",
    "ey_am_step": f"pl theta target {_AM} z u_mix u {_DRAW} accepted log_rate branch breakdowns stream",
    "ey_am_run": f"pl theta target {_AM} {_DRAW} {_RECS} breakdowns stream",
    "ey_am_softabs_step": f"pl theta target {_AM} z u_mix u {_DRAW} accepted log_rate branch breakdowns stream",
    "ey_am_softabs_run": f"pl theta target {_AM} {_DRAW} {_RECS} breakdowns stream",
    "ey_gibbs_step": f"pl tb theta target z u {_DRAW} accepted log_rate stream",
    "ey_gibbs_run": f"pl tb theta target {_DRAW} {_REC}",
}.items()}
ENTRIES = list(ARGS)
# the buffers a served call needs (the validation refuses each of them when null); everything else is optional and null
BUFFERS = ("theta", "target", "grad", "scale", "chol", "tril", "running_mean", "cov_sum", "cov", "num_accepted", "cov0",
           "breakdowns", "accepted")
SCALARS = dict(step=0.1, L=2, seed=1, iter=1, chain_offset=0, flags=0, n_iters=1, a=0.234, g=0.7, n=1, G=1, cov0_per_chain=0,
               l=0.05, b=1.0, c=1.0, eps=0.5, t0=2, idx=5, offset=0)
WORLDS = ("f32", "f64", "large")  # "large": the MLP(10-200-2) f64 plan under a Laplace prior, refused and never launched

Case = namedtuple("Case", "name mut worlds")


def _checks(entry):
    """[(check, [variant, ...])] in the order the library makes the checks of ``entry``; a variant is (name, changes).
    Changes: ``pl`` names a plan of the world (None: null), ``moments`` / ``da`` attach accumulators or dual averaging
    sized for the call's chains ("same") or for one chain more ("other"), a buffer name maps to None (null) or to the
    name of another tensor of the world, a scalar name to its value."""
    sampler, run = entry[3:].rsplit("_", 1)
    run = run == "run"
    required = [n for n in ARGS[entry] if n in BUFFERS]
    null = ("null", [(f"null_{n}", {n: None}) for n in required])
    n_iters = ("n_iters", [("n_iters_0", {"n_iters": 0}), ("n_iters_negative", {"n_iters": -2})])
    c0 = ("c0", [("c0_null_buffers", dict({n: None for n in required}, C=0))])
    moments = ("moments", [("moments_other_c", {"moments": "other"})])
    replay = ("replay", [("replay_no_samples", {"moments": "same", "n_iters": 2, "accepted_rec": "accepted_rec2"}),
                         ("replay_no_accepted_rec", {"moments": "same", "n_iters": 2, "samples": "samples2"})])
    step = ("step", [("step_0", {"step": 0.0}), ("step_negative", {"step": -0.1}), ("step_nan", {"step": NAN})])
    tril = [("G", [("G_0", {"G": 0})]), ("G_pair", [("G_2_no_index", {"G": 2})])]
    ready = [("null_plan", [("null_plan", {"pl": None})]), ("no_data", [("no_data", {"pl": "nodata"})]),
             ("no_prior", [("no_prior", {"pl": "noprior"})]), ("prior_fits", [("laplace_large", {"pl": "ok@large"})]),
             ("c_range", [("c_negative", {"C": -1}), ("c_beyond_int32", {"C": 2 ** 31})])]
    if sampler == "gibbs":  # its own order: the table before the C == 0 answer, the buffers after it
        out = [("mixture", [("mixture_plan", {"pl": "mix"})])] + ready
        out.append(("null_table", [("null_table", {"tb": None})]))
        out.append(("table", [("table_other_p", {"tb": "tb_other_p"}), ("table_other_dtype", {"tb": "tb_other_dtype"})]))
        out += [n_iters] * run
        out += [c0, null, moments]
        if run:
            out.append(("replay", [("replay_no_samples", {"moments": "same", "n_iters": 2})]))
        return out
    out = ready + [c0, null]  # an empty batch is answered as soon as the plan and the chain count are known
    if sampler == "hmc":
        out.append(("L", [("L_0", {"L": 0})]))
    if sampler in ("mala", "mala_tril"):
        out.append(step)
    out += [n_iters] * run
    if sampler == "ram":
        out += [("n", [("n_0", {"n": 0})]), ("a", [("a_0", {"a": 0.0}), ("a_1", {"a": 1.0}), ("a_nan", {"a": NAN})]),
                ("g", [("g_inf", {"g": INF}), ("g_nan", {"g": NAN})])]
    if sampler in ("mh_tril", "mala_tril"):
        out += tril
    if sampler in ("am", "am_softabs"):
        eps = ([("a_0", {"eps": 0.0}), ("a_negative", {"eps": -1.0}), ("a_inf", {"eps": INF})] if sampler == "am_softabs"
               else [("eps_negative", {"eps": -1e-3}), ("eps_nan", {"eps": NAN})])
        out += [("t0", [("t0_1", {"t0": 1})]),
                ("l", [("l_negative", {"l": -0.1}), ("l_above_1", {"l": 1.1}), ("l_nan", {"l": NAN})]),
                ("bc", [("b_inf", {"b": INF}), ("c_nan", {"c": NAN})]), ("eps", eps),
                ("idx", [("idx_negative", {"idx": -1}), ("idx_before_offset", {"idx": 3, "offset": 4})])]
    out.append(moments)
    if sampler == "hmc":
        out += [("da_c", [("da_other_c", {"da": "other"})]),
                ("da_fused", [("da_not_fused", {"da": "same", "flags": L.EY_FORCE_GENERIC})])]
    if run:
        out.append(replay)
    return out


def _merge(a, b):
    """The changes of two variants made together, or None where they cannot be (two plans, two tables)."""
    out = dict(a)
    for k, v in b.items():
        if k in out and out[k] != v:
            if k == "pl" and {out[k], v} == {"nodata", "noprior"}:
                v = "fresh"
            elif k in ("moments", "da"):  # sized for one chain more: the earlier of the two checks fails
                v = "other"
            else:
                return None
        out[k] = v
    return out


def _worlds(mut):
    return ("large",) if mut.get("pl") == "ok@large" else ("f32", "f64")


def c_cases(entry):
    """Every variant of every check of ``entry`` alone, then the first variants of every two neighbouring checks together,
    then the C == 0 call together with the first variant of every check that follows it."""
    checks = _checks(entry)
    cases = [Case(name, mut, _worlds(mut)) for _, variants in checks for name, mut in variants]
    first = [variants[0] for _, variants in checks]
    at0 = [n for n, _ in checks].index("c0")
    rest = first[:at0] + first[at0 + 1:]  # the neighbours of a call that has chains
    pairs = list(zip(first, first[1:])) + [(first[at0], later) for later in first[at0 + 2:]] + list(zip(rest, rest[1:]))
    for (na, ma), (nb, mb) in pairs:
        m = _merge(ma, mb)
        if m is not None and m != ma and m != mb and f"{na}+{nb}" not in [c.name for c in cases]:
            cases.append(Case(f"{na}+{nb}", m, _worlds(m)))
    return cases


# ---------------------------------------------------------------------------------------------------------- the worlds
class World:
    """The plans and the buffers the cases of one dtype are made of (MLP(2-2-1), sigmoid, BCE, 4 rows, 3 chains; for
    "large" MLP(10-200-2) f64 under a Laplace prior, 1 chain)."""

    def __init__(self, name, device):
        from eeyore_amd.plan import GibbsTable, Plan
        self.name, self.dev = name, torch.device(device)
        self.dtype = dt = torch.float32 if name == "f32" else torch.float64
        large = name == "large"
        dims, acts, lik = ([10, 200, 2], [1, 0], 1) if large else ([2, 2, 1], [1, 1], 0)
        self.C = C = 1 if large else 3
        g = torch.Generator().manual_seed(5)
        x = torch.randn(4, dims[0], generator=g, dtype=torch.float64)
        y = torch.eye(2, dtype=torch.float64)[[0, 1, 1, 0]] if large else torch.tensor([[0.], [1.], [1.], [0.]], dtype=torch.float64)

        def plan(data, prior):
            pl = Plan(dims, [1, 1], acts, lik, dt, self.dev)
            if data:
                pl.set_data(x.to(dt).to(self.dev), y.to(dt).to(self.dev))
            if prior:
                pl.set_prior(torch.zeros(pl.P), torch.ones(pl.P))
            return pl

        self.plans = {"ok": plan(True, True)}
        self.P = P = self.plans["ok"].P
        if large:
            self.plans["ok"].set_prior_family(L.EY_PRIOR_LAPLACE, torch.zeros(P), torch.ones(P))
        else:
            self.plans.update(nodata=plan(False, True), noprior=plan(True, False), fresh=plan(False, False))
            self.plans["mix"] = Plan.mixture([0.0, -0.5], [[0.0] * P, [0.5] * P], [torch.eye(P).tolist()] * 2, dt, self.dev)
        S = self.S = 3
        other = torch.float64 if dt == torch.float32 else torch.float32
        self.tables = {"tb": GibbsTable(self.plans["ok"], [list(range(i, P, S)) for i in range(S)], [0.1] * S)}
        if not large:
            ns = types.SimpleNamespace
            self.tables["tb_other_p"] = GibbsTable(ns(P=P - 1, dtype=dt, device=self.dev), [[0, 1], [2, 3]], [0.1, 0.2])
            self.tables["tb_other_dtype"] = GibbsTable(ns(P=P, dtype=other, device=self.dev), [[0, 1], [2, 3]], [0.1, 0.2])

        def t(*shape, dtype=dt, fill=None):
            if fill is not None:
                return torch.full(shape, fill, dtype=dtype, device=self.dev)
            return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).to(self.dev)

        eye = torch.eye(P, dtype=dt, device=self.dev)
        self.t = dict(
            theta=t(C, P), target=t(C), grad=t(C, P), scale=t(P, fill=0.1), chol=eye.repeat(C, 1, 1), tril=eye.clone(),
            running_mean=t(C, P), cov_sum=eye.repeat(C, 1, 1), cov=eye.repeat(C, 1, 1),
            num_accepted=t(C, dtype=torch.int32, fill=1), cov0=eye.clone(), breakdowns=t(C, dtype=torch.int32, fill=0),
            accepted=t(C, S, dtype=torch.uint8, fill=7), samples2=t(2, C, P, fill=0.25),
            accepted_rec2=t(2, C, S, dtype=torch.uint8, fill=9))
        f64 = torch.float64
        self.moments = {k: (t(c, P, dtype=f64, fill=0.5), t(c, P, dtype=f64, fill=1.5), t(c, dtype=f64, fill=2.5), c)
                        for k, c in (("same", C), ("other", C + 1))}
        self.da = {k: (t(c, 3, dtype=f64, fill=0.0), t(c, fill=0.1), t(4, 3, dtype=f64, fill=0.5), c)
                   for k, c in (("same", C), ("other", C + 1))}
        self.state = dict(self.t)
        for kind, sets in (("moments", self.moments), ("da", self.da)):
            for k, v in sets.items():
                self.state.update({f"{kind}_{k}_{i}": x for i, x in enumerate(v[:3])})
        torch.cuda.synchronize(self.dev)
        self.before = {k: v.clone() for k, v in self.state.items()}

    def changed(self):
        """Names of the buffers that no longer hold the bytes they were made with."""
        return [k for k, v in self.state.items() if not torch.equal(v, self.before[k])]

    def attach(self, pl, mut):
        lib = L.lib()
        if "moments" in mut:
            s1, s2, acc, c = self.moments[mut["moments"]]
            assert lib.ey_plan_attach_moments(pl.handle, L.ptr(s1), L.ptr(s2), L.ptr(acc), c) == 0
        if "da" in mut:
            st, sv, tab, c = self.da[mut["da"]]
            assert lib.ey_plan_attach_da(pl.handle, L.ptr(st), L.ptr(sv), L.ptr(tab), 4, c, 0.65, NAN, 1) == 0

    def detach(self, pl):
        lib = L.lib()
        assert lib.ey_plan_attach_moments(pl.handle, None, None, None, 0) == 0
        assert lib.ey_plan_attach_da(pl.handle, None, None, None, 0, 0, 0.5, NAN, 0) == 0


def c_args(entry, mut, world=None):
    """The ctypes arguments of ``entry`` under the changes ``mut``; without a world every pointer is null (the host-only
    null-plan call)."""
    args = []
    for name in ARGS[entry]:
        if name in mut:
            v = mut[name]
        elif name == "pl":
            v = "ok"
        elif name == "tb":
            v = "tb"
        elif name == "C":
            v = world.C if world else 3
        elif name in BUFFERS:
            v = name
        else:
            v = SCALARS.get(name)
        if isinstance(v, str):
            if world is None:
                v = None
            elif name == "pl":
                v = world.plans[v.split("@")[0]].handle
            elif name == "tb":
                v = world.tables[v].handle
            else:
                v = L.ptr(world.t[v])
        args.append(v)
    return args


def run_c(world, entry, case):
    """(status, message) of the C entry point on this case; the message of an OK call is ''."""
    lib = L.lib()
    name = case.mut.get("pl", "ok")
    pl = world.plans[name.split("@")[0]] if name else None
    if pl is not None:
        world.attach(pl, case.mut)
    try:
        rc = getattr(lib, entry)(*c_args(entry, case.mut, world))
        return rc, (lib.ey_last_error().decode() if rc else "")
    finally:
        if pl is not None:
            world.detach(pl)


def null_plan_call(entry):
    """(status, message) of ``entry`` on a null plan and null buffers: needs no device."""
    lib = L.lib()
    rc = getattr(lib, entry)(*c_args(entry, {"pl": None}))
    return rc, lib.ey_last_error().decode()


# ------------------------------------------------------------------------------------------------- through Plan
PLAN_METHODS = ["hmc_step", "hmc_run", "mala_step", "mala_run", "mh_step", "mh_run", "mh_tril_step", "mh_tril_run",
                "mala_tril_step", "mala_tril_run", "ram_step", "ram_run", "gibbs_step", "gibbs_run", "am_step", "am_run"]
_PLAN_BASE = {
    "hmc": dict(theta="theta", target="target", grad="grad", step=0.1, num_steps=2),
    "mala": dict(theta="theta", target="target", grad="grad", step=0.1),
    "mh": dict(theta="theta", target="target", scale=0.1),
    "mh_tril": dict(theta="theta", target="target", tril="tril"),
    "mala_tril": dict(theta="theta", target="target", grad="grad", step=0.1, tril="tril"),
    "ram": dict(theta="theta", target="target", chol="chol", n=1),
    "gibbs": dict(theta="theta", target="target", table="tb"),
    "am": dict(theta="theta", target="target", running_mean="running_mean", cov_sum="cov_sum", cov="cov",
               num_accepted="num_accepted", cov0="cov0", idx=5, breakdowns="breakdowns"),
}


def _bad(kind, base):
    """A tensor like the world's ``base`` but wrong in one way; resolved against the world when the case runs."""
    return ("bad", kind, base)


def plan_entries():
    """The 18 (entry, method, base keywords): am_step / am_run serve the softabs entry points with ``softabs_a``."""
    out = []
    for m in PLAN_METHODS:
        sampler, kind = m.rsplit("_", 1)
        base = dict(_PLAN_BASE[sampler], **({"n_iters": 1} if kind == "run" else {}))
        out.append((f"ey_{m}", m, base))
        if sampler == "am":
            out.append((f"ey_am_softabs_{kind}", m, dict(base, softabs_a=1.0)))
    return out


def plan_cases(entry):
    """[(check, [variant, ...])] of the ValueErrors Plan raises itself, in the order the method makes the checks, then the
    library's own refusal of n_iters = 0 (through L.check); singles and neighbouring pairs as for the C entry points."""
    sampler, run = entry[3:].rsplit("_", 1)
    run = run == "run"
    S = 3
    theta = ("theta", [("theta_dtype", {"theta": _bad("dtype", "theta")}), ("theta_shape", {"theta": _bad("shape", "theta")}),
                       ("theta_strided", {"theta": _bad("strided", "theta")}), ("theta_cpu", {"theta": _bad("cpu", "theta")})])
    checks = [theta]
    if sampler in ("mh_tril", "mala_tril"):
        checks += [("tril", [("tril_shape", {"tril": _bad("shape", "tril")}), ("tril_dtype", {"tril": _bad("dtype", "tril")}),
                             ("tril_list", {"tril": [[1.0]]}), ("tril_cpu", {"tril": _bad("cpu", "tril")})]),
                   ("tril_G", [("tril_2_factors", {"tril": ("tril_g", 2)})]),
                   ("index", [("index_int64", {"tril": ("tril_g", 2), "index": ("index", torch.int64, [0, 1, 0])}),
                              ("index_short", {"tril": ("tril_g", 2), "index": ("index", torch.int32, [0, 1])}),
                              ("index_range", {"tril": ("tril_g", 2), "index": ("index", torch.int32, [0, 1, 2])}),
                              ("index_negative", {"tril": ("tril_g", 2), "index": ("index", torch.int32, [0, -1, 1])})])]
    if sampler == "ram":
        checks.append(("chol", [("chol_shape", {"chol": "tril"}), ("chol_dtype", {"chol": _bad("dtype", "chol")}),
                                ("chol_strided", {"chol": _bad("strided", "chol")})]))
    if sampler == "gibbs":
        checks += [("table", [("table_not_a_table", {"table": 3})]), ("mode", [("mode_unknown", {"mode": "carry"})])]
        if not run:
            checks += [("z", [("z_shape", {"z": "target"}), ("z_dtype", {"z": _bad("dtype", "theta")})]),
                       ("u", [("u_shape", {"u": "target"}), ("u_cpu", {"u": ("zeros", (3, S), None, "cpu")})])]
    if sampler in ("am", "am_softabs"):
        checks.append(("am_state", [("running_mean_shape", {"running_mean": "target"}),
                                    ("cov_sum_dtype", {"cov_sum": _bad("dtype", "cov_sum")}),
                                    ("cov_strided", {"cov": _bad("strided", "cov")}),
                                    ("num_accepted_int64", {"num_accepted": ("zeros", (3,), torch.int64, None)}),
                                    ("breakdowns_shape", {"breakdowns": ("zeros", (4,), torch.int32, None)}),
                                    ("cov0_shape", {"cov0": "theta"}), ("cov0_dtype", {"cov0": _bad("dtype", "cov0")})]))
    if run:
        rec = (3, S) if sampler == "gibbs" else (3,)
        checks.append(("records", [("samples_shape", {"samples": ("zeros", (2, 3, 9), None, None)}),
                                   ("targets_dtype", {"targets": ("zeros", (1, 3), torch.int32, None)}),
                                   ("samples_cpu", {"samples": ("zeros", (1, 3, 9), None, "cpu")}),
                                   ("accepted_rec_shape", {"accepted_rec": ("zeros", (1, 4), torch.uint8, None)}),
                                   ("accepted_rec_dtype", {"accepted_rec": ("zeros", (1,) + rec, torch.int32, None)}),
                                   ("accept_count_int64", {"accept_count": ("zeros", rec, torch.int64, None)}),
                                   ("accept_count_shape", {"accept_count": ("zeros", (5,), torch.int32, None)})]))
    if sampler == "gibbs":
        checks.append(("table_other", [("table_other_p", {"table": "tb_other_p"})]))
    if sampler == "hmc":
        checks.append(("L", [("num_steps_0", {"num_steps": 0})]))
    if sampler in ("mala", "mala_tril"):
        checks.append(("step", [("step_0", {"step": 0.0})]))
    if run:
        checks.append(("n_iters", [("n_iters_0", {"n_iters": 0})]))
    checks.append(("moments", [("moments_other_c", {"moments": "other"})]))
    cases = [Case(n, m, ("f32", "f64")) for _, vs in checks for n, m in vs]
    for (_, va), (_, vb) in zip(checks, checks[1:]):
        (na, ma), (nb, mb) = va[0], vb[0]
        if not set(ma) & set(mb):
            cases.append(Case(f"{na}+{nb}", dict(ma, **mb), ("f32", "f64")))
    return cases


def _resolve(world, v):
    dt, dev = world.dtype, world.dev
    other = torch.float64 if dt == torch.float32 else torch.float32
    if isinstance(v, str):  # the name of a table or a buffer of the world; any other string is the value itself
        return world.tables.get(v, world.t.get(v, v))
    if isinstance(v, tuple) and v[0] == "bad":
        base = world.t[v[2]]
        if v[1] == "dtype":
            return base.to(other)
        if v[1] == "shape":
            return torch.zeros(tuple(base.shape[:-1]) + (base.shape[-1] + 1,), dtype=dt, device=dev)
        if v[1] == "strided":
            return torch.zeros(tuple(base.shape[:-1]) + (2 * base.shape[-1],), dtype=dt, device=dev)[..., ::2]
        if v[1] == "cpu":
            return base.cpu()
    if isinstance(v, tuple) and v[0] == "zeros":
        return torch.zeros(v[1], dtype=v[2] or dt, device=v[3] or dev)
    if isinstance(v, tuple) and v[0] == "tril_g":
        return torch.eye(world.P, dtype=dt, device=dev).repeat(v[1], 1, 1)
    if isinstance(v, tuple) and v[0] == "index":
        return torch.tensor(v[2], dtype=v[1], device=dev)
    return v


def run_plan(world, method, base, case):
    """(exception type name, text) of the Plan method on this case; ('', '') when it returned (no case is meant to)."""
    pl = world.plans["ok"]
    kw = {k: _resolve(world, v) for k, v in dict(base, **{k: v for k, v in case.mut.items() if k != "moments"}).items()}
    world.attach(pl, case.mut)
    try:
        getattr(pl, method)(**kw)
        return "", ""
    except (ValueError, RuntimeError, TypeError) as e:
        return type(e).__name__, str(e)
    finally:
        world.detach(pl)


def record_key(level, entry, world, case):
    return f"{level}:{entry}:{world}:{case}"


# ------------------------------------------------------------------------------------------------- the record on disk
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_entry_errors.json")
_ANSWER = {"c": ("status", "message"), "plan": ("exception", "text")}


def symbol_text(entry):
    """A _lib.SYMBOLS entry by the names of its ctypes types: ``restype(argtype, ...)``."""
    res, args = entry
    return f"{res.__name__}({', '.join(t.__name__ for t in args)})"


def dump_record(rec, path):
    """Write ``rec`` (signatures, docs, symbols, cases = {record_key: answer}) one item per line, with the cases that
    answer alike but for the entry point's own name (``{who}``) written once: level, case, the answer, the worlds and the
    entry points it holds for."""
    groups = {}
    for key, v in rec["cases"].items():
        level, entry, world, case = key.split(":", 3)
        code, text = (v[k] for k in _ANSWER[level])
        groups.setdefault((level, case, code, text.replace(entry, "{who}")), {}).setdefault(entry, []).append(world)
    lines = []
    for (level, case, code, text), by_entry in sorted(groups.items(), key=lambda kv: kv[0][:2] + (str(kv[0][2]), kv[0][3])):
        by_worlds = {}
        for entry, worlds in by_entry.items():
            by_worlds.setdefault(",".join(sorted(worlds)), []).append(entry)
        for worlds, entries in sorted(by_worlds.items()):
            lines.append(json.dumps([level, case, code, text, worlds, sorted(entries)]))
    with open(path, "w") as f:
        f.write("{\n")
        for name in ("signatures", "docs", "symbols"):
            items = ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(rec[name].items()))
            f.write(f"{json.dumps(name)}: {{\n{items}\n}},\n")
        f.write('"cases": [\n' + ",\n".join(lines) + "\n]\n}\n")


def load_record(path=GOLDEN):
    """The record as ``dump_record`` was given it: cases = {record_key: {status, message} or {exception, text}}."""
    with open(path) as f:
        rec = json.load(f)
    cases = {}
    for level, case, code, text, worlds, entries in rec["cases"]:
        for entry in entries:
            for world in worlds.split(","):
                cases[record_key(level, entry, world, case)] = dict(zip(_ANSWER[level], (code, text.replace("{who}", entry))))
    return dict(rec, cases=cases)
