"""Plan: the Python handle of a C-ABI ``ey_plan`` (include/eeyore_amd.h) operating on torch device tensors.

PyTorch is plumbing here (device memory, streams); all arithmetic of the hot path happens in the HIP library.
A plan fixes the model (dims/bias/activations/likelihood/dtype); data and prior are attached to it.
"""
import ctypes as ct

import torch

from . import _lib as L

_DT = {torch.float32: L.EY_F32, torch.float64: L.EY_F64}


def _stream(device):
    return ct.c_void_p(torch.cuda.current_stream(device).cuda_stream)


GIBBS_MODES = {'intended': 0, 'reference': L.EY_GIBBS_CARRY}


def gibbs_table_arrays(blocks, scales):
    """(blk_off [S+1] int32, blk_idx int32, blk_scale [S] double) as ctypes arrays from a list of index lists and one
    scale per list -- the host form ey_gibbs_table_create validates."""
    blocks = [[int(i) for i in b] for b in blocks]
    scales = [float(v) for v in scales]
    if len(scales) != len(blocks):
        raise ValueError(f"a Gibbs table needs one scale per block: {len(blocks)} blocks, {len(scales)} scales")
    off = [0]
    for b in blocks:
        off.append(off[-1] + len(b))
    flat = [i for b in blocks for i in b]
    return ((ct.c_int32 * len(off))(*off), (ct.c_int32 * max(len(flat), 1))(*flat),
            (ct.c_double * max(len(scales), 1))(*scales))


class GibbsTable:
    """Device copy of a Gibbs block table (ey_gibbs_table): built once per sampler, freed with the object."""

    def __init__(self, plan, blocks, scales):
        off, idx, scl = gibbs_table_arrays(blocks, scales)
        self.S = len(off) - 1
        self.blocks = [list(b) for b in blocks]
        self.handle = ct.c_void_p()
        L.check(L.lib().ey_gibbs_table_create(ct.byref(self.handle), plan.P, self.S, off, idx, scl, _DT[plan.dtype],
                                              plan.device.index), "ey_gibbs_table_create")

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                L.lib().ey_gibbs_table_destroy(self.handle)
                self.handle = ct.c_void_p()
        except Exception:
            pass


class PtLadder:
    """Device copy of a tempering ladder (ey_pt_ladder) for ``pt_between``: temperatures ``t`` [K] and partner weights
    ``q`` [K, K] (row i: the weights with which chain i proposes its partner, diagonal ignored), validated by the library
    on the host.  Built once per sampler, freed with the object."""

    def __init__(self, t, q, dtype, device):
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}")
        self.dtype, self.device = dtype, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        t = [float(v) for v in t]
        self.K = K = len(t)
        q = [[float(v) for v in row] for row in q]
        if len(q) != K or any(len(row) != K for row in q):
            raise ValueError(f"q must be [{K}, {K}], one row of partner weights per temperature")
        self.handle = ct.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().ey_pt_ladder_create((ct.c_double * K)(*t), (ct.c_double * (K * K))(*[v for row in q for v in row]),
                                                K, _DT[dtype], ct.byref(self.handle)), "ey_pt_ladder_create")

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                L.lib().ey_pt_ladder_destroy(self.handle)
                self.handle = ct.c_void_p()
        except Exception:
            pass


class Plan:
    def __init__(self, dims, bias, acts, likelihood, dtype, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(
                f"eeyore_amd: the hot path runs on an MI355X through the HIP library; device '{device}' is not a ROCm "
                "device and there is no CPU fallback")
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}")
        self.dtype = dtype
        self.dims = [int(d) for d in dims]
        n = len(self.dims) - 1
        self.handle = ct.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        L.check(L.lib().ey_plan_create(ct.byref(self.handle), n, (ct.c_int * (n + 1))(*self.dims),
                                       (ct.c_int * n)(*[int(b) for b in bias]), (ct.c_int * n)(*[int(a) for a in acts]),
                                       int(likelihood), _DT[dtype], idx), "ey_plan_create")
        P = ct.c_int64()
        L.check(L.lib().ey_plan_num_params(self.handle, ct.byref(P)), "ey_plan_num_params")
        self.P = P.value
        self._data_key, self._data_ref = None, (None, None)
        self._prior_key = None
        self._moments = None
        self._da_refs = None  # tensors an attached dual averaging points into: alive for as long as it is attached

    @classmethod
    def mixture(cls, c, mean, prec, dtype, device):
        """The plan of a Gaussian-mixture target on theta itself (ey_plan_create_mixture): ``c`` [M], ``mean`` [M, P] and
        ``prec`` [M, P, P] are host arrays of doubles, validated by the library before anything touches the device.  Data
        and prior are "set" from birth; ``kernel`` is 'dist'."""
        import numpy as np
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(
                f"eeyore_amd: the hot path runs on an MI355X through the HIP library; device '{device}' is not a ROCm "
                "device and there is no CPU fallback")
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}")
        c, mean, prec = (np.ascontiguousarray(a, dtype=np.float64) for a in (c, mean, prec))
        if c.ndim != 1 or mean.ndim != 2 or mean.shape[0] != c.shape[0] or prec.shape != mean.shape + mean.shape[1:]:
            raise ValueError(f"expected c [M], mean [M, P] and prec [M, P, P], got {c.shape}, {mean.shape}, {prec.shape}")
        self = cls.__new__(cls)
        self.dtype = dtype
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.dims = None
        self.handle = ct.c_void_p()
        dp = ct.POINTER(ct.c_double)
        L.check(L.lib().ey_plan_create_mixture(ct.byref(self.handle), mean.shape[1], c.shape[0], c.ctypes.data_as(dp),
                                               mean.ctypes.data_as(dp), prec.ctypes.data_as(dp), _DT[dtype], idx),
                "ey_plan_create_mixture")
        P = ct.c_int64()
        L.check(L.lib().ey_plan_num_params(self.handle, ct.byref(P)), "ey_plan_num_params")
        self.P, self.M = P.value, int(c.shape[0])
        self._data_key, self._data_ref = None, (None, None)
        self._prior_key = None
        self._moments = None
        self._da_refs = None
        return self

    @classmethod
    def exp_tilt(cls, c, a, b, s, dtype, device):
        """The plan of a separable exponential-tilt target on theta itself (ey_plan_create_exptilt):
        log p = sum_i [c_i + a_i theta_i - b_i exp(s_i theta_i)].  ``c``, ``a``, ``b``, ``s`` [P] are host arrays of doubles,
        validated by the library before anything touches the device.  Data and prior are "set" from birth; ``kernel`` is
        'dist'."""
        import numpy as np
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(
                f"eeyore_amd: the hot path runs on an MI355X through the HIP library; device '{device}' is not a ROCm "
                "device and there is no CPU fallback")
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}")
        c, a, b, s = (np.ascontiguousarray(t, dtype=np.float64) for t in (c, a, b, s))
        if c.ndim != 1 or a.shape != c.shape or b.shape != c.shape or s.shape != c.shape:
            raise ValueError(f"expected c, a, b and s of one shape [P], got {c.shape}, {a.shape}, {b.shape}, {s.shape}")
        self = cls.__new__(cls)
        self.dtype = dtype
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.dims = None
        self.handle = ct.c_void_p()
        dp = ct.POINTER(ct.c_double)
        L.check(L.lib().ey_plan_create_exptilt(ct.byref(self.handle), c.shape[0], c.ctypes.data_as(dp), a.ctypes.data_as(dp),
                                               b.ctypes.data_as(dp), s.ctypes.data_as(dp), _DT[dtype], idx),
                "ey_plan_create_exptilt")
        P = ct.c_int64()
        L.check(L.lib().ey_plan_num_params(self.handle, ct.byref(P)), "ey_plan_num_params")
        self.P = P.value
        self._data_key, self._data_ref = None, (None, None)
        self._prior_key = None
        self._moments = None
        self._da_refs = None
        return self

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                L.lib().ey_plan_destroy(self.handle)
                self.handle = ct.c_void_p()
        except Exception:
            pass

    @property
    def kernel(self):
        return L.lib().ey_plan_kernel(self.handle).decode()

    @property
    def f32_products(self):
        """'bf16x3' or 'exact': how the fused f32 trajectory kernel forms its 32x32x32 products (EY_OPT_F32_PRODUCTS in
        include/eeyore_amd.h); only plans that kernel serves are affected."""
        v = ct.c_int()
        L.check(L.lib().ey_plan_get_option(self.handle, L.EY_OPT_F32_PRODUCTS, ct.byref(v)), "ey_plan_get_option")
        return "exact" if v.value == L.EY_PRODUCTS_EXACT else "bf16x3"

    @f32_products.setter
    def f32_products(self, mode):
        if mode not in ("bf16x3", "exact"):
            raise ValueError("f32_products must be 'bf16x3' or 'exact'")
        L.check(L.lib().ey_plan_set_option(self.handle, L.EY_OPT_F32_PRODUCTS,
                                           L.EY_PRODUCTS_EXACT if mode == "exact" else L.EY_PRODUCTS_BF16X3),
                "ey_plan_set_option")

    @property
    def row_waves(self):
        """'off', 'on' or 'auto': several waves per chain for tiny models on batches of two row tiles or more
        (EY_OPT_ROW_WAVES in include/eeyore_amd.h: a latency option that changes the order of the gradient sums).  'off' is
        the default: a chain's bits then do not depend on how many chains share its launch; 'auto' opts in to the waves
        whenever the launch would leave the chip idle."""
        v = ct.c_int()
        L.check(L.lib().ey_plan_get_option(self.handle, L.EY_OPT_ROW_WAVES, ct.byref(v)), "ey_plan_get_option")
        return ("off", "on", "auto")[v.value]

    @row_waves.setter
    def row_waves(self, mode):
        if mode not in ("off", "on", "auto"):
            raise ValueError("row_waves must be 'off', 'on' or 'auto'")
        L.check(L.lib().ey_plan_set_option(self.handle, L.EY_OPT_ROW_WAVES, ("off", "on", "auto").index(mode)),
                "ey_plan_set_option")

    @property
    def max_chunk_chains(self):
        """Most chains the layerwise path ('bgemm') runs in one set of launches (EY_OPT_MAX_CHUNK_CHAINS in
        include/eeyore_amd.h); 0, the default, leaves it to the path's own rule (16 GiB of activations, 32768 chains).  A
        positive value bounds the activation scratch by that many chains'; the results do not depend on it."""
        v = ct.c_int()
        L.check(L.lib().ey_plan_get_option(self.handle, L.EY_OPT_MAX_CHUNK_CHAINS, ct.byref(v)), "ey_plan_get_option")
        return v.value

    @max_chunk_chains.setter
    def max_chunk_chains(self, k):
        L.check(L.lib().ey_plan_set_option(self.handle, L.EY_OPT_MAX_CHUNK_CHAINS, int(k)), "ey_plan_set_option")

    def set_variant(self, variant):
        """Diagnostic switches of THIS plan (ey_plan_set_variant); returns the previous value."""
        return L.lib().ey_plan_set_variant(self.handle, int(variant))

    # ------------------------------------------------------------------ data / prior
    def _prep(self, t, shape=None):
        t = torch.as_tensor(t)
        t = t.to(device=self.device, dtype=self.dtype).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def set_data(self, x, y):
        """Attach the batch (asynchronous on the current stream: device-to-device copies and two small kernels).
        The upload is skipped only when the SAME tensor objects, unmodified (``_version``), are passed again: the plan
        keeps references to them, so their storage cannot be recycled for another batch while the key is live (an
        address-based key matches a freed temporary's successor and would silently keep the old data)."""
        key = (x._version, y._version)
        if self._data_key is not None and self._data_ref[0] is x and self._data_ref[1] is y and key == self._data_key:
            return
        xd = self._prep(x)
        yd = self._prep(y)
        if xd.dim() != 2 or xd.shape[1] != self.dims[0]:
            raise ValueError(f"x must be [N, {self.dims[0]}], got {tuple(xd.shape)}")
        yd = yd.reshape(xd.shape[0], -1)
        if yd.shape[1] != self.dims[-1]:
            raise ValueError(f"y must be [N, {self.dims[-1]}], got {tuple(yd.shape)}")
        L.check(L.lib().ey_plan_set_data(self.handle, L.ptr(xd), L.ptr(yd), xd.shape[0], _stream(self.device)),
                "ey_plan_set_data")
        self._data_key, self._data_ref = key, (x, y)
        self.N = xd.shape[0]

    def set_prior(self, mu, sigma):
        mu = self._prep(torch.broadcast_to(torch.as_tensor(mu), (self.P,)), (self.P,))
        sigma = self._prep(torch.broadcast_to(torch.as_tensor(sigma), (self.P,)), (self.P,))
        L.check(L.lib().ey_plan_set_prior(self.handle, L.ptr(mu), L.ptr(sigma), _stream(self.device)),
                "ey_plan_set_prior")

    def set_prior_family(self, family, loc, scale, df=None):
        """An elementwise prior of another family (ey_plan_set_prior_family): ``family`` is ``EY_PRIOR_NORMAL``,
        ``EY_PRIOR_LAPLACE`` or ``EY_PRIOR_STUDENT_T`` of ``eeyore_amd._lib`` (a Cauchy prior is Student-t with ``df`` = 1);
        ``loc``, ``scale`` and, for Student-t, ``df`` broadcast to [P].  The library validates the tables on the host
        (``ValueError``) before it stores anything.  A plan whose family is not Normal runs on the generic kernels only:
        ``kernel`` says 'generic', and a model they cannot hold in LDS raises on every operation."""
        loc = self._prep(torch.broadcast_to(torch.as_tensor(loc), (self.P,)), (self.P,))
        scale = self._prep(torch.broadcast_to(torch.as_tensor(scale), (self.P,)), (self.P,))
        if df is not None:
            df = self._prep(torch.broadcast_to(torch.as_tensor(df), (self.P,)), (self.P,))
        L.check(L.lib().ey_plan_set_prior_family(self.handle, int(family), L.ptr(loc), L.ptr(scale), L.ptr(df),
                                                 _stream(self.device)), "ey_plan_set_prior_family")

    @property
    def prior_family(self):
        """``EY_PRIOR_NORMAL`` / ``_LAPLACE`` / ``_STUDENT_T``: the family of the prior the plan holds."""
        return L.lib().ey_plan_prior_family(self.handle)

    def set_lik_scale(self, scale):
        """The scale s of a Gaussian or Laplace likelihood (ey_plan_set_lik_scale; the default is 1): one positive number
        for all outputs.  ``ValueError`` when it is not finite and > 0, or on a plan of a classification or Poisson code."""
        L.check(L.lib().ey_plan_set_lik_scale(self.handle, float(scale)), "ey_plan_set_lik_scale")

    @property
    def lik_scale(self):
        """The scale of the plan's Gaussian or Laplace likelihood (1 for the codes that have none)."""
        return L.lib().ey_plan_lik_scale(self.handle)

    # ------------------------------------------------------------------ helpers
    def _theta(self, theta):
        if theta.device != self.device or theta.dtype != self.dtype or not theta.is_contiguous():
            raise ValueError("theta must be a contiguous tensor of the plan's dtype on the plan's device")
        if theta.dim() != 2 or theta.shape[1] != self.P:
            raise ValueError(f"theta must be [C, {self.P}]")
        return theta.shape[0]

    def _opt(self, t, C):
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=self.dtype, device=self.device)
        if t.dim() == 0:
            t = t.expand(C)
        return t.contiguous()

    def empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.dtype, device=self.device)

    # ------------------------------------------------------------------ compute
    def log_target(self, theta, temp=None, prior_only=False):
        C = self._theta(theta)
        lik, prior = (None if prior_only else self.empty(C)), self.empty(C)
        temp = self._opt(temp, C)
        L.check(L.lib().ey_log_target(self.handle, L.ptr(theta), L.ptr(temp), C, L.ptr(lik), L.ptr(prior),
                                      _stream(self.device)), "ey_log_target")
        return lik, prior

    def log_lik_rows(self, theta, temp=None):
        """[C, N]: the log-likelihood term of every data row under every chain's parameters (ey_log_lik_rows)."""
        C = self._theta(theta)
        rows = self.empty(C, self.N)
        temp = self._opt(temp, C)
        L.check(L.lib().ey_log_lik_rows(self.handle, L.ptr(theta), L.ptr(temp), C, L.ptr(rows), _stream(self.device)),
                "ey_log_lik_rows")
        return rows

    def forward(self, theta):
        """[C, N, dK]: the network outputs of every chain's parameters on the attached batch, after the last activation
        (ey_forward).  Any likelihood, any prior; the generic kernels or the layerwise forward products, whatever family
        serves the plan's draws (``kernel`` is unchanged)."""
        C = self._theta(theta)
        out = self.empty(C, self.N, self.dims[-1])
        L.check(L.lib().ey_forward(self.handle, L.ptr(theta), C, L.ptr(out), _stream(self.device)), "ey_forward")
        return out

    def log_target_grad(self, theta, temp=None):
        C = self._theta(theta)
        target, grad = self.empty(C), self.empty(C, self.P)
        temp = self._opt(temp, C)
        L.check(L.lib().ey_log_target_grad(self.handle, L.ptr(theta), L.ptr(temp), C, L.ptr(target), L.ptr(grad),
                                           _stream(self.device)), "ey_log_target_grad")
        return target, grad

    # ------------------------------------------------------------------ attached dual averaging
    def attach_da(self, state, step_vec, table, n, d, log_eub=None, final_avg=True):
        """ey_plan_attach_da; the plan keeps the three tensors alive until ``detach_da`` (the library holds raw device
        pointers into them and writes the step and the state after every adapting iteration)."""
        L.check(L.lib().ey_plan_attach_da(self.handle, L.ptr(state), L.ptr(step_vec), L.ptr(table), int(n),
                                          int(step_vec.shape[0]), float(d),
                                          float('nan') if log_eub is None else float(log_eub), int(bool(final_avg))),
                "ey_plan_attach_da")
        self._da_refs = (state, step_vec, table)

    def detach_da(self):
        """Drop whatever dual averaging is attached (a no-op when none is): safe to call before every run."""
        L.check(L.lib().ey_plan_attach_da(self.handle, None, None, None, 0, 0, 0.5, float('nan'), 0),
                "ey_plan_attach_da")
        self._da_refs = None

    # ------------------------------------------------------------------ attached running moments
    def attach_moments(self, s1, s2, acc, on_step=None):
        """From now on every hmc_step / mala_step / mh_step also adds the state each chain is left in to the double
        accumulators s1, s2 [C, P] and its accept flag to acc [C] (ey_plan_attach_moments): inside the fused kernel where
        there is one.  ``on_step`` is called after each such step (e.g. to count iterations)."""
        for t in (s1, s2, acc):
            if t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("moment accumulators must be contiguous float64 tensors on the plan's device")
        C = s1.shape[0]
        if tuple(s1.shape) != (C, self.P) or tuple(s2.shape) != (C, self.P) or tuple(acc.shape) != (C,):
            raise ValueError(f"expected s1, s2 [C, {self.P}] and acc [C]")
        L.check(L.lib().ey_plan_attach_moments(self.handle, L.ptr(s1), L.ptr(s2), L.ptr(acc), C),
                "ey_plan_attach_moments")
        self._moments = (s1, s2, acc, on_step)  # keeps the tensors alive

    def detach_moments(self):
        L.check(L.lib().ey_plan_attach_moments(self.handle, None, None, None, 0), "ey_plan_attach_moments")
        self._moments = None

    def _stepped(self, times=1):
        if self._moments is not None and self._moments[3] is not None:
            for _ in range(times):
                self._moments[3]()

    # ------------------------------------------------------------------ samplers
    def _want(self, name, t, shape, dtype, msg=None):
        """``t`` is a contiguous tensor of that shape and dtype on the plan's device, or ValueError (``msg`` where a
        caller words it its own way)."""
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
            raise ValueError(msg or f"{name} must be a contiguous {dtype} tensor of shape {shape} on the plan's device")

    def _records(self, n_iters, C, samples, targets, accepted_rec, accept_count, each=()):
        for name, t, shape, dt in (("samples", samples, (n_iters, C, self.P), self.dtype),
                                   ("targets", targets, (n_iters, C), self.dtype),
                                   ("accepted_rec", accepted_rec, (n_iters, C) + each, torch.uint8),
                                   ("accept_count", accept_count, (C,) + each, torch.int32)):
            if t is not None:
                self._want(name, t, shape, dt)

    def _sample(self, fn, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=None, records=None, each=(),
                tail=None):
        """One call of the sampler entry point ``fn``.  ``lead``: its own arguments between the plan and
        ``temp``; ``out``: the caller's dict or None (then accepted and, for a step, log_rate, of shape [C]);
        ``n_iters`` and ``records`` (samples, targets, accepted_rec, accept_count) make it a run; ``tail``: what the
        entry point takes between accepted and the stream (None: a step's log_rate, nothing for a run).  ``lead`` and
        ``tail`` hold device pointers (``L.ptr``): a caller that converts an argument (``_opt``) keeps the result in a
        local, alive until the call has queued its work.  ``each``: the trailing shape of Gibbs's per-block records."""
        if out is None:
            out = dict(accepted=self.empty(C, dtype=torch.uint8))
            if n_iters is None:
                out["log_rate"] = self.empty(C)
        temp = self._opt(temp, C)
        if n_iters is None:
            rc = fn(self.handle, *lead, L.ptr(temp), C, int(seed), int(it), int(chain_offset), int(flags),
                    L.ptr(out["accepted"]), *(tail or (L.ptr(out["log_rate"]),)), _stream(self.device))
        else:
            n_iters = int(n_iters)
            self._records(n_iters, C, *records, each)
            rc = fn(self.handle, *lead, L.ptr(temp), C, int(seed), int(it), int(chain_offset), int(flags), n_iters,
                    *[L.ptr(r) for r in records], L.ptr(out["accepted"]), *(tail or ()), _stream(self.device))
        if rc:  # (L.check and _stepped return at once for most draws; not calling them is 0.2 us of every sampler call)
            L.check(rc, fn.__name__)
        if self._moments is not None:
            self._stepped(n_iters or 1)
        return out

    def hmc_step(self, theta, target, grad, step, num_steps, p0=None, u=None, step_vec=None, temp=None, seed=0, it=0,
                 chain_offset=0, flags=0, out=None):
        C = self._theta(theta)
        if out is None:
            out = dict(accepted=self.empty(C, dtype=torch.uint8), rate=self.empty(C), h_cur=self.empty(C),
                       h_prop=self.empty(C))
        u, step_vec = self._opt(u, C), self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(p0), L.ptr(u), float(step), L.ptr(step_vec), int(num_steps))
        return self._sample(L.lib().ey_hmc_step, C, lead, temp, seed, it, chain_offset, flags, out,
                            tail=(L.ptr(out["rate"]), L.ptr(out["h_cur"]), L.ptr(out["h_prop"])))

    def hmc_run(self, theta, target, grad, step, num_steps, n_iters, step_vec=None, temp=None, seed=0, it=0,
                chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` HMC iterations (it, it + 1, ...) of every chain in ONE launch (ey_hmc_run): the in-kernel Philox
        streams only, bit-identical to ``n_iters`` calls of ``hmc_step`` without ``p0`` / ``u``.  Optional records of the
        state after each iteration: ``samples`` [n_iters, C, P], ``targets`` [n_iters, C], ``accepted_rec`` [n_iters, C]
        uint8 (contiguous views, e.g. slices of a ChainBuffer's storage); ``accept_count`` [C] int32 is incremented."""
        C = self._theta(theta)
        step_vec = self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), float(step), L.ptr(step_vec), int(num_steps))
        return self._sample(L.lib().ey_hmc_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def mala_run(self, theta, target, grad, step, n_iters, step_vec=None, temp=None, seed=0, it=0, chain_offset=0,
                 flags=0, samples=None, targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` MALA iterations of every chain in one launch (ey_mala_run); records as in ``hmc_run``."""
        C = self._theta(theta)
        step_vec = self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), float(step), L.ptr(step_vec))
        return self._sample(L.lib().ey_mala_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def mh_run(self, theta, target, scale, n_iters, temp=None, seed=0, it=0, chain_offset=0, flags=0, samples=None,
               targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` random-walk MH iterations of every chain in one launch (ey_mh_run); records as in ``hmc_run``."""
        C = self._theta(theta)
        scale = self._prep(torch.broadcast_to(torch.as_tensor(scale, dtype=self.dtype, device=self.device), (self.P,)))
        lead = (L.ptr(theta), L.ptr(target), L.ptr(scale))
        return self._sample(L.lib().ey_mh_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def leapfrog(self, theta, p, step, num_steps, step_vec=None, temp=None):
        """HMC.leapfrog (hmc.py:100-124) in place on theta [C,P], p [C,P]; returns (target [C], grad [C,P])."""
        C = self._theta(theta)
        self._theta(p)
        target, grad = self.empty(C), self.empty(C, self.P)
        temp, step_vec = self._opt(temp, C), self._opt(step_vec, C)
        L.check(L.lib().ey_hmc_leapfrog(self.handle, L.ptr(theta), L.ptr(p), float(step), L.ptr(step_vec),
                                        int(num_steps), L.ptr(temp), C, L.ptr(target), L.ptr(grad),
                                        _stream(self.device)), "ey_hmc_leapfrog")
        return target, grad

    def mala_step(self, theta, target, grad, step, z=None, u=None, step_vec=None, temp=None, seed=0, it=0,
                  chain_offset=0, flags=0, out=None):
        C = self._theta(theta)
        u, step_vec = self._opt(u, C), self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(z), L.ptr(u), float(step), L.ptr(step_vec))
        return self._sample(L.lib().ey_mala_step, C, lead, temp, seed, it, chain_offset, flags, out)

    def mh_step(self, theta, target, scale, z=None, u=None, temp=None, seed=0, it=0, chain_offset=0, flags=0, out=None):
        C = self._theta(theta)
        scale = self._prep(torch.broadcast_to(torch.as_tensor(scale, dtype=self.dtype, device=self.device), (self.P,)))
        u = self._opt(u, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(z), L.ptr(u), L.ptr(scale))
        return self._sample(L.lib().ey_mh_step, C, lead, temp, seed, it, chain_offset, flags, out)

    def _tril(self, tril, index, C):
        """(G, index) of a proposal factor ``tril`` ([P, P] or [G, P, P]) for C chains, checked: without ``index`` G is 1
        or C, with it ``index`` is an int32 [C] tensor on the device with every entry in [0, G)."""
        if (not torch.is_tensor(tril) or tril.device != self.device or tril.dtype != self.dtype
                or not tril.is_contiguous() or tril.dim() not in (2, 3) or tuple(tril.shape[-2:]) != (self.P, self.P)
                or tril.shape[0] < 1):
            raise ValueError(f"tril must be a contiguous [{self.P}, {self.P}] or [G, {self.P}, {self.P}] tensor of the "
                             "plan's dtype on its device")
        G = 1 if tril.dim() == 2 else int(tril.shape[0])
        if index is None:
            if G not in (1, C):
                raise ValueError(f"tril holds {G} factors for {C} chains: without index it must hold 1 or {C}")
            return G, None
        return G, self._index(index, G, C)

    def _index(self, index, G, C):
        """``index`` as ``_tril`` and ``_metric`` take it, checked: an int32 [C] tensor on the device with every entry in
        [0, G).  The range check reads the device, so it runs once per index, not per draw: it is skipped only when the
        SAME tensor object, unmodified (``_version``), comes again for the same G and C.  The plan keeps a reference to the
        tensor it checked, as ``set_data`` does, so that its address cannot be recycled for another index while the key
        is live."""
        if (not torch.is_tensor(index) or index.device != self.device or index.dtype != torch.int32
                or tuple(index.shape) != (C,) or not index.is_contiguous()):
            raise ValueError(f"index must be a contiguous int32 tensor of shape ({C},) on the plan's device")
        key = (index._version, G, C)
        seen = getattr(self, "_tril_index_checked", None)
        if C and not (seen is not None and seen[0] is index and seen[1] == key):
            if int(index.min()) < 0 or int(index.max()) >= G:
                raise ValueError(f"index must lie in [0, {G})")
            self._tril_index_checked = (index, key)
        return index

    def mh_tril_step(self, theta, target, tril, index=None, z=None, u=None, temp=None, seed=0, it=0, chain_offset=0,
                     flags=0, out=None):
        """One MetropolisHastings.draw of every chain with the proposal theta + L z (ey_mh_tril_step): ``tril`` is one
        lower-triangular factor [P, P] for all chains, one per chain [C, P, P], or [G, P, P] with ``index`` [C] int32
        naming each chain's factor.  Only the lower triangle is read."""
        C = self._theta(theta)
        G, index = self._tril(tril, index, C)
        u = self._opt(u, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(tril), G, L.ptr(index), L.ptr(z), L.ptr(u))
        return self._sample(L.lib().ey_mh_tril_step, C, lead, temp, seed, it, chain_offset, flags, out)

    def mh_tril_run(self, theta, target, tril, n_iters, index=None, temp=None, seed=0, it=0, chain_offset=0, flags=0,
                    samples=None, targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` iterations of ``mh_tril_step`` in one launch (ey_mh_tril_run); records as in ``hmc_run``."""
        C = self._theta(theta)
        G, index = self._tril(tril, index, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(tril), G, L.ptr(index))
        return self._sample(L.lib().ey_mh_tril_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def mala_tril_step(self, theta, target, grad, step, tril, index=None, z=None, u=None, step_vec=None, temp=None, seed=0,
                       it=0, chain_offset=0, flags=0, out=None):
        """One MALA.draw of every chain with the proposal theta + step/2 grad + L z (ey_mala_tril_step): ``tril`` and
        ``index`` as in ``mh_tril_step``, the rest as in ``mala_step``.  Only the lower triangle is read."""
        C = self._theta(theta)
        G, index = self._tril(tril, index, C)
        u, step_vec = self._opt(u, C), self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(tril), G, L.ptr(index), L.ptr(z), L.ptr(u), float(step),
                L.ptr(step_vec))
        return self._sample(L.lib().ey_mala_tril_step, C, lead, temp, seed, it, chain_offset, flags, out)

    def mala_tril_run(self, theta, target, grad, step, tril, n_iters, index=None, step_vec=None, temp=None, seed=0, it=0,
                      chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` iterations of ``mala_tril_step`` in one launch (ey_mala_tril_run); records as in ``hmc_run``."""
        C = self._theta(theta)
        G, index = self._tril(tril, index, C)
        step_vec = self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(tril), G, L.ptr(index), float(step), L.ptr(step_vec))
        return self._sample(L.lib().ey_mala_tril_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def _metric(self, metric, form, index, C):
        """(form code, G, index) of an HMC metric for C chains, checked: ``form`` 'diag' with scales [P] or [G, P], 'dense'
        with lower-triangular factors [P, P] or [G, P, P]; ``index`` as in ``_tril``."""
        P = self.P
        if form not in ("diag", "dense"):
            raise ValueError("form must be 'diag' or 'dense'")
        if form == "dense":
            G, index = self._tril(metric, index, C)
            return L.EY_METRIC_TRIL, G, index
        if (not torch.is_tensor(metric) or metric.device != self.device or metric.dtype != self.dtype
                or not metric.is_contiguous() or metric.dim() not in (1, 2) or metric.shape[-1] != P
                or metric.shape[0] < 1):
            raise ValueError(f"a diagonal metric must be a contiguous [{P}] or [G, {P}] tensor of the plan's dtype on its "
                             "device")
        G = 1 if metric.dim() == 1 else int(metric.shape[0])
        if index is None:
            if G not in (1, C):
                raise ValueError(f"metric holds {G} scale vectors for {C} chains: without index it must hold 1 or {C}")
            return L.EY_METRIC_DIAG, G, None
        return L.EY_METRIC_DIAG, G, self._index(index, G, C)

    def hmc_metric_kernel(self, flags=0):
        """'mfma32' or 'generic' (ey_hmc_metric_kernel, include/eeyore_amd_hmc_metric_fused.h): the kernel
        ``hmc_metric_step``, ``hmc_metric_run`` and ``hmc_metric_warmup`` take on this plan under a diagonal metric with
        ``flags`` -- the draw on the matrix cores when ``flags`` holds EY_HMC_METRIC_FUSED without
        EY_FORCE_GENERIC and ``kernel`` is 'mfma32', otherwise the generic kernels."""
        return L.lib().ey_hmc_metric_kernel(self.handle, int(flags)).decode()

    def hmc_metric_step(self, theta, target, grad, step, num_steps, metric, form, index=None, v0=None, u=None,
                        step_vec=None, temp=None, seed=0, it=0, chain_offset=0, flags=0, out=None):
        """One HMC draw of every chain under a fixed metric with inverse L L^T (ey_hmc_metric_step,
        include/eeyore_amd_ext.h): ``form`` 'dense' with ``metric`` a lower-triangular factor L [P, P], one per chain
        [C, P, P], or [G, P, P] with ``index`` [C] int32 naming each chain's (at most 128 parameters; only the lower
        triangle is read); ``form`` 'diag' with scales s [P], [C, P] or [G, P], L = diag(s).  ``v0`` [C, P] replaces the
        draw of the whitened velocity v = L^T p, the rest is ``hmc_step``'s.  Returns accepted, rate, h_cur, h_prop."""
        C = self._theta(theta)
        code, G, index = self._metric(metric, form, index, C)
        if out is None:
            out = dict(accepted=self.empty(C, dtype=torch.uint8), rate=self.empty(C), h_cur=self.empty(C),
                       h_prop=self.empty(C))
        u, step_vec = self._opt(u, C), self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(metric), code, G, L.ptr(index), L.ptr(v0), L.ptr(u),
                float(step), L.ptr(step_vec), int(num_steps))
        return self._sample(L.lib().ey_hmc_metric_step, C, lead, temp, seed, it, chain_offset, flags, out,
                            tail=(L.ptr(out["rate"]), L.ptr(out["h_cur"]), L.ptr(out["h_prop"])))

    def hmc_metric_run(self, theta, target, grad, step, num_steps, metric, form, n_iters, index=None, step_vec=None,
                       temp=None, seed=0, it=0, chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None,
                       accept_count=None, out=None):
        """``n_iters`` iterations of ``hmc_metric_step`` in one launch (ey_hmc_metric_run); records as in ``hmc_run``."""
        C = self._theta(theta)
        code, G, index = self._metric(metric, form, index, C)
        step_vec = self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(metric), code, G, L.ptr(index), float(step),
                L.ptr(step_vec), int(num_steps))
        return self._sample(L.lib().ey_hmc_metric_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def hmc_metric_warmup(self, theta, target, grad, step, num_steps, metric, form, n_iters, index=None, step_vec=None,
                          temp=None, seed=0, it=0, chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None,
                          accept_count=None, out=None, da_state=None, da_table=None, d=0.8, log_eub=None, final_avg=False,
                          mean=None, M2=None, count=0, steps_rec=None, rate_rec=None):
        """``n_iters`` draws of ``hmc_metric_run`` in one launch that also adapt (ey_hmc_metric_warmup,
        include/eeyore_amd_warmup.h).  ``da_state`` [C, 3] float64 (barh, logbare, mu) with ``da_table`` [k, 3] float64,
        k <= n_iters rows (1/(t + t0), sqrt(t)/gamma, t^-kappa) for the launch's first k draws: dual averaging of every
        chain's step towards the acceptance ``d``, capped at exp(``log_eub``); ``step_vec`` [C] (a tensor of the plan's
        dtype, required then) is read and written in place, with ``final_avg`` draw k - 1 leaves the averaged step.
        ``mean`` [C, P] and ``M2`` [C, P] ('diag') or [C, P, P] ('dense', the lower triangle only) float64: Welford moments of
        the state each chain is left in, ``count`` draws already in them.  ``steps_rec`` / ``rate_rec`` [n_iters, C]: the
        step each draw used and its acceptance rate.  With none of these it is ``hmc_metric_run``, bit for bit."""
        C = self._theta(theta)
        code, G, index = self._metric(metric, form, index, C)
        n_iters, f64 = int(n_iters), torch.float64
        if da_state is not None or steps_rec is not None:
            if step_vec is not None:  # in/out: the caller's own tensor, not a converted copy
                self._want("step_vec", step_vec, (C,), self.dtype)
        else:
            step_vec = self._opt(step_vec, C)
        if da_state is not None:
            self._want("da_state", da_state, (C, 3), f64)
            if da_table is not None:
                self._want("da_table", da_table, (da_table.shape[0], 3), f64)
        for name, t, shape in (("mean", mean, (C, self.P)),
                               ("M2", M2, (C, self.P) if form == "diag" else (C, self.P, self.P))):
            if t is not None:
                self._want(name, t, shape, f64)
        for name, t in (("steps_rec", steps_rec), ("rate_rec", rate_rec)):
            if t is not None:
                self._want(name, t, (n_iters, C), self.dtype)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(metric), code, G, L.ptr(index), float(step),
                L.ptr(step_vec), int(num_steps))
        tail = (L.ptr(da_state), L.ptr(da_table), 0 if da_table is None else int(da_table.shape[0]), float(d),
                float('nan') if log_eub is None else float(log_eub), int(bool(final_avg)), L.ptr(mean), L.ptr(M2),
                int(count), L.ptr(steps_rec), L.ptr(rate_rec))
        return self._sample(L.lib().ey_hmc_metric_warmup, C, lead, temp, seed, it, chain_offset, flags, out,
                            n_iters=n_iters, records=(samples, targets, accepted_rec, accept_count), tail=tail)

    # ------------------------------------------------------------------ NUTS under a metric (include/eeyore_amd_nuts.h)
    def nuts_tree_bytes(self, C, max_depth):
        """The bytes of the tree's workspace for ``C`` chains at ``max_depth`` (ey_nuts_tree_bytes,
        include/eeyore_amd_nuts_tree.h): C (12 + 2 max_depth) vectors of P rounded up to 64 elements of the plan's dtype."""
        n = L.lib().ey_nuts_tree_bytes(self.handle, int(C), int(max_depth))
        if n < 0:
            L.check(int(n), "ey_nuts_tree_bytes")
        return int(n)

    def attach_nuts_tree(self, C, max_depth):
        """Gives the plan a workspace for the trees of ``C`` chains at ``max_depth`` (ey_plan_attach_nuts_tree), which the
        NUTS calls with ``flags`` | EY_NUTS_TREE_DEVICE run in: a uint8 tensor the plan keeps referenced.  It grows to the
        largest request and never shrinks; what it holds is of no account.  Returns the tensor."""
        need = self.nuts_tree_bytes(C, max_depth)
        ws = getattr(self, "_nuts_tree", None)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
            L.check(L.lib().ey_plan_attach_nuts_tree(self.handle, L.ptr(ws), ws.numel()), "ey_plan_attach_nuts_tree")
            self._nuts_tree = ws  # keeps the memory alive (and lets the old one go only now)
        return ws

    def detach_nuts_tree(self):
        L.check(L.lib().ey_plan_attach_nuts_tree(self.handle, None, 0), "ey_plan_attach_nuts_tree")
        self._nuts_tree = None

    def nuts_kernel(self, flags=0):
        """'mfma32' or 'generic' (ey_nuts_kernel, include/eeyore_amd_nuts_fused.h): the kernel ``nuts_step``, ``nuts_run``
        and ``nuts_warmup`` take on this plan under ``flags`` -- the draw on the matrix cores when
        ``flags`` holds EY_NUTS_FUSED without EY_FORCE_GENERIC and ``kernel`` is 'mfma32', otherwise the generic kernels."""
        return L.lib().ey_nuts_kernel(self.handle, int(flags)).decode()

    def _nuts_args(self, theta, metric, form, index, max_depth, out, flags=0):
        """(C, form code, G, index, out) of a NUTS call, checked: the metric as ``_metric`` checks it, at most 128 parameters
        in either form -- unless ``flags`` carry EY_NUTS_TREE_DEVICE or EY_NUTS_FUSED and the form is 'diag' (the tree in
        the attached workspace) --, ``max_depth`` in [1, 10]; ``out`` gets the [C] outputs of a draw it does not hold yet."""
        C = self._theta(theta)
        if self.P > 128 and not (int(flags) & (L.EY_NUTS_TREE_DEVICE | L.EY_NUTS_FUSED) and form == "diag"):
            raise ValueError(f"NUTS is limited to 128 parameters (the model has {self.P}): the tree lives in LDS")
        code, G, index = self._metric(metric, form, index, C)
        if int(max_depth) != max_depth:
            raise ValueError(f"max_depth must be an integer in [1, {L.EY_NUTS_MAX_DEPTH}]")  # (the range: the library's)
        out = {} if out is None else out
        for name, dt in (("accepted", torch.uint8), ("depth", torch.int32), ("n_leapfrog", torch.int32),
                         ("divergent", torch.uint8), ("accept_stat", self.dtype), ("energy", self.dtype)):
            if name not in out:
                out[name] = self.empty(C, dtype=dt)
            self._want(name, out[name], (C,), dt)
        return C, code, G, index, out

    @staticmethod
    def _nuts_out(out):
        return tuple(L.ptr(out[k]) for k in ("depth", "n_leapfrog", "divergent", "accept_stat", "energy"))

    def nuts_step(self, theta, target, grad, step, max_depth, metric, form, index=None, v0=None, u=None, step_vec=None,
                  temp=None, seed=0, it=0, chain_offset=0, flags=0, out=None):
        """One draw of multinomial NUTS for every chain under a fixed metric (ey_nuts_step): ``metric``,
        ``form`` and ``index`` as in ``hmc_metric_step``, at most 128 parameters in either form; ``max_depth`` in [1, 10]
        doublings.  With EY_NUTS_TREE_DEVICE in ``flags`` and form 'diag' the tree lives in the workspace of
        ``attach_nuts_tree`` and P is not limited (include/eeyore_amd_nuts_tree.h; the same holds of the run and the warm-up);
        with EY_NUTS_FUSED the draw also runs on the matrix cores where ``nuts_kernel`` says 'mfma32'
        (include/eeyore_amd_nuts_fused.h).  ``v0`` [C, P] replaces the draw of the whitened velocity, ``u`` [C, S] (S >= 21 + 2^max_depth) the
        chain's uniform stream in its word layout (1 + 2d the direction of doubling d, 2 + 2d its top-level move, 21 + n
        leaf n).  Returns accepted (the state moved), depth, n_leapfrog, divergent, accept_stat, energy, each [C]."""
        C, code, G, index, out = self._nuts_args(theta, metric, form, index, max_depth, out, flags)
        step_vec = self._opt(step_vec, C)
        S = 0
        if u is not None:
            if u.dim() != 2:
                raise ValueError("u must be a [C, S] table of uniforms")
            S = int(u.shape[1])
            self._want("u", u, (C, S), self.dtype)
        if v0 is not None:
            self._want("v0", v0, (C, self.P), self.dtype)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(metric), code, G, L.ptr(index), L.ptr(v0), L.ptr(u), S,
                float(step), L.ptr(step_vec), int(max_depth))
        return self._sample(L.lib().ey_nuts_step, C, lead, temp, seed, it, chain_offset, flags, out,
                            tail=self._nuts_out(out))

    def _nuts_recs(self, n_iters, C, depth_rec, divergent_rec):
        for name, t, dt in (("depth_rec", depth_rec, torch.int32), ("divergent_rec", divergent_rec, torch.uint8)):
            if t is not None:
                self._want(name, t, (n_iters, C), dt)
        return L.ptr(depth_rec), L.ptr(divergent_rec)

    def nuts_run(self, theta, target, grad, step, max_depth, metric, form, n_iters, index=None, step_vec=None, temp=None,
                 seed=0, it=0, chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None, accept_count=None,
                 depth_rec=None, divergent_rec=None, out=None):
        """``n_iters`` iterations of ``nuts_step`` on the in-kernel streams in one launch (ey_nuts_run), bit for bit;
        records as in ``hmc_run``, and ``depth_rec`` [n_iters, C] int32, ``divergent_rec`` [n_iters, C] uint8."""
        C, code, G, index, out = self._nuts_args(theta, metric, form, index, max_depth, out, flags)
        step_vec = self._opt(step_vec, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(metric), code, G, L.ptr(index), float(step),
                L.ptr(step_vec), int(max_depth))
        tail = self._nuts_out(out) + self._nuts_recs(int(n_iters), C, depth_rec, divergent_rec)
        return self._sample(L.lib().ey_nuts_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count), tail=tail)

    def nuts_warmup(self, theta, target, grad, step, max_depth, metric, form, n_iters, index=None, step_vec=None,
                    temp=None, seed=0, it=0, chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None,
                    accept_count=None, depth_rec=None, divergent_rec=None, out=None, da_state=None, da_table=None, d=0.8,
                    log_eub=None, final_avg=False, mean=None, M2=None, count=0, steps_rec=None, rate_rec=None):
        """``nuts_run`` with the two epilogues of ``hmc_metric_warmup`` after each draw (ey_nuts_warmup): dual averaging of
        every chain's step on the draw's accept_stat, Welford moments of the state it is left in.  The arguments from
        ``da_state`` on are ``hmc_metric_warmup``'s (``rate_rec`` records accept_stat); with none of them it is
        ``nuts_run``, bit for bit."""
        C, code, G, index, out = self._nuts_args(theta, metric, form, index, max_depth, out, flags)
        n_iters, f64 = int(n_iters), torch.float64
        if da_state is not None or steps_rec is not None:
            if step_vec is not None:  # in/out: the caller's own tensor, not a converted copy
                self._want("step_vec", step_vec, (C,), self.dtype)
        else:
            step_vec = self._opt(step_vec, C)
        if da_state is not None:
            self._want("da_state", da_state, (C, 3), f64)
            if da_table is not None:
                self._want("da_table", da_table, (da_table.shape[0], 3), f64)
        for name, t, shape in (("mean", mean, (C, self.P)),
                               ("M2", M2, (C, self.P) if form == "diag" else (C, self.P, self.P))):
            if t is not None:
                self._want(name, t, shape, f64)
        for name, t in (("steps_rec", steps_rec), ("rate_rec", rate_rec)):
            if t is not None:
                self._want(name, t, (n_iters, C), self.dtype)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(grad), L.ptr(metric), code, G, L.ptr(index), float(step),
                L.ptr(step_vec), int(max_depth))
        tail = self._nuts_out(out) + self._nuts_recs(n_iters, C, depth_rec, divergent_rec) + (
            L.ptr(da_state), L.ptr(da_table), 0 if da_table is None else int(da_table.shape[0]), float(d),
            float('nan') if log_eub is None else float(log_eub), int(bool(final_avg)), L.ptr(mean), L.ptr(M2), int(count),
            L.ptr(steps_rec), L.ptr(rate_rec))
        return self._sample(L.lib().ey_nuts_warmup, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count), tail=tail)

    # ------------------------------------------------------------------ elliptical slice sampling (include/eeyore_amd_eslice.h)
    def _eslice_base(self, base_loc, base_scale):
        """The two base tables as [P] tensors of the plan's dtype on its device (or None, None), checked: both or neither,
        every scale positive and finite (the library sees device pointers only and cannot look)."""
        if (base_loc is None) != (base_scale is None):
            raise ValueError("base_loc and base_scale go together: give both tables of the Gaussian base, or neither")
        if base_loc is None:
            return None, None
        seen = getattr(self, '_eslice_seen', None)  # the pair checked last, unmodified: no second look (it synchronises)
        if (seen is not None and seen[0] is base_loc and seen[1] is base_scale
                and seen[2] == (base_loc._version, base_scale._version)):
            return base_loc, base_scale
        kw = dict(dtype=self.dtype, device=self.device)
        loc = self._prep(torch.broadcast_to(torch.as_tensor(base_loc, **kw), (self.P,)))
        scale = self._prep(torch.broadcast_to(torch.as_tensor(base_scale, **kw), (self.P,)))
        if not bool((torch.isfinite(scale) & (scale > 0)).all()):
            raise ValueError("base_scale must be positive and finite in every coordinate")
        if not bool(torch.isfinite(loc).all()):
            raise ValueError("base_loc must be finite in every coordinate")
        if loc is base_loc and scale is base_scale:  # already [P] tensors of the plan's: remembered
            self._eslice_seen = (loc, scale, (loc._version, scale._version))
        return loc, scale

    def eslice_kernel(self, flags=0):
        """'mfma32' or 'generic' (ey_eslice_kernel, include/eeyore_amd_eslice_fused.h): the kernel ``eslice_step`` and
        ``eslice_run`` take on this plan under ``flags`` -- the fused form on the matrix cores wherever ``kernel`` is
        'mfma32' (DESIGN.md 4.26), unless ``flags`` holds EY_FORCE_GENERIC.  ``eslice_ell`` takes no flags and follows the
        plan alone."""
        return L.lib().ey_eslice_kernel(self.handle, int(flags)).decode()

    def eslice_ell(self, theta, base_loc=None, base_scale=None, temp=None):
        """(ell [C], target [C]) at ``theta`` (ey_eslice_ell): what elliptical slice sampling slices on -- the (tempered)
        log-likelihood under the plan's Normal prior, or with a Gaussian base the (tempered) log-target minus the base's
        exponent -- and the (tempered) log-target, from the value-only evaluation ``eslice_step`` makes."""
        C = self._theta(theta)
        loc, scale = self._eslice_base(base_loc, base_scale)
        ell, target = self.empty(C), self.empty(C)
        temp = self._opt(temp, C)
        L.check(L.lib().ey_eslice_ell(self.handle, L.ptr(theta), L.ptr(loc), L.ptr(scale), L.ptr(temp), C, L.ptr(ell),
                                      L.ptr(target), _stream(self.device)), "ey_eslice_ell")
        return ell, target

    def _eslice_args(self, theta, target, ell, max_shrinks, out):
        C = self._theta(theta)
        self._want("target", target, (C,), self.dtype)
        self._want("ell", ell, (C,), self.dtype)
        if int(max_shrinks) != max_shrinks:
            raise ValueError(f"max_shrinks must be an integer in [1, {L.EY_ESLICE_MAX_SHRINKS}]")  # (the range: the library's)
        out = {} if out is None else out
        for name, dt in (("accepted", torch.uint8), ("n_evals", torch.int32)):
            if name not in out:
                out[name] = self.empty(C, dtype=dt)
            self._want(name, out[name], (C,), dt)
        return C, out

    def eslice_step(self, theta, target, ell, base_loc=None, base_scale=None, z=None, u=None, max_shrinks=64, temp=None,
                    seed=0, it=0, chain_offset=0, flags=0, out=None):
        """One elliptical slice draw of every chain (ey_eslice_step), in place on ``theta`` [C, P],
        ``target`` [C] and ``ell`` [C] (as ``eslice_ell`` returns them).  Without a base the plan's Normal prior is the
        Gaussian and ell the log-likelihood; ``base_loc`` / ``base_scale`` [P] name another.  ``z`` [C, P] replaces the
        chain's normal stream, ``u`` [C, S] (S >= 2 + max_shrinks) its uniform stream in the word layout (0 the slice
        height, 1 the first angle, 2 + k the k-th shrink).  Returns accepted (the chain moved) and n_evals, each [C]."""
        C, out = self._eslice_args(theta, target, ell, max_shrinks, out)
        loc, scale = self._eslice_base(base_loc, base_scale)
        S = 0
        if u is not None:
            if u.dim() != 2:
                raise ValueError("u must be a [C, S] table of uniforms")
            S = int(u.shape[1])
            self._want("u", u, (C, S), self.dtype)
        if z is not None:
            self._want("z", z, (C, self.P), self.dtype)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(ell), L.ptr(loc), L.ptr(scale), L.ptr(z), L.ptr(u), S, int(max_shrinks))
        return self._sample(L.lib().ey_eslice_step, C, lead, temp, seed, it, chain_offset, flags, out,
                            tail=(L.ptr(out["n_evals"]),))

    def eslice_run(self, theta, target, ell, n_iters, base_loc=None, base_scale=None, max_shrinks=64, temp=None, seed=0,
                   it=0, chain_offset=0, flags=0, samples=None, targets=None, accepted_rec=None, accept_count=None,
                   n_evals_rec=None, out=None):
        """``n_iters`` iterations of ``eslice_step`` on the in-kernel streams in one launch (ey_eslice_run), bit for bit;
        records as in ``mh_run``, and ``n_evals_rec`` [n_iters, C] int32."""
        C, out = self._eslice_args(theta, target, ell, max_shrinks, out)
        loc, scale = self._eslice_base(base_loc, base_scale)
        if n_evals_rec is not None:
            self._want("n_evals_rec", n_evals_rec, (int(n_iters), C), torch.int32)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(ell), L.ptr(loc), L.ptr(scale), int(max_shrinks))
        return self._sample(L.lib().ey_eslice_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count),
                            tail=(L.ptr(out["n_evals"]), L.ptr(n_evals_rec)))

    def metric_from_moments(self, mean, M2, n, form, pooled=True, table=None, status=None):
        """A metric table of the plan's dtype from the running moments ``hmc_metric_warmup`` leaves after ``n`` draws of
        every chain (ey_metric_from_moments): Stan's regularised estimate as ``DiagMetric`` / ``DenseMetric.from_samples``
        define it, one for all chains (``pooled``: [P] or [P, P], the chains summed in index order) or one per chain
        ([C, P] or [C, P, P]).  Returns (table, status): status int32 per entry, 0 fine, 1 a non-finite input or a pivot
        that is not positive -- that entry of ``table`` (the caller's, or a new one of zeros) is then left untouched."""
        if form not in ("diag", "dense"):
            raise ValueError("form must be 'diag' or 'dense'")
        P, f64 = self.P, torch.float64
        if not torch.is_tensor(mean) or mean.dim() != 2:
            raise ValueError(f"mean must be a [C, {P}] float64 tensor")
        C = int(mean.shape[0])
        self._want("mean", mean, (C, P), f64)
        self._want("M2", M2, (C, P) if form == "diag" else (C, P, P), f64)
        entries = 1 if pooled else C
        shape = ((P,) if form == "diag" else (P, P)) if pooled else ((C, P) if form == "diag" else (C, P, P))
        if table is None:
            table = torch.zeros(shape, dtype=self.dtype, device=self.device)
        self._want("table", table, shape, self.dtype)
        if status is None:
            status = torch.zeros(entries, dtype=torch.int32, device=self.device)
        self._want("status", status, (entries,), torch.int32)
        with torch.cuda.device(self.device):  # the entry point takes no plan: it runs on the current device
            L.check(L.lib().ey_metric_from_moments(L.ptr(mean), L.ptr(M2), int(n), C, P,
                                                   L.EY_METRIC_DIAG if form == "diag" else L.EY_METRIC_TRIL,
                                                   int(bool(pooled)), _DT[self.dtype], L.ptr(table), L.ptr(status),
                                                   _stream(self.device)), "ey_metric_from_moments")
        return table, status

    def _chol(self, chol, C):
        P = self.P
        self._want("chol", chol, (C, P, P), self.dtype,
                   f"chol must be a contiguous [{C}, {P}, {P}] tensor of the plan's dtype on its device")

    def ram_step(self, theta, target, chol, n, a=0.234, g=0.7, z=None, u=None, temp=None, seed=0, it=0, chain_offset=0,
                 flags=0, out=None):
        """One RAM.draw (eeyore/samplers/ram.py:38-70) of every chain (ey_ram_step): theta [C,P], target [C] and the
        lower-triangular factor chol [C,P,P] are updated in place; ``n`` is the adaptation index counter.idx + 1 - offset."""
        C = self._theta(theta)
        self._chol(chol, C)
        u = self._opt(u, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(chol), L.ptr(z), L.ptr(u), float(a), float(g), int(n))
        return self._sample(L.lib().ey_ram_step, C, lead, temp, seed, it, chain_offset, flags, out)

    def ram_run(self, theta, target, chol, n, n_iters, a=0.234, g=0.7, temp=None, seed=0, it=0, chain_offset=0, flags=0,
                samples=None, targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` RAM iterations of every chain in one launch (ey_ram_run), adaptation indices n, n + 1, ...;
        records as in ``hmc_run``."""
        C = self._theta(theta)
        self._chol(chol, C)
        lead = (L.ptr(theta), L.ptr(target), L.ptr(chol), float(a), float(g), int(n))
        return self._sample(L.lib().ey_ram_run, C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count))

    def gibbs_table(self, blocks, scales):
        """The device block table of a Gibbs sampler on this plan (ey_gibbs_table_create): ``blocks`` is a list of S
        disjoint index lists in visiting order, ``scales`` one positive proposal scale per block."""
        return GibbsTable(self, blocks, scales)

    def _gibbs_args(self, table, C, mode):
        if not isinstance(table, GibbsTable):
            raise ValueError("table must be a GibbsTable (Plan.gibbs_table)")
        if mode not in GIBBS_MODES:
            raise ValueError("mode must be 'intended' (a rejected block is restored) or 'reference' (it is carried)")
        return table.S, GIBBS_MODES[mode]

    def gibbs_step(self, theta, target, table, z=None, u=None, mode='intended', temp=None, seed=0, it=0, chain_offset=0,
                   flags=0, out=None):
        """One Gibbs.draw (eeyore/samplers/gibbs.py:67-102) of every chain (ey_gibbs_step): the table's S Metropolis
        sub-steps; theta [C,P] and target [C] are updated in place.  z [C,P] and u [C,S] replace the random draws.
        Returns accepted [C,S] uint8 and log_rate [C,S]."""
        C = self._theta(theta)
        S, carry = self._gibbs_args(table, C, mode)
        for name, t, shape in (("z", z, (C, self.P)), ("u", u, (C, S))):
            if t is not None:
                self._want(name, t, shape, self.dtype,
                           f"{name} must be a contiguous {shape} tensor of the plan's dtype on its device")
        if out is None:
            out = dict(accepted=self.empty(C, S, dtype=torch.uint8), log_rate=self.empty(C, S))
        lead = (table.handle, L.ptr(theta), L.ptr(target), L.ptr(z), L.ptr(u))
        return self._sample(L.lib().ey_gibbs_step, C, lead, temp, seed, it, chain_offset, int(flags) | carry, out)

    def gibbs_run(self, theta, target, table, n_iters, mode='intended', temp=None, seed=0, it=0, chain_offset=0, flags=0,
                  samples=None, targets=None, accepted_rec=None, accept_count=None, out=None):
        """``n_iters`` Gibbs draws of every chain in one launch (ey_gibbs_run); records as in ``hmc_run`` except that
        ``accepted_rec`` is [n_iters, C, S] and ``accept_count`` [C, S]."""
        C = self._theta(theta)
        S, carry = self._gibbs_args(table, C, mode)
        if out is None:
            out = dict(accepted=self.empty(C, S, dtype=torch.uint8))
        lead = (table.handle, L.ptr(theta), L.ptr(target))
        return self._sample(L.lib().ey_gibbs_run, C, lead, temp, seed, it, chain_offset, int(flags) | carry, out,
                            n_iters=n_iters, records=(samples, targets, accepted_rec, accept_count), each=(S,))

    def _am_state(self, C, running_mean, cov_sum, cov, num_accepted, cov0, breakdowns):
        P = self.P
        for name, t, shape, dt in (("running_mean", running_mean, (C, P), self.dtype),
                                   ("cov_sum", cov_sum, (C, P, P), self.dtype), ("cov", cov, (C, P, P), self.dtype),
                                   ("num_accepted", num_accepted, (C,), torch.int32),
                                   ("breakdowns", breakdowns, (C,), torch.int32)):
            self._want(name, t, shape, dt)
        self._want("cov0", cov0, (P, P) if cov0.dim() == 2 else (C, P, P), self.dtype,
                   f"cov0 must be a contiguous [{P}, {P}] or [{C}, {P}, {P}] tensor of the plan's dtype on its device")
        return int(cov0.dim() == 3)

    def _am(self, kind, theta, target, state, cov0, breakdowns, settings, softabs_a):
        """(entry, C, the leading arguments, breakdowns) of ey_am_<kind> (ey_am_softabs_<kind> with ``softabs_a``, which
        then takes the place of eps) on the checked ``state`` = (running_mean, cov_sum, cov, num_accepted)."""
        C = self._theta(theta)
        if breakdowns is None:
            breakdowns = torch.zeros(C, dtype=torch.int32, device=self.device)
        per_chain = self._am_state(C, *state, cov0, breakdowns)
        l, b, c, eps, t0, idx, offset = settings
        lead = (L.ptr(theta), L.ptr(target), *[L.ptr(t) for t in state], L.ptr(cov0), per_chain, float(l), float(b), float(c),
                float(eps if softabs_a is None else softabs_a), int(t0), int(idx), int(offset))
        return ("ey_am_" if softabs_a is None else "ey_am_softabs_") + kind, C, lead, breakdowns

    def am_step(self, theta, target, running_mean, cov_sum, cov, num_accepted, cov0, idx, l=0.05, b=1., c=1., eps=0.,
                t0=2, offset=0, z=None, u_mix=None, u=None, temp=None, seed=0, it=0, chain_offset=0, flags=0,
                breakdowns=None, out=None, softabs_a=None):
        """One AM.draw (eeyore/samplers/am.py:61-107) of every chain (ey_am_step) with the ridge cov + eps I fused, or,
        with ``softabs_a``, the transform softabs(cov, softabs_a) (ey_am_softabs_step; ``eps`` is then not used):
        theta [C,P], target [C], running_mean [C,P], cov_sum and cov [C,P,P] (lower triangles) and num_accepted [C] int32
        are updated in place; ``cov0`` is the transformed initial covariance, ``idx`` the counter index of the draw.
        ``breakdowns`` [C] int32 is incremented for a chain whose covariance could not be factorised."""
        entry, C, lead, breakdowns = self._am("step", theta, target, (running_mean, cov_sum, cov, num_accepted), cov0,
                                              breakdowns, (l, b, c, eps, t0, idx, offset), softabs_a)
        if out is None:
            out = dict(accepted=self.empty(C, dtype=torch.uint8), log_rate=self.empty(C),
                       branch=self.empty(C, dtype=torch.uint8))
        out["breakdowns"] = breakdowns
        u_mix, u = self._opt(u_mix, C), self._opt(u, C)
        lead += (L.ptr(z), L.ptr(u_mix), L.ptr(u))
        return self._sample(getattr(L.lib(), entry), C, lead, temp, seed, it, chain_offset, flags, out,
                            tail=(L.ptr(out.get("log_rate")), L.ptr(out.get("branch")), L.ptr(breakdowns)))

    def am_run(self, theta, target, running_mean, cov_sum, cov, num_accepted, cov0, idx, n_iters, l=0.05, b=1., c=1.,
               eps=0., t0=2, offset=0, temp=None, seed=0, it=0, chain_offset=0, flags=0, breakdowns=None, samples=None,
               targets=None, accepted_rec=None, accept_count=None, out=None, softabs_a=None):
        """``n_iters`` AM iterations of every chain in one launch (ey_am_run; ey_am_softabs_run with ``softabs_a``),
        counter indices idx, idx + 1, ...; records as in ``hmc_run``."""
        entry, C, lead, breakdowns = self._am("run", theta, target, (running_mean, cov_sum, cov, num_accepted), cov0,
                                              breakdowns, (l, b, c, eps, t0, idx, offset), softabs_a)
        if out is None:
            out = dict(accepted=self.empty(C, dtype=torch.uint8))
        out["breakdowns"] = breakdowns
        return self._sample(getattr(L.lib(), entry), C, lead, temp, seed, it, chain_offset, flags, out, n_iters=n_iters,
                            records=(samples, targets, accepted_rec, accept_count), tail=(L.ptr(breakdowns),))

    def am_softabs_fits(self):
        """Whether the softabs instantiation of the AM kernel has room for this plan's model (ey_am_softabs_fits)."""
        return bool(L.lib().ey_am_softabs_fits(self.handle))

    def pt_swap_decide(self, ell_i, ell_j, t_i, t_j, u, dlogq=None):
        return pt_swap_decide(ell_i, ell_j, t_i, t_j, u, dlogq=dlogq)

    def pt_ladder(self, t, q):
        """The device ladder of a power-posterior sampler on this plan's dtype and device (ey_pt_ladder_create)."""
        return PtLadder(t, q, self.dtype, self.device)

    def pt_between(self, ladder, theta, target, grad=None, **kw):
        return pt_between(ladder, theta, target, grad, **kw)

    def philox_normal(self, C, seed, it, chain_offset=0):
        out = self.empty(C, self.P)
        L.check(L.lib().ey_philox_normal(L.ptr(out), C, self.P, int(seed), int(it), int(chain_offset), _DT[self.dtype],
                                         _stream(self.device)), "ey_philox_normal")
        return out

    def philox_uniform(self, C, seed, it, chain_offset=0):
        out = self.empty(C)
        L.check(L.lib().ey_philox_uniform(L.ptr(out), C, int(seed), int(it), int(chain_offset), _DT[self.dtype],
                                          _stream(self.device)), "ey_philox_uniform")
        return out

    def philox_uniform_blocks(self, C, S, seed, it, chain_offset=0):
        """u [C, S]: the accept variates of the S sub-steps of a Gibbs draw (ey_philox_uniform_blocks)."""
        out = self.empty(C, S)
        L.check(L.lib().ey_philox_uniform_blocks(L.ptr(out), C, int(S), int(seed), int(it), int(chain_offset),
                                                 _DT[self.dtype], _stream(self.device)), "ey_philox_uniform_blocks")
        return out


def pt_swap_decide(ell_i, ell_j, t_i, t_j, u, dlogq=None):
    """PowerPosteriorSampler.between_chain_move decision (power_posterior_sampler.py:135-163) for C pairs."""
    C = ell_i.shape[0]
    dt = ell_i.dtype
    dev = ell_i.device
    args = [a.to(device=dev, dtype=dt).contiguous() if a is not None else None for a in (ell_i, ell_j, t_i, t_j, dlogq, u)]
    swap = torch.empty(C, dtype=torch.uint8, device=dev)
    log_rate = torch.empty(C, dtype=dt, device=dev)
    L.check(L.lib().ey_pt_swap_decide(*[L.ptr(a) for a in args], C, _DT[dt], L.ptr(swap), L.ptr(log_rate), _stream(dev)),
            "ey_pt_swap_decide")
    return swap, log_rate


def pt_between(ladder, theta, target, grad=None, partners=None, u=None, seed=0, it=0, replica_offset=0, rec_theta=None,
               rec_target=None, outputs=True):
    """PowerPosteriorSampler.between_chain_moves for every replica of the ladder in ONE launch (ey_pt_between): theta
    [K*R, P], target [K*R] and grad [K*R, P] (or None) are updated in place, row k * R + r being temperature k of replica r.
    ``partners`` [K, R] int32 and ``u`` [K, R] replace the Philox draws keyed (seed, replica_offset + r, it); ``rec_theta``
    [K*R, P] / ``rec_target`` [K*R] are the record of the draw the move belongs to and take the exchanged rows too.
    Returns dict(partners, u, swap, log_rate), each [K, R] (an empty dict with ``outputs=False``).  Nothing here
    synchronises with the device."""
    if not isinstance(ladder, PtLadder):
        raise ValueError("ladder must be a PtLadder (Plan.pt_ladder)")
    K, dt, dev = ladder.K, ladder.dtype, ladder.device
    if theta.dim() != 2 or theta.shape[0] % K:
        raise ValueError(f"theta must be [K * R, P] with K = {K}")
    C, P = theta.shape
    R = C // K

    def want(name, t, shape, dtype=dt):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on the ladder's device")

    for name, t, shape in (("theta", theta, (C, P)), ("target", target, (C,)), ("grad", grad, (C, P)), ("u", u, (K, R)),
                           ("rec_theta", rec_theta, (C, P)), ("rec_target", rec_target, (C,))):
        want(name, t, shape)
    want("partners", partners, (K, R), torch.int32)
    out = {}
    if outputs:
        out = dict(partners=torch.empty(K, R, dtype=torch.int32, device=dev), u=torch.empty(K, R, dtype=dt, device=dev),
                   swap=torch.empty(K, R, dtype=torch.uint8, device=dev), log_rate=torch.empty(K, R, dtype=dt, device=dev))
    L.check(L.lib().ey_pt_between(ladder.handle, L.ptr(theta), L.ptr(target), L.ptr(grad), R, P, L.ptr(partners), L.ptr(u),
                                  int(seed), int(it), int(replica_offset), L.ptr(rec_theta), L.ptr(rec_target),
                                  L.ptr(out.get("partners")), L.ptr(out.get("u")), L.ptr(out.get("swap")),
                                  L.ptr(out.get("log_rate")), _stream(dev)), "ey_pt_between")
    return out
