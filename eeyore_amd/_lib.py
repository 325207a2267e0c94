"""ctypes binding of the C-ABI HIP library (include/eeyore_amd.h, include/eeyore_amd_ext.h, include/eeyore_amd_warmup.h,
include/eeyore_amd_nuts.h, include/eeyore_amd_eslice.h, include/eeyore_amd_eslice_fused.h,
include/eeyore_amd_nuts_tree.h, include/eeyore_amd_nuts_fused.h, include/eeyore_amd_hmc_metric_fused.h).

The library is the product path: there is no CPU or eager fallback.  ``lib()`` raises if the shared
object is missing, and every compute call raises ``RuntimeError`` with ``ey_last_error()`` on failure.
"""
import ctypes as ct
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EEYORE_AMD_LIB", os.path.join(HERE, "lib", "libeeyore_amd.so"))  # override: diagnostics
CSRC = os.path.join(HERE, "csrc")

EY_F32, EY_F64 = 0, 1
EY_ACT_NONE, EY_ACT_SIGMOID, EY_ACT_TANH, EY_ACT_RELU = 0, 1, 2, 3
EY_LIK_BCE_SUM, EY_LIK_CE_SUM = 0, 1
EY_RECOMPUTE_INITIAL_GRAD, EY_FORCE_GENERIC, EY_GIBBS_CARRY = 1, 2, 4

# every symbol include/eeyore_amd.h declares: (name, restype, argtypes)
_vp, _i, _i64, _u64, _u32, _d = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_uint64, ct.c_uint32, ct.c_double
EY_OPT_F32_PRODUCTS, EY_PRODUCTS_BF16X3, EY_PRODUCTS_EXACT = 1, 0, 1
EY_OPT_ROW_WAVES, EY_ROW_WAVES_OFF, EY_ROW_WAVES_ON, EY_ROW_WAVES_AUTO = 2, 0, 1, 2
EY_OPT_MAX_CHUNK_CHAINS = 3
EY_PRIOR_NORMAL, EY_PRIOR_LAPLACE, EY_PRIOR_STUDENT_T = 0, 1, 2
EY_LIK_BCE_SUM, EY_LIK_CE_SUM, EY_LIK_GAUSS_SUM, EY_LIK_LAPLACE_SUM, EY_LIK_POISSON_SUM = 0, 1, 2, 3, 4

# The arguments every sampler entry point ends with.  _DRAW: temp, C, seed, iter, chain_offset, flags; a step goes on with
# accepted, log_rate (_STEP), a run with n_iters, samples, targets, accepted_rec, accept_count, accepted (_RUN); then the
# stream.  _AM: plan, theta, target and the state and settings of the AM entry points.
_DRAW = [_vp, _i64, _u64, _u64, _u64, _u32]
_STEP = _DRAW + [_vp] * 3
_RUN = _DRAW + [_i] + [_vp] * 6
_AM = [_vp] * 8 + [_i, _d, _d, _d, _d, _i64, _i64, _i64]

SYMBOLS = {
    "ey_version": (_i, []),
    "ey_last_error": (ct.c_char_p, []),
    "ey_plan_create": (_i, [ct.POINTER(_vp), _i, ct.POINTER(_i), ct.POINTER(_i), ct.POINTER(_i), _i, _i, _i]),
    "ey_plan_create_mixture": (_i, [ct.POINTER(_vp), _i64, _i, ct.POINTER(_d), ct.POINTER(_d), ct.POINTER(_d), _i, _i]),
    "ey_plan_create_exptilt": (_i, [ct.POINTER(_vp), _i64, ct.POINTER(_d), ct.POINTER(_d), ct.POINTER(_d), ct.POINTER(_d), _i,
                                    _i]),
    "ey_plan_destroy": (_i, [_vp]),
    "ey_plan_num_params": (_i, [_vp, ct.POINTER(_i64)]),
    "ey_plan_kernel": (ct.c_char_p, [_vp]),
    "ey_plan_set_data": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "ey_plan_set_prior": (_i, [_vp, _vp, _vp, _vp]),
    "ey_plan_set_prior_family": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "ey_plan_prior_family": (_i, [_vp]),
    "ey_plan_set_lik_scale": (_i, [_vp, _d]),
    "ey_plan_lik_scale": (_d, [_vp]),
    "ey_forward": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "ey_log_target": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "ey_log_target_grad": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "ey_hmc_step": (_i, [_vp] * 6 + [_d, _vp, _i] + _DRAW + [_vp] * 5),
    "ey_hmc_leapfrog": (_i, [_vp, _vp, _vp, _d, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    "ey_mala_step": (_i, [_vp] * 6 + [_d, _vp] + _STEP),
    "ey_mh_step": (_i, [_vp] * 6 + _STEP),
    "ey_pt_swap_decide": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "ey_pt_ladder_create": (_i, [_vp, _vp, _i, _i, ct.POINTER(_vp)]),
    "ey_pt_ladder_destroy": (_i, [_vp]),
    "ey_pt_between": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ey_philox_normal": (_i, [_vp, _i64, _i64, _u64, _u64, _u64, _i, _vp]),
    "ey_philox_uniform": (_i, [_vp, _i64, _u64, _u64, _u64, _i, _vp]),
    "ey_philox_block": (_i, [ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_uint32)]),
    "ey_stats_update": (_i, [_vp, _vp, _i64, _i64, _i, _vp, _vp, _vp, _vp]),
    "ey_plan_attach_moments": (_i, [_vp, _vp, _vp, _vp, _i64]),
    "ey_hmc_run": (_i, [_vp] * 4 + [_d, _vp, _i] + _RUN),
    "ey_mala_run": (_i, [_vp] * 4 + [_d, _vp] + _RUN),
    "ey_mh_run": (_i, [_vp] * 4 + _RUN),
    "ey_log_lik_rows": (_i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "ey_ram_step": (_i, [_vp] * 6 + [_d, _d, _u64] + _STEP),
    "ey_ram_run": (_i, [_vp] * 4 + [_d, _d, _u64] + _RUN),
    "ey_mh_tril_step": (_i, [_vp] * 4 + [_i64] + [_vp] * 3 + _STEP),
    "ey_mh_tril_run": (_i, [_vp] * 4 + [_i64, _vp] + _RUN),
    "ey_mala_tril_step": (_i, [_vp] * 5 + [_i64] + [_vp] * 3 + [_d, _vp] + _STEP),
    "ey_mala_tril_run": (_i, [_vp] * 5 + [_i64, _vp, _d, _vp] + _RUN),
    "ey_am_step": (_i, _AM + [_vp] * 3 + _STEP + [_vp] * 2),
    "ey_am_run": (_i, _AM + _RUN + [_vp]),
    "ey_am_softabs_step": (_i, _AM + [_vp] * 3 + _STEP + [_vp] * 2),
    "ey_am_softabs_run": (_i, _AM + _RUN + [_vp]),
    "ey_am_softabs_fits": (_i, [_vp]),
    "ey_softabs": (_i, [_vp, _i64, _i64, _i, _d, _vp, _vp, _vp]),
    "ey_gibbs_table_create": (_i, [ct.POINTER(_vp), _i64, _i, _vp, _vp, _vp, _i, _i]),
    "ey_gibbs_table_destroy": (_i, [_vp]),
    "ey_gibbs_step": (_i, [_vp] * 6 + _STEP),
    "ey_gibbs_run": (_i, [_vp] * 4 + _RUN),
    "ey_philox_uniform_blocks": (_i, [_vp, _i64, _i64, _u64, _u64, _u64, _i, _vp]),
    "ey_inse_univariate": (_i, [_vp, _i64, _i64, _i, _vp, _vp, _vp, _vp]),
    "ey_plan_attach_da": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _d, _d, _i]),
    "ey_inse_multivariate": (_i, [_vp, _i64, _i64, _i64, _i64, _i64, _i, _vp, _vp, _vp, _vp, _vp]),
    "ey_kernel_pair_sums": (_i, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i, _i, ct.POINTER(_d),
                                 ct.POINTER(_i64), ct.POINTER(_i64), _i64, _i, _vp, _vp, _vp, _vp]),
    "ey_debug_mmd_last_split": (_i, []),
    "ey_debug_set_variant": (_i, [_i]),
    "ey_plan_set_variant": (_i, [_vp, _i]),
    "ey_plan_set_option": (_i, [_vp, _i, _i]),
    "ey_plan_get_option": (_i, [_vp, _i, ct.POINTER(ct.c_int)]),
    "ey_debug_bgemm": (_i, [_vp, _vp, _vp, _i, _i, _i] + [_i64] * 9 + [_vp, _i64, _i, _i, _vp]),
}

# ... and every symbol include/eeyore_amd_ext.h declares, the entry points added since that surface was recorded: a table of
# its own, bound by lib() beside SYMBOLS
EY_METRIC_DIAG, EY_METRIC_TRIL = 0, 1
EXT_SYMBOLS = {
    "ey_hmc_metric_step": (_i, [_vp] * 5 + [_i, _i64] + [_vp] * 3 + [_d, _vp, _i] + _DRAW + [_vp] * 5),
    "ey_hmc_metric_run": (_i, [_vp] * 5 + [_i, _i64, _vp, _d, _vp, _i] + _RUN),
}

# ... and what include/eeyore_amd_warmup.h declares, the warm-up of HMC under a metric: a third table, bound by lib() beside
# the other two.  ey_hmc_metric_warmup: ey_hmc_metric_run's arguments, then da_state, da_table, da_n, d, log_eub, final_avg,
# mean, M2, count, steps_rec, rate_rec before the stream.
WARMUP_SYMBOLS = {
    "ey_hmc_metric_warmup": (_i, [_vp] * 5 + [_i, _i64, _vp, _d, _vp, _i] + _RUN[:-1]
                             + [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _i64, _vp, _vp, _vp]),
    "ey_metric_from_moments": (_i, [_vp, _vp, _i64, _i64, _i64, _i, _i, _i, _vp, _vp, _vp]),
}

# ... and what include/eeyore_amd_nuts.h declares, the No-U-Turn sampler under a metric: a fourth table.  The outputs of a
# draw (_NUTS_OUT) follow accepted: depth, n_leapfrog, divergent, accept_stat, energy; a run adds depth_rec, divergent_rec;
# the warm-up then takes ey_hmc_metric_warmup's tail.
EY_NUTS_MAX_DEPTH = 10
_NUTS_OUT = [_vp] * 5
NUTS_SYMBOLS = {
    "ey_nuts_step": (_i, [_vp] * 5 + [_i, _i64] + [_vp] * 3 + [_i64, _d, _vp, _i] + _DRAW + [_vp] + _NUTS_OUT + [_vp]),
    "ey_nuts_run": (_i, [_vp] * 5 + [_i, _i64, _vp, _d, _vp, _i] + _RUN[:-1] + _NUTS_OUT + [_vp] * 3),
    "ey_nuts_warmup": (_i, [_vp] * 5 + [_i, _i64, _vp, _d, _vp, _i] + _RUN[:-1] + _NUTS_OUT + [_vp] * 2
                       + [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _i64, _vp, _vp, _vp]),
}

# ... and what include/eeyore_amd_eslice.h declares, elliptical slice sampling: a fifth table.  A step takes theta, target,
# ell, base_loc, base_scale, z, u, S, max_shrinks before _DRAW and accepted, n_evals after it; a run adds n_evals_rec.
EY_ESLICE_MAX_SHRINKS = 64
ESLICE_SYMBOLS = {
    "ey_eslice_ell": (_i, [_vp] * 5 + [_i64] + [_vp] * 3),
    "ey_eslice_step": (_i, [_vp] * 8 + [_i64, _i] + _DRAW + [_vp] * 3),
    "ey_eslice_run": (_i, [_vp] * 6 + [_i] + _RUN + [_vp] * 2),
}

# ... and what include/eeyore_amd_eslice_fused.h declares, a sixth table: which kernel serves elliptical slice sampling on a
# plan under given flags, b"mfma32" (the fused form on the matrix cores) or b"generic"
ESLICE_FUSED_SYMBOLS = {
    "ey_eslice_kernel": (ct.c_char_p, [_vp, _u32]),
}

# ... and what include/eeyore_amd_nuts_tree.h declares, a seventh table: the tree of NUTS in a device workspace.
# EY_NUTS_TREE_DEVICE is a bit of the flags of the three NUTS entry points.
EY_NUTS_TREE_DEVICE = 8
NUTS_TREE_SYMBOLS = {
    "ey_nuts_tree_bytes": (_i64, [_vp, _i64, _i]),
    "ey_plan_attach_nuts_tree": (_i, [_vp, _vp, _i64]),
}

# ... and what include/eeyore_amd_nuts_fused.h declares, an eighth table: NUTS on the matrix cores for the plans of the mfma32
# family.  EY_NUTS_FUSED is a bit of the flags of the three NUTS entry points (it implies EY_NUTS_TREE_DEVICE);
# ey_nuts_kernel says which kernel serves a plan under given flags, b"mfma32" or b"generic".
EY_NUTS_FUSED = 16
NUTS_FUSED_SYMBOLS = {
    "ey_nuts_kernel": (ct.c_char_p, [_vp, _u32]),
}

# ... and what include/eeyore_amd_hmc_metric_fused.h declares, a ninth table: HMC under a diagonal metric and its warm-up on
# the matrix cores for the plans of the mfma32 family.  EY_HMC_METRIC_FUSED is a bit of the flags of ey_hmc_metric_step /
# ey_hmc_metric_run / ey_hmc_metric_warmup; ey_hmc_metric_kernel says which kernel serves a plan under given flags,
# b"mfma32" or b"generic".
EY_HMC_METRIC_FUSED = 32
HMC_METRIC_FUSED_SYMBOLS = {
    "ey_hmc_metric_kernel": (ct.c_char_p, [_vp, _u32]),
}


def build(force=False, verbose=False, diagnostics=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU).  ``diagnostics``: also the fused16
    family once more at -O1 (the build that computed wrong results before the hazard pass), on which
    tests/test_fused16.py runs its oracle suite -- a diagnostic library: a compiler failure that only -O1 shows must not
    fail the build of the production library, so it is not part of the default build (the test builds it when missing)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=out)
    if diagnostics:
        subprocess.check_call(["make", "-C", CSRC, "-j4", "o1"], stdout=out)
    return LIB_PATH


O1_LIB_PATH = os.path.join(HERE, "lib", "libeeyore_amd_f16o1.so")
SPILL_LIB_DIR = os.path.join(HERE, "lib")  # `make spill`: diagnostic builds libeeyore_amd_spill_<unit>.so


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"eeyore_amd: HIP library {LIB_PATH} is missing -- run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C eeyore_amd/csrc`); there is no CPU fallback")
        L = ct.CDLL(LIB_PATH)
        for name, (res, args) in (list(SYMBOLS.items()) + list(EXT_SYMBOLS.items()) + list(WARMUP_SYMBOLS.items())
                                  + list(NUTS_SYMBOLS.items()) + list(ESLICE_SYMBOLS.items())
                                  + list(ESLICE_FUSED_SYMBOLS.items()) + list(NUTS_TREE_SYMBOLS.items())
                                  + list(NUTS_FUSED_SYMBOLS.items()) + list(HMC_METRIC_FUSED_SYMBOLS.items())):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().ey_last_error().decode()
        if rc == -1:
            raise ValueError(f"eeyore_amd {what}: {msg}")
        raise RuntimeError(f"eeyore_amd {what}: {msg} (status {rc})")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ct.c_void_p(t.data_ptr())
