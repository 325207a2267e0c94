/* eeyore_amd_ext.h -- entry points added to the C ABI of libeeyore_amd.so after eeyore_amd.h was recorded.
 *
 * eeyore_amd.h is the surface the fixtures of the test suite pin, name by name; what the library has gained since is
 * declared here, under the same conventions (status codes, device pointers of the plan's dtype, a HIP stream as the last
 * argument, ey_last_error for the message).  Include this header alone: it includes eeyore_amd.h.
 */
#ifndef EEYORE_AMD_EXT_H
#define EEYORE_AMD_EXT_H

#include "eeyore_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the form of a fixed HMC metric: L = diag(s), or a lower-triangular factor L */
enum ey_metric_form { EY_METRIC_DIAG = 0, EY_METRIC_TRIL = 1 };

/* One HMC draw for C chains under a FIXED Euclidean metric with inverse Sigma = L L^T: momentum p ~ N(0, Sigma^-1),
 * K(p) = p^T Sigma p / 2.  Written in the whitened velocity v = L^T p, which needs no solve:
 *   v ~ N(0, I);  H_cur = -target + |v|^2 / 2;  v += step/2 L^T grad;
 *   L times:  theta += step L v;  (target, grad) at theta;  v += w L^T grad  (w = step, on the last step step / 2);
 *   H_prop = -target + |v|^2 / 2;  accept iff u < min(exp(H_cur - H_prop), 1)  (strict; a NaN rate rejects).
 * With L = I this is ey_hmc_step's draw on the same random numbers.
 *  theta, target, grad, u, step, step_vec, L, temp, seed, iter, chain_offset, accepted, accept_rate, H_cur, H_prop:
 *    ey_hmc_step's.  flags: EY_RECOMPUTE_INITIAL_GRAD as there, the others are ignored;
 *  v0 [C,P] replaces the draw of v (NULL => the in-kernel Philox stream ey_hmc_step draws its momentum from);
 *  metric, form: EY_METRIC_TRIL: [G,P,P] row-major lower-triangular factors with a positive diagonal, only j <= i of a
 *    factor is read (the strict upper triangle may hold anything), P <= 128; EY_METRIC_DIAG: [G,P] scales s > 0, L = diag(s),
 *    any P the generic kernels hold.  A device array of the plan's dtype, read only, staged once per launch;
 *  G, metric_index: which entry a chain uses, as ey_mh_tril_step's tril_index: G == 1, the one entry; metric_index == NULL,
 *    chain c uses entry c (G == C); otherwise entry metric_index[c] (device int32 [C]), clamped into [0, G) -- checking
 *    its range is the caller's business.
 * EY_ERR_INVALID: a null theta / target / grad / metric / accepted, an unknown form, L < 1, n_iters < 1, G < 1,
 * metric_index == NULL with G neither 1 nor C, step <= 0 without step_vec, a plan with a dual-averaging table attached
 * (ey_plan_attach_da: this kernel does not consume it).  Served by one kernel of the generic family for every model, whatever
 * ey_plan_kernel reports (which the call leaves as it is), mixture and exponential-tilt plans included.
 * EY_ERR_UNSUPPORTED, before any launch and with nothing written: EY_METRIC_TRIL with P > 128 or a factor that does not fit
 * beside the evaluation image in LDS; EY_METRIC_DIAG on a model whose generic LDS image does not fit a CU.
 * Attached moments are accumulated as ey_mala_tril_step accumulates them. */
int ey_hmc_metric_step(ey_plan* plan, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                       const void* metric_index, const void* v0, const void* u, double step, const void* step_vec, int L,
                       const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                       void* accepted, void* accept_rate, void* H_cur, void* H_prop, void* stream);

/* n_iters iterations in one launch (the metric is staged once), records as ey_hmc_run; ey_hmc_metric_run is bit-identical
 * to n_iters calls of ey_hmc_metric_step with v0 = u = NULL. */
int ey_hmc_metric_run(ey_plan* plan, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                      const void* metric_index, double step, const void* step_vec, int L, const void* temp, int64_t C,
                      uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                      void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_EXT_H */
