/* eeyore_amd_hmc_metric_fused.h -- HMC under a diagonal metric, and its warm-up, on the matrix cores for the
 * MLP(4-32-32-dK) plans: every leapfrog step on the fused evaluation.
 *
 * A ninth header beside the other eight, under the same conventions.  Include this header alone: it includes the other
 * eight.
 *
 * With the bit EY_HMC_METRIC_FUSED in `flags` and form == EY_METRIC_DIAG, ey_hmc_metric_step / ey_hmc_metric_run
 * (eeyore_amd_ext.h) and ey_hmc_metric_warmup (eeyore_amd_warmup.h) run on k_hmc_metric_mfma for the f32 plans whose
 * ey_plan_kernel is "mfma32" (DESIGN.md 4.29): the same draw on the same Philox words and streams, the same inputs (v0, u,
 * temp, step_vec, metric_index / G, chain_offset, EY_RECOMPUTE_INITIAL_GRAD), the same outputs, records and warm-up
 * epilogues, every leapfrog step evaluated by the fused evaluation of that family.  The two kernels add the same terms in
 * different orders, so values agree to rounding and a decision whose margin is of rounding size may differ.  A rejected
 * chain's theta, target and gradient are not written.  A call without the bit runs what it ran before, bit for bit.
 *
 * With the bit, after every refusal the three entry points make without it and before anything is launched or written --
 * EY_ERR_INVALID: form == EY_METRIC_TRIL (diagonal metric only); EY_FORCE_GENERIC in the same flags.
 * EY_ERR_UNSUPPORTED: a plan the mfma32 family does not serve with the batch it holds (another shape, dtype or prior
 * family, more rows than its data image takes): the message names ey_plan_kernel and what it says.
 */
#ifndef EEYORE_AMD_HMC_METRIC_FUSED_H
#define EEYORE_AMD_HMC_METRIC_FUSED_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"
#include "eeyore_amd_warmup.h"
#include "eeyore_amd_nuts.h"
#include "eeyore_amd_eslice.h"
#include "eeyore_amd_eslice_fused.h"
#include "eeyore_amd_nuts_tree.h"
#include "eeyore_amd_nuts_fused.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a bit of `flags` of ey_hmc_metric_step / ey_hmc_metric_run / ey_hmc_metric_warmup (1, 2, 4, 8 and 16 are taken) */
#define EY_HMC_METRIC_FUSED 32

/* The kernel ey_hmc_metric_step / ey_hmc_metric_run / ey_hmc_metric_warmup take on this plan with these flags under a
 * diagonal metric: "mfma32" (k_hmc_metric_mfma) when the flags carry EY_HMC_METRIC_FUSED without EY_FORCE_GENERIC and the
 * plan is served by the mfma32 family, otherwise "generic" (k_hmc_metric, k_hmc_metric_warmup).  A static string; "generic"
 * for a NULL plan. */
const char* ey_hmc_metric_kernel(const ey_plan* plan, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_HMC_METRIC_FUSED_H */
