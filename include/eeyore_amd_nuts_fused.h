/* eeyore_amd_nuts_fused.h -- NUTS on the matrix cores for the MLP(4-32-32-dK) plans: the tree in the device workspace,
 * every leaf on the fused evaluation.
 *
 * An eighth header beside the other seven, under the same conventions.  Include this header alone: it includes the other
 * seven.
 *
 * With the bit EY_NUTS_FUSED in `flags` and form == EY_METRIC_DIAG, ey_nuts_step / ey_nuts_run / ey_nuts_warmup
 * (eeyore_amd_nuts.h) run on k_nuts_mfma for the f32 plans whose ey_plan_kernel is "mfma32" (DESIGN.md 4.28): the same draw,
 * decision for decision on the same Philox words and block words, the same outputs, records and warm-up epilogues, every
 * leapfrog step evaluated by the fused evaluation of that family.  The two kernels add the same terms in different orders, so
 * values agree to rounding and a decision whose margin is of rounding size may differ.
 *
 * The tree lives in the workspace of eeyore_amd_nuts_tree.h, with the size ey_nuts_tree_bytes reports and under the same
 * rules: the bit implies EY_NUTS_TREE_DEVICE, and a call may carry both.  A call without the bit runs what it ran before.
 *
 * With the bit, before anything is launched or written --
 * EY_ERR_INVALID: form == EY_METRIC_TRIL; EY_FORCE_GENERIC in the same flags; no workspace attached, or one smaller than
 * ey_nuts_tree_bytes(plan, C, max_depth) of this call.
 * EY_ERR_UNSUPPORTED: a plan the mfma32 family does not serve with the batch it holds (another shape, dtype or prior
 * family, more rows than its data image takes): ey_plan_kernel says which family does.
 */
#ifndef EEYORE_AMD_NUTS_FUSED_H
#define EEYORE_AMD_NUTS_FUSED_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"
#include "eeyore_amd_warmup.h"
#include "eeyore_amd_nuts.h"
#include "eeyore_amd_eslice.h"
#include "eeyore_amd_eslice_fused.h"
#include "eeyore_amd_nuts_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a bit of `flags` of the three NUTS entry points, beside EY_NUTS_TREE_DEVICE (8) */
#define EY_NUTS_FUSED 16

/* The kernel ey_nuts_step / ey_nuts_run / ey_nuts_warmup take on this plan with these flags: "mfma32" (k_nuts_mfma) when
 * the flags carry EY_NUTS_FUSED without EY_FORCE_GENERIC and the plan is served by the mfma32 family, otherwise "generic"
 * (k_nuts, k_nuts_ws).  A static string; "generic" for a NULL plan. */
const char* ey_nuts_kernel(const ey_plan* plan, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_NUTS_FUSED_H */
