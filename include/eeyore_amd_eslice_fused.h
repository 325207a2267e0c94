/* eeyore_amd_eslice_fused.h -- which kernel serves elliptical slice sampling on a plan.
 *
 * A sixth header beside eeyore_amd.h, eeyore_amd_ext.h, eeyore_amd_warmup.h, eeyore_amd_nuts.h and eeyore_amd_eslice.h,
 * under the same conventions.  Include this header alone: it includes the other five.
 *
 * ey_eslice_ell, ey_eslice_step and ey_eslice_run (eeyore_amd_eslice.h) run on the matrix cores for the f32
 * MLP(4-32-32-dK) plans whose ey_plan_kernel is "mfma32" (DESIGN.md 4.26): the same transition, the same streams and block
 * words, the same records and refusals, every point of the ellipse evaluated by the fused value-only evaluation.
 * EY_FORCE_GENERIC in a step's or a run's flags sends the call back to the generic kernel; ey_eslice_ell takes no flags and
 * follows the plan alone.  The two kernels add the same terms in different orders, so a carried ell should come from the
 * kernel that will compare against it: after switching flags, call ey_eslice_ell's counterpart or accept a difference of
 * rounding size in the first slice height.
 */
#ifndef EEYORE_AMD_ESLICE_FUSED_H
#define EEYORE_AMD_ESLICE_FUSED_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"
#include "eeyore_amd_warmup.h"
#include "eeyore_amd_nuts.h"
#include "eeyore_amd_eslice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The kernel ey_eslice_step / ey_eslice_run take on this plan with these flags: "mfma32" (k_eslice_mfma) or "generic"
 * (k_eslice).  A static string; "generic" for a NULL plan. */
const char* ey_eslice_kernel(const ey_plan* plan, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_ESLICE_FUSED_H */
