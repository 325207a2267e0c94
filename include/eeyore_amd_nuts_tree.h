/* eeyore_amd_nuts_tree.h -- NUTS beyond 128 parameters: the tree in a device workspace, for the diagonal metric.
 *
 * A seventh header beside the other six, under the same conventions.  Include this header alone: it includes the other six.
 *
 * ey_nuts_step / ey_nuts_run / ey_nuts_warmup (eeyore_amd_nuts.h) keep the 12 + 2 EY_NUTS_MAX_DEPTH vectors of a chain's
 * tree in LDS and therefore stop at P = 128.  With the bit EY_NUTS_TREE_DEVICE in `flags` and form == EY_METRIC_DIAG they
 * run on a sibling kernel whose tree lives in a workspace the caller has attached to the plan: the same draw, decision for
 * decision on the same Philox words and with the same sums in the same order (at P <= 128 the same bits), for any P whose
 * evaluation image fits LDS as ey_hmc_metric_step's diagonal form needs it.  Small P is served too.
 *
 * The workspace of one call holds 12 + 2 max_depth vectors of P rounded up to 64 elements of the plan's dtype per chain.
 * It need not be initialised and carries nothing from one call to the next; a workspace larger than a call needs serves
 * it.  Two calls that run at the same time on one plan (on two streams) need a plan each: the plan holds one workspace.
 *
 * With the flag, EY_ERR_INVALID before anything is launched or written: form == EY_METRIC_TRIL; no workspace attached; an
 * attached workspace smaller than ey_nuts_tree_bytes(plan, C, max_depth) of this call (the message has both counts).
 * EY_ERR_UNSUPPORTED: an evaluation image beyond 160 KiB.  Without the flag an attached workspace changes nothing.
 */
#ifndef EEYORE_AMD_NUTS_TREE_H
#define EEYORE_AMD_NUTS_TREE_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"
#include "eeyore_amd_warmup.h"
#include "eeyore_amd_nuts.h"
#include "eeyore_amd_eslice.h"
#include "eeyore_amd_eslice_fused.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a bit of `flags` of the three NUTS entry points, beside EY_RECOMPUTE_INITIAL_GRAD (1), EY_FORCE_GENERIC (2) and
 * EY_GIBBS_CARRY (4) */
#define EY_NUTS_TREE_DEVICE 8

/* The bytes of the workspace for C chains at max_depth: C (12 + 2 max_depth) ((P + 63) & ~63) element sizes.
 * Negative (EY_ERR_INVALID) for a null plan, C < 0 or max_depth outside [1, EY_NUTS_MAX_DEPTH]. */
int64_t ey_nuts_tree_bytes(const ey_plan* plan, int64_t C, int max_depth);

/* Attaches `bytes` bytes of device memory at ws (aligned to the plan's dtype) as the tree's workspace; ws == NULL
 * detaches.  The plan does not own the memory: it must stay valid until it is detached or replaced, or the plan is
 * destroyed.  EY_ERR_INVALID: a null plan, or ws != NULL with bytes <= 0 or not aligned to the plan's dtype. */
int ey_plan_attach_nuts_tree(ey_plan* plan, void* ws, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_NUTS_TREE_H */
