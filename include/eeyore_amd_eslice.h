/* eeyore_amd_eslice.h -- elliptical slice sampling: the entry points behind samplers.EllipticalSlice.
 *
 * A fifth header beside eeyore_amd.h, eeyore_amd_ext.h (the fixed metric), eeyore_amd_warmup.h (its warm-up) and
 * eeyore_amd_nuts.h (the No-U-Turn sampler), under the same conventions: status codes, device pointers of the plan's
 * dtype, a HIP stream as the last argument, ey_last_error for the message.  Include this header alone: it includes the
 * other four.
 *
 * One draw is the transition of Murray, Adams & MacKay (2010) for a target N(m, diag s^2) x exp(ell): nu ~ N(0, diag s^2),
 * a slice height log y = ell(theta) + log u_0, and points theta' = m + (theta - m) cos(2 pi a) + nu sin(2 pi a) on the
 * ellipse through theta and m + nu, the angle a (in turns) drawn from a bracket that shrinks towards 0 until
 * ell(theta') > log y.  No free parameter, no rejection, no gradient: one value-only evaluation per point.
 *
 * The Gaussian base N(m, diag s^2) and ell:
 *  base_loc = base_scale = NULL   the plan's own Normal prior: m = mu, s = sigma / sqrt(t) under a temperature t (the
 *                                 reference tempers likelihood and prior alike, and N(mu, sigma^2)^t ~ N(mu, sigma^2 / t));
 *                                 ell is the (tempered) log-likelihood
 *  base_loc, base_scale [P]       any plan: ell = (tempered) log-target - sum_i -((theta_i - m_i) / s_i)^2 / 2; the base
 *                                 is not tempered and its constant is dropped
 *
 * EY_ESLICE_MAX_SHRINKS caps max_shrinks.  After max_shrinks shrinks without a point on the slice the chain stays where it
 * is: the truncated transition is still reversible.
 *
 * The uniform stream of (seed, chain, iteration) is read at these block words (ey_philox_uniform_blocks' index):
 *   0        u_0: the slice height
 *   1        u_1: the first angle, a = u_1, with the bracket [a - 1, a]
 *   2 + k    the k-th shrink: a = lo + (hi - lo) u
 * The layout does not depend on max_shrinks, so changing max_shrinks moves no variate.
 */
#ifndef EEYORE_AMD_ESLICE_H
#define EEYORE_AMD_ESLICE_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"
#include "eeyore_amd_warmup.h"
#include "eeyore_amd_nuts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EY_ESLICE_MAX_SHRINKS 64

/* ell [C] and the (tempered) log-target [C] at theta [C,P]: the value-only evaluation ey_eslice_step makes, used to start a
 * chain and after a minibatch change.  Either output may be NULL.  Refusals as ey_eslice_step's about the base. */
int ey_eslice_ell(ey_plan* plan, const void* theta, const void* base_loc, const void* base_scale, const void* temp,
                  int64_t C, void* ell, void* target, void* stream);

/* One draw of every chain.  theta [C,P], target [C] and ell [C] are in/out: the state, its (tempered) log-target and ell.
 *  z [C,P] or NULL: the standard normals behind nu (NULL: the chain's normal stream, as ey_mh_step);
 *  u [C,S] or NULL: the uniforms of the draw in the word layout above, S >= 2 + max_shrinks (NULL: the chain's uniform
 *    stream; S is then ignored);
 *  max_shrinks in [1, EY_ESLICE_MAX_SHRINKS]: a draw makes at most max_shrinks + 1 evaluations.
 * Outputs [C]: accepted uint8, 1 iff the chain moved; n_evals int32 (may be NULL), the evaluations made.  A chain whose
 * carried ell is not finite stays put without evaluating (n_evals = 0).
 * EY_ERR_INVALID, before anything is launched or written: base_loc = base_scale = NULL on a plan whose prior is not Normal
 *  or on a distribution plan; only one of the two base tables; max_shrinks out of range; u with S too small; a plan with
 *  ey_plan_attach_da attached.
 * EY_ERR_UNSUPPORTED, before any launch: an LDS image beyond 160 KiB (the message has the byte count).  There is no limit on
 *  the number of parameters otherwise. */
int ey_eslice_step(ey_plan* plan, void* theta, void* target, void* ell, const void* base_loc, const void* base_scale,
                   const void* z, const void* u, int64_t S, int max_shrinks, const void* temp, int64_t C, uint64_t seed,
                   uint64_t iter, uint64_t chain_offset, uint32_t flags, void* accepted, void* n_evals, void* stream);

/* n_iters draws (iterations iter, iter + 1, ...) in one launch on the chains' own streams: bit-identical to n_iters calls
 * of ey_eslice_step with z = u = NULL.  The records of ey_mh_run (samples, targets, accepted_rec, accept_count), accepted and
 * n_evals of the last draw, and n_evals_rec [n_iters,C] int32 or NULL.  Attached moments accumulate as in ey_mh_run. */
int ey_eslice_run(ey_plan* plan, void* theta, void* target, void* ell, const void* base_loc, const void* base_scale,
                  int max_shrinks, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                  uint32_t flags, int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count,
                  void* accepted, void* n_evals, void* n_evals_rec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_ESLICE_H */
