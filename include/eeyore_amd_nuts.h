/* eeyore_amd_nuts.h -- the No-U-Turn sampler under a fixed metric: the entry points behind samplers.NUTS.
 *
 * A fourth header beside eeyore_amd.h, eeyore_amd_ext.h (the fixed metric) and eeyore_amd_warmup.h (its warm-up), under the
 * same conventions: status codes, device pointers of the plan's dtype, a HIP stream as the last argument, ey_last_error for
 * the message.  Include this header alone: it includes the other three.
 *
 * One draw is multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017) in ey_hmc_metric_step's whitened velocity
 * v = L^T p: the tree doubles backward or forward until the generalised U-turn criterion v_first . rho > 0 and
 * v_last . rho > 0 (rho the sum of v over a span's leaves) fails between the tree's edges or inside an aligned block of
 * the new subtree, a leaf's energy error exceeds 1000 (a divergent draw), or max_depth doublings are made.  A new
 * subtree's candidate is drawn leaf by leaf with probability weight / (weights so far); it replaces the tree's proposal
 * with probability min(1, W_new / W_old).  DESIGN.md 4.24 states every decision.
 *
 * EY_NUTS_MAX_DEPTH caps max_depth: at most 2^10 - 1 leapfrog steps a draw.
 *
 * The uniform stream of (seed, chain, iteration) is read at these block words (ey_philox_uniform_blocks' index):
 *   0                               unused (the accept variate of ey_hmc_metric_step)
 *   1 + 2 d                         the direction of doubling d: < 0.5 backward, otherwise forward
 *   2 + 2 d                         u_top(d): the tree takes the new subtree's candidate
 *   1 + 2 EY_NUTS_MAX_DEPTH + n     u_leaf(n): leaf n of the draw (n counts from 0 over all subtrees) becomes the candidate
 * The layout uses the cap, not max_depth, so changing max_depth moves no variate.
 */
#ifndef EEYORE_AMD_NUTS_H
#define EEYORE_AMD_NUTS_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"
#include "eeyore_amd_warmup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EY_NUTS_MAX_DEPTH 10

/* One NUTS draw of every chain.  The arguments of ey_hmc_metric_step with max_depth in [1, EY_NUTS_MAX_DEPTH] for L;
 *  v0 [C,P] or NULL: the whitened velocity of the draw (NULL: the chain's normal stream, as ey_hmc_metric_step);
 *  u [C,S] or NULL: the uniforms of the draw in the word layout above, S >= 1 + 2 EY_NUTS_MAX_DEPTH + 2^max_depth
 *    (NULL: the chain's uniform stream; S is then ignored);
 *  both metric forms: P <= 128.
 * Outputs [C], each may be NULL except accepted:
 *  accepted uint8: 1 iff the state moved;  depth int32: the doublings kept (a discarded subtree does not count);
 *  n_leapfrog int32: the leaves whose weight was taken (a divergent leaf is not among them);  divergent uint8;
 *  accept_stat: the mean of min(1, exp(H_0 - H_leaf)) over those leaves (0 when there are none);
 *  energy: the Hamiltonian at the state the chain is left in, with the draw's velocity there.
 * EY_ERR_INVALID, before anything is launched or written: what ey_hmc_metric_step refuses (a plan with ey_plan_attach_da
 *  attached among them), max_depth outside [1, EY_NUTS_MAX_DEPTH], u with S too small.
 * EY_ERR_UNSUPPORTED, before any launch: P > 128, or an LDS image beyond 160 KiB (the message has the byte count). */
int ey_nuts_step(ey_plan* plan, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                 const void* metric_index, const void* v0, const void* u, int64_t S, double step, const void* step_vec,
                 int max_depth, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                 uint32_t flags, void* accepted, void* depth, void* n_leapfrog, void* divergent, void* accept_stat,
                 void* energy, void* stream);

/* n_iters draws (iterations iter, iter + 1, ...) in one launch on the chains' own streams: bit-identical to n_iters calls
 * of ey_nuts_step with v0 = u = NULL.  The arguments of ey_hmc_metric_run with max_depth for L, the outputs of
 * ey_nuts_step (of the last draw), and two more records: depth_rec [n_iters,C] int32, divergent_rec [n_iters,C] uint8,
 * or NULL. */
int ey_nuts_run(ey_plan* plan, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                const void* metric_index, double step, const void* step_vec, int max_depth, const void* temp, int64_t C,
                uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                void* targets, void* accepted_rec, void* accept_count, void* accepted, void* depth, void* n_leapfrog,
                void* divergent, void* accept_stat, void* energy, void* depth_rec, void* divergent_rec, void* stream);

/* ey_nuts_run with the two optional epilogues of ey_hmc_metric_warmup after each draw -- dual averaging of each chain's
 * step and Welford moments of the state it is left in -- where the rate of a draw is its accept_stat.  The arguments from
 * da_state on, and what is refused about them, are ey_hmc_metric_warmup's; rate_rec records accept_stat.  With all of
 * them NULL the call leaves the bits of ey_nuts_run. */
int ey_nuts_warmup(ey_plan* plan, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                   const void* metric_index, double step, void* step_vec, int max_depth, const void* temp, int64_t C,
                   uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                   void* targets, void* accepted_rec, void* accept_count, void* accepted, void* depth, void* n_leapfrog,
                   void* divergent, void* accept_stat, void* energy, void* depth_rec, void* divergent_rec, void* da_state,
                   const void* da_table, int da_n, double d, double log_eub, int final_avg, void* mean, void* M2,
                   int64_t count, void* steps_rec, void* rate_rec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_NUTS_H */
