/* eeyore_amd_warmup.h -- the warm-up of HMC under a metric: the entry points behind tuners.WindowedAdaptation.
 *
 * A third header beside eeyore_amd.h (the surface the fixtures pin) and eeyore_amd_ext.h (the fixed metric), under the same
 * conventions: status codes, device pointers of the plan's dtype, a HIP stream as the last argument, ey_last_error for the
 * message.  Include this header alone: it includes the other two.
 *
 * A warm-up is a handful of launches of ey_hmc_metric_warmup -- draws that adapt each chain's step by dual averaging and
 * accumulate each chain's running moments where the draws are made -- with ey_metric_from_moments between them, which
 * turns the moments into the next metric.  No draw is stored and nothing is read back between draws.
 */
#ifndef EEYORE_AMD_WARMUP_H
#define EEYORE_AMD_WARMUP_H

#include "eeyore_amd.h"
#include "eeyore_amd_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_iters draws of ey_hmc_metric_run in one launch, with two optional epilogues after each draw's accept step.  Every
 * argument up to `accepted` is ey_hmc_metric_run's, except that step_vec is in/out when a dual averaging is given.  With
 * da_state, mean, M2, steps_rec and rate_rec all NULL the call leaves the bits of ey_hmc_metric_run.
 *
 * Dual averaging per chain (Hoffman & Gelman 2014, algorithm 5; the recurrence of ey_plan_attach_da, as arguments of the
 * call and not state of the plan):
 *  da_state [C,3] double, in/out: (barh, logbare, mu) per chain; NULL: the steps stay what they are;
 *  da_table [da_n,3] double on the device: (1/(t + t0), sqrt(t)/gamma, t^-kappa) for this launch's first da_n draws, worked
 *    out by the caller; draws beyond da_n keep the last step;
 *  d, log_eub (NaN: none), final_avg: as ey_plan_attach_da's; final_avg != 0: draw da_n - 1 of the launch leaves the
 *    averaged step exp(logbare);
 *  step_vec [C] of the plan's dtype: the step of the launch's first draw; after each adapting draw the step of the next
 *    one is written there, and is the step of the next draw in the same launch.
 *
 * Running moments of the state each chain is left in (a rejected draw counts its old state again), Welford's update in
 * double whatever the plan's dtype: with n the count including this draw and dlt = x - mean,
 *    mean += dlt / n;   EY_METRIC_DIAG: M2[c,i] += ((n-1)/n) dlt_i^2;   EY_METRIC_TRIL: M2[c,i,j] += ((n-1)/n) dlt_i dlt_j, j <= i
 *  mean [C,P] double, in/out; M2 [C,P] (EY_METRIC_DIAG) or [C,P,P] (EY_METRIC_TRIL) double, in/out: the form is the
 *    metric's.  Only j <= i of a dense M2 is read or written: the strict upper triangle may hold anything and keeps it;
 *  count: the draws already in the accumulators (the same for all chains), so that a window may span launches.
 *  The order of every sum depends on P alone: no floating-point atomics.
 *
 * Records beside ey_hmc_metric_run's: steps_rec [n_iters,C] (the step each draw used) and rate_rec [n_iters,C] (its
 * acceptance rate min(exp(H_cur - H_prop), 1)), of the plan's dtype, or NULL.
 *
 * EY_ERR_INVALID, before anything is launched and with nothing written: every refusal of ey_hmc_metric_run, a plan with
 * ey_plan_attach_da attached among them, n_iters < 1, L < 1, da_state without da_table or with da_n < 1 or da_n > n_iters,
 * da_state without step_vec, exactly one of mean / M2 NULL, count < 0.  EY_ERR_UNSUPPORTED: as ey_hmc_metric_run
 * (EY_METRIC_TRIL with P > 128). */
int ey_hmc_metric_warmup(ey_plan* plan, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                         const void* metric_index, double step, void* step_vec, int L, const void* temp, int64_t C,
                         uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                         void* targets, void* accepted_rec, void* accept_count, void* accepted, void* da_state,
                         const void* da_table, int da_n, double d, double log_eub, int final_avg, void* mean, void* M2,
                         int64_t count, void* steps_rec, void* rate_rec, void* stream);

/* A metric table from running moments: Stan's regularised estimate, as samplers/metric.py defines it for draws.
 *  mean [C,P], M2 [C,P] (EY_METRIC_DIAG) or [C,P,P] (EY_METRIC_TRIL, only j <= i is read) double: the accumulators of
 *    ey_hmc_metric_warmup after n draws of every chain;
 *  pooled != 0: ONE estimate from all chains, N = C n draws: with gm = (1/C) sum_c mean_c,
 *    total = sum_c M2_c + n sum_c (mean_c - gm)(mean_c - gm)^T, every element summed over the chains in index order;
 *    table [P] or [P,P], status [1];
 *  pooled == 0: one estimate per chain, N = n, total = M2_c; table [C,P] or [C,P,P], status [C];
 *  then S = total / (N - 1), shrunk to N/(N+5) S + 1e-3 5/(N+5) I; EY_METRIC_DIAG: the square roots; EY_METRIC_TRIL: the
 *    Cholesky factor, worked in double in LDS (P <= 128); rounded once to dtype (EY_F32 / EY_F64), the strict upper
 *    triangle written as zero;
 *  status int32: 0 fine; 1 a non-finite input or a pivot that is not positive -- that entry of table is then left
 *    untouched, and no other entry is affected.
 * EY_ERR_INVALID before the device is touched: a NULL argument, an unknown form or dtype, C < 1, P < 1, N < 2.
 * EY_ERR_UNSUPPORTED: EY_METRIC_TRIL with P > 128.  Runs on the current device. */
int ey_metric_from_moments(const void* mean, const void* M2, int64_t n, int64_t C, int64_t P, int form, int pooled,
                           int dtype, void* table, void* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_WARMUP_H */
