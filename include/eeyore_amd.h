/* eeyore_amd C ABI -- the drop-in boundary for the chain-batched MCMC hot path on MI355X (gfx950).
 *
 * The reference (papamarkou/eeyore v0.0.20) is pure Python and has no FFI: its boundary is the duck-typed
 * protocol between a sampler and a model.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - every `const void*` / `void*` data argument is a DEVICE pointer (torch.Tensor.data_ptr()) of the plan's
 *    dtype unless stated otherwise; the caller owns every buffer, the library never returns memory;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); compute entry points AND ey_plan_set_data
 *    are asynchronous on it (set_data: device-to-device copies and packing kernels on `stream`; it allocates -- and
 *    then synchronises the device -- only when a batch is larger than any before it); ey_plan_create /
 *    ey_plan_set_prior / ey_plan_destroy synchronise;
 *  - return value 0 = EY_OK, negative = ey_status; ey_last_error() gives a thread-local message;
 *  - parameters are flat `theta[C, P]`, chain-major, each row in nn.Module.parameters() order: per layer
 *    W_l [d_{l+1} x d_l] row-major then b_l (eeyore/models/model.py:38-55, eeyore/models/mlp.py:37-43);
 *  - C = 1 is the reference's single-chain case.
 *  - a plan is not thread-safe; distinct plans on distinct streams/devices are independent.
 */
#ifndef EEYORE_AMD_H
#define EEYORE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ey_plan ey_plan;
typedef struct ey_gibbs_table ey_gibbs_table;
typedef struct ey_pt_ladder ey_pt_ladder;

enum ey_status {
  EY_OK = 0,
  EY_ERR_INVALID = -1,      /* bad argument (ValueError in the reference, eeyore/models/mlp.py:15-19) */
  EY_ERR_UNSUPPORTED = -2,  /* model/shape outside what the kernels cover */
  EY_ERR_HIP = -3,          /* HIP runtime error (RuntimeError in the reference's benchmark(), serial_sampler.py:112) */
  EY_ERR_STATE = -4         /* data or prior not set */
};

/* activation codes: eeyore/models/mlp.py:9-13,45-50 (`None` or torch.sigmoid in every reference test/example) */
enum ey_act { EY_ACT_NONE = 0, EY_ACT_SIGMOID = 1, EY_ACT_TANH = 2, EY_ACT_RELU = 3 };

/* likelihood codes: eeyore/constants/constants.py:15-18 */
enum ey_lik {
  EY_LIK_BCE_SUM = 0, /* 'binary_classification': naive BCE(sum) on probabilities, eeyore/stats/loss.py:1-11 */
  EY_LIK_CE_SUM = 1,  /* 'multiclass_classification': CrossEntropyLoss(sum)(logits, argmax(y,1)) */
  /* Regression on a continuous or count response: BayesianModel takes any callable as loss, log_lik = -loss(forward(x), y)
   * (eeyore/models/bayesian_model.py:30-35).  out = the network output after the last layer's activation (any supported
   * activation), r = out - y, s = the plan's likelihood scale (ey_plan_set_lik_scale); the row term is summed over the
   * d_K outputs:
   *   EY_LIK_GAUSS_SUM    -log(s sqrt(2 pi)) - r^2 / (2 s^2)    = Normal(out, s).log_prob(y).sum()
   *   EY_LIK_LAPLACE_SUM  -log(2 s) - |r| / s                   = Laplace(out, s).log_prob(y).sum(); the gradient takes
   *                                                               sign(0) = 0, what autograd gives at the kink
   *   EY_LIK_POISSON_SUM  y out - exp(out)                      = -PoissonNLLLoss(log_input=True, full=False,
   *                                                               reduction='sum')(out, y): out is the log-rate and the
   *                                                               y! term is left out, so this is the log-density of y up
   *                                                               to a constant in y (no constant in theta is missing)
   * Nothing is clamped: an exp that overflows gives a -inf or NaN target, which every accept step rejects, as the naive
   * logs of the classification losses do.  A plan of these codes is served by the "generic" kernels or by "bgemm" (the
   * separate layerwise launches); the fused families carry the classification losses only. */
  EY_LIK_GAUSS_SUM = 2,
  EY_LIK_LAPLACE_SUM = 3,
  EY_LIK_POISSON_SUM = 4
};

enum ey_dtype { EY_F32 = 0, EY_F64 = 1 }; /* model.dtype, eeyore/models/model.py:7-10 */

/* Plan options (ey_plan_set_option).
 * EY_OPT_F32_PRODUCTS: how the fused f32 trajectory kernel ("mfma32": MLP(4-32-32-3), BASELINE configs 3/4) forms its three
 * 32x32x32 products per row tile, and the layerwise path ("bgemm") its 128-wide batched products.  The reference computes them with torch's f32 matmul (eeyore/models/mlp.py:45-50 ->
 * nn.Linear); both forms below are f32 in, f32 out, f32 accumulate, and both pass every f32 parity test at the same
 * tolerances:
 *   EY_PRODUCTS_BF16X3 (default): each f32 operand is split EXACTLY into three bf16 pieces (hi + mid + lo = x) and the
 *     product is summed from the six piece products of relative size >= 2^-18 on v_mfma_f32_32x32x16_bf16 (bf16 x bf16 is
 *     exact in f32, accumulation in f32, smallest terms first); measured error against f64 (profiles/r03_bf3_error_probe.txt,
 *     tests/test_bf16x3.py): rms within 0.85 .. 1.06 x the exact form's, maximum within 0.74 .. 1.48 x (1.30 x on the
 *     golden fixtures; the bar the tests hold it to is 1.5 x); the fused kernel takes it for batches of up to 512
 *     rows, and in this form it also serves the other MLP(4-32-32-dK) models with one hidden activation (sigmoid / tanh /
 *     relu; CE-sum on 3 logits or BCE-sum on one sigmoid output), which otherwise run on "fused16";
 *   EY_PRODUCTS_EXACT: v_mfma_f32_32x32x2_f32 (16x16x4 on "fused16"), bit for bit a k-ordered f32 fma chain.
 * The environment variable EY_F32_PRODUCTS=exact|bf16x3 sets what new plans start with. */
enum ey_option { EY_OPT_F32_PRODUCTS = 1, EY_OPT_ROW_WAVES = 2, EY_OPT_MAX_CHUNK_CHAINS = 3 };
enum ey_products { EY_PRODUCTS_BF16X3 = 0, EY_PRODUCTS_EXACT = 1 };
/* EY_OPT_ROW_WAVES: tiny models (at most three layers, eight inputs, other widths <= 4: the reference's own test and example
 * models) on batches of 128 rows or more may give a chain up to four waves, each taking every fourth 64-row tile of an
 * evaluation; the waves' partial gradients are added in a fixed order, which is not the order one wave adds them in, so the
 * two differ in the last bits.  EY_ROW_WAVES_OFF is the default (environment EY_ROW_WAVES=0|1|2 sets what new plans start
 * with): a chain's bits then depend on (seed, chain_offset + chain, iteration) alone -- not on how many chains share the
 * launch, how they are sharded over ranks, or the device's CU count.  _ON pins the waves (same guarantee, the other
 * summation order).  EY_ROW_WAVES_AUTO is the opt-in latency setting: the waves while one wave per chain would leave the
 * chip idle (chains <= 4 x CUs), so a chain's last bits follow the launch's chain count: BASELINE config 2 (MALA, 256
 * chains, N = 256) 7.7 -> 5.4 us per draw (tools/bench_configs.py opts in). */
enum ey_row_waves { EY_ROW_WAVES_OFF = 0, EY_ROW_WAVES_ON = 1, EY_ROW_WAVES_AUTO = 2 };
/* EY_OPT_MAX_CHUNK_CHAINS: the layerwise path ("bgemm") runs a call's chains in chunks, one set of launches per chunk, so
 * that the activations of a chunk fit a scratch budget: min(16 GiB / activation bytes per chain, 32768) chains.  Value 0
 * (default) is that rule; k > 0 bounds a chunk by k chains as well, which bounds the scratch by k chains' activations;
 * negative values are refused.  A workgroup of this path sees one chain, so a chain's bits do not depend on the value. */

enum ey_flags {
  EY_RECOMPUTE_INITIAL_GRAD = 1, /* HMC: re-evaluate the gradient at the start of the trajectory exactly as
                                    hmc.py:104 does (L+1 evaluations) instead of using the cached `grad` (L) */
  EY_FORCE_GENERIC = 2,          /* route to the generic VALU kernels even when an MFMA kernel covers the plan */
  EY_GIBBS_CARRY = 4             /* ey_gibbs_*: a rejected sub-step's proposal stays in the proposal vector for the rest
                                    of the draw, as eeyore/samplers/gibbs.py:67-102 leaves it (mode 'reference') */
};

int ey_version(void);
const char* ey_last_error(void);

/* Replaces mlp.Hyperparameters + MLP.__init__/set_fc_layers (eeyore/models/mlp.py:9-43) and the choice of
 * loss_functions[...] (eeyore/constants/constants.py:15-18).  dims has n_layers+1 entries; bias/act n_layers. */
int ey_plan_create(ey_plan** out, int n_layers, const int* dims, const int* bias, const int* act, int likelihood,
                   int dtype, int device_id);
/* Replaces DistributionModel.__init__ + log_target (eeyore/models/distribution_model.py:6-28) for the closures the
 * reference's own examples use: a multivariate normal or a mixture of M of them on theta in R^P,
 *   log p(theta) = log sum_k exp(c[k] - (theta - mean[k])^T prec[k] (theta - mean[k]) / 2)
 * (c[k] = log w_k - log det(2 pi Sigma_k) / 2 for the normalised density, log w_k for the kernel alone).  c [M],
 * mean [M, P], prec [M, P, P] row-major are HOST arrays of doubles, read during the call only and rounded once to the plan's
 * dtype.  Validated before anything touches the device -- EY_ERR_INVALID: P < 1, M < 1, a non-finite entry, a prec[k] that
 * is not exactly symmetric or has a diagonal entry that is not > 0; EY_ERR_UNSUPPORTED: P > 128, M > 16.
 * The plan is born with data and prior "set", ey_plan_kernel says "dist" and ey_plan_num_params P.  It serves
 * ey_log_target (log_lik = the tempered log-density, log_prior = 0), ey_log_target_grad, ey_hmc_*, ey_mala_*, ey_mh_*,
 * ey_mh_tril_*, ey_mala_tril_*, ey_ram_*, ey_am_* and ey_plan_attach_moments with their usual array semantics; ey_plan_set_data / _set_prior return
 * EY_ERR_INVALID, ey_log_lik_rows, ey_gibbs_* and ey_plan_attach_da EY_ERR_UNSUPPORTED; EY_FORCE_GENERIC, the options and
 * the variant switches are accepted and change nothing. */
int ey_plan_create_mixture(ey_plan** out, int64_t P, int M, const double* c, const double* mean, const double* prec,
                           int dtype, int device_id);
/* The same for the closures of the reference's Gamma examples and their relatives: theta = log x with the Jacobian in the
 * closure (Gamma, inverse Gamma, Weibull) or a Gumbel density on theta itself -- one separable family on theta in R^P,
 *   log p(theta) = sum_i [ c[i] + a[i] theta_i - b[i] exp(s[i] theta_i) ],   d/dtheta_i = a[i] - b[i] s[i] exp(s[i] theta_i)
 * (Gamma(shape k, scale t): a = k, b = 1/t, s = 1, c = -lgamma(k) - k log t, or 0 for the unnormalised density).  c, a, b, s
 * [P] are HOST arrays of doubles, read during the call only and rounded once to the plan's dtype.  Validated before anything
 * touches the device, *out null on failure -- EY_ERR_INVALID: a null argument, P < 1, a non-finite entry, b[i] <= 0,
 * s[i] == 0 or a[i] / s[i] <= 0 (the density would not be proper; the message names i); EY_ERR_UNSUPPORTED: P > 128.
 * Nothing is clamped: where exp(s[i] theta_i) overflows the value is -inf and the gradient component -sign(s[i]) inf (a
 * sampler rejects such a proposal), where it underflows the component is a[i] exactly, a NaN coordinate gives a NaN value.
 * The plan serves and refuses the calls a plan of ey_plan_create_mixture does (its messages say "a distribution plan") and
 * ey_plan_kernel says "dist". */
int ey_plan_create_exptilt(ey_plan** out, int64_t P, const double* c, const double* a, const double* b, const double* s,
                           int dtype, int device_id);
int ey_plan_destroy(ey_plan* plan);
/* Model.num_params (eeyore/models/model.py:34-36) */
int ey_plan_num_params(const ey_plan* plan, int64_t* P);
/* name of the kernel family that serves ey_hmc_step for this plan: "mfma32" (fused f32 trajectory, 4-32-32-dK), "fused16"
 * (fused 16x16x4 trajectory, f32 and f64: one or two hidden layers of at most 64 units (32 in f64), at most 16 inputs,
 * CE-sum on at most 16 logits or BCE-sum on at most 4 sigmoid outputs, every layer with or without a bias), "bgemm"
 * (layerwise batched GEMMs for models beyond LDS and for wide ones that fit, f32 and f64) or "generic" (anything mlp.py
 * builds); "dist" for a plan of ey_plan_create_mixture */
const char* ey_plan_kernel(const ey_plan* plan);
int ey_plan_set_option(ey_plan* plan, int option, int value);
int ey_plan_get_option(const ey_plan* plan, int option, int* value);

/* The (x, y) full batch the samplers receive from their DataLoader (eeyore/samplers/serial_sampler.py:41-46).
 * x [N, d_0]; y [N, d_K] (one-hot for CE as XYDataset(yonehot=True) yields, {0,1} for BCE, the responses for the
 * regression codes: counts for EY_LIK_POISSON_SUM).  Copied into the plan. */
int ey_plan_set_data(ey_plan* plan, const void* x, const void* y, int64_t N, void* stream);
/* model.prior = Normal(mu, sigma) elementwise (eeyore/models/mlp.py:31-35).  mu, sigma [P].  Copied. */
int ey_plan_set_prior(ey_plan* plan, const void* mu, const void* sigma, void* stream);
/* model.prior = Laplace(loc, scale) / StudentT(df, loc, scale) / Cauchy(loc, scale) elementwise: any prior the reference
 * sums as prior.log_prob(theta) parameter by parameter (eeyore/models/bayesian_model.py:46-50).
 *   EY_PRIOR_LAPLACE    log p = sum_i -log(2 b_i) - |theta_i - loc_i| / b_i; the gradient takes sign(0) = 0
 *   EY_PRIOR_STUDENT_T  log p = sum_i lgamma((nu_i+1)/2) - lgamma(nu_i/2) - log(nu_i pi)/2 - log s_i
 *                                     - (nu_i+1)/2 log1p((theta_i - loc_i)^2 / (nu_i s_i^2));  Cauchy is nu = 1
 * loc, scale, df: [P] device arrays of the plan's dtype, copied; df is read for EY_PRIOR_STUDENT_T only and may be NULL
 * otherwise.  EY_PRIOR_NORMAL here is exactly ey_plan_set_prior(plan, loc, scale, stream), and ey_plan_set_prior sets the
 * family back to Normal.  Validated on the host before anything is stored -- EY_ERR_INVALID: an unknown family, a loc that is
 * not finite, a scale or df that is not finite and > 0, a mixture plan.  The tables are built in double and rounded once
 * to the plan's dtype.
 * A plan whose family is not Normal is served by the "generic" kernels only, whatever the model (ey_plan_kernel says so):
 * every operation of a model whose generic LDS image does not fit a CU returns EY_ERR_UNSUPPORTED, and in-kernel dual
 * averaging (ey_plan_attach_da) is refused as for every generic plan.  Setting a Normal prior again restores the plan's
 * routing and its results bit for bit. */
enum ey_prior_family { EY_PRIOR_NORMAL = 0, EY_PRIOR_LAPLACE = 1, EY_PRIOR_STUDENT_T = 2 };
int ey_plan_set_prior_family(ey_plan* plan, int family, const void* loc, const void* scale, const void* df, void* stream);
int ey_plan_prior_family(const ey_plan* plan);
/* The scale s of EY_LIK_GAUSS_SUM / EY_LIK_LAPLACE_SUM: one positive number per plan (default 1), shared by the d_K outputs.
 * The constants the kernels use (1/s^2 or 1/s, and the per-element log-normaliser) are worked out here in double and rounded
 * once to the plan's dtype.  EY_ERR_INVALID: s not finite or not > 0, or a plan of a classification or Poisson code (which
 * have no scale).  ey_plan_lik_scale returns s (1 for the codes without one). */
int ey_plan_set_lik_scale(ey_plan* plan, double s);
double ey_plan_lik_scale(const ey_plan* plan);

/* BayesianModel.log_lik / log_prior / log_target (eeyore/models/bayesian_model.py:30-56) for C chains.
 * temp: per-chain temperature [C] or NULL (model.temperature = None); multiplies BOTH outputs (:33-34,48-49).
 * log_lik, log_prior: [C] outputs (either may be NULL). */
int ey_log_target(ey_plan* plan, const void* theta, const void* temp, int64_t C, void* log_lik, void* log_prior,
                  void* stream);
/* The N terms of BayesianModel.log_lik's sum, one per data row (the loss of eeyore/constants/constants.py:15-18 is a
 * sum over rows): rows [C, N], rows[c, n] = log-likelihood of row n under theta[c] (times temp[c] if given).  This is
 * the integrand of BayesianModel.predictive_posterior for N points and C posterior samples at once
 * (eeyore/models/bayesian_model.py:58-67: exp of the log-likelihood of ONE point, averaged over samples by MCIntegrator,
 * eeyore/integrators/mcintegrator.py:16-36). */
int ey_log_lik_rows(ey_plan* plan, const void* theta, const void* temp, int64_t C, void* rows, void* stream);
/* MLP.forward (eeyore/models/mlp.py:45-50) of C parameter vectors on the attached batch: out [C, N, d_K] of the plan's
 * dtype, out[c, n, :] = the network output of row n under theta[c] after the last layer's activation (logits under CE-sum,
 * probabilities under BCE-sum, the mean / location / log-rate under the regression codes).  Any likelihood code, any prior
 * family; data and prior must be attached (the y of the batch is not read into the result).  One launch of the generic
 * kernels when the model fits their LDS image, the layerwise forward products otherwise -- also for a model that "mfma32"
 * or "fused16" serves: the fused families have no such output, and ey_plan_kernel is unchanged by the call.
 * EY_ERR_INVALID on a mixture plan (it has no network). */
int ey_forward(ey_plan* plan, const void* theta, int64_t C, void* out, void* stream);
/* LogTargetModel.upto_grad_log_target (eeyore/models/log_target_model.py:15-23): target [C], grad [C,P]. */
int ey_log_target_grad(ey_plan* plan, const void* theta, const void* temp, int64_t C, void* target, void* grad,
                       void* stream);

/* One HMC.draw (eeyore/samplers/hmc.py:126-156, full-batch path) for C chains: momentum draw, HMC.leapfrog
 * (:100-124), Hamiltonians (:91-98), accept `u < min(exp(H_cur-H_prop),1)` (:143-148), state update.
 *  theta [C,P], target [C], grad [C,P]: current state, updated in place for accepted chains;
 *  p0 [C,P] replaces torch.randn (:134) and u [C] replaces torch.rand(1) (:148); NULL => the in-kernel
 *    Philox4x32-10 stream keyed by (seed, chain_offset + chain, iter) -- see ey_philox_normal/uniform;
 *  step: scalar step size; step_vec [C] overrides it per chain when not NULL; L = num_steps;
 *  accepted [C] uint8, accept_rate [C], H_cur [C], H_prop [C]: outputs (the last three may be NULL). */
int ey_hmc_step(ey_plan* plan, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                const void* step_vec, int L, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                uint64_t chain_offset, uint32_t flags, void* accepted, void* accept_rate, void* H_cur, void* H_prop,
                void* stream);

/* n_iters consecutive iterations (iter, iter + 1, ...) of HMC.draw for every chain inside ONE launch: exactly what
 * n_iters calls of ey_hmc_step with p0 = u = NULL do (same Philox streams, bit-identical states), without the launches
 * in between and with every chain looping on its own.  This is SerialSampler.run's inner loop
 * (eeyore/samplers/serial_sampler.py:41-52) for the iterations in which nothing on the host looks at the state
 * (no tuner step, no minibatch change).  Records, each nullable: samples [n_iters, C, P], targets [n_iters, C] and
 * accepted_rec [n_iters, C] uint8 = the state of every chain after each iteration, i.e. what ChainList.update stores
 * (eeyore/chains/chain_list.py:64-67); accept_count [C] int32 is incremented per accepted iteration.
 * accepted [C] uint8 receives the last iteration's flags.  Attached moments are accumulated every iteration. */
int ey_hmc_run(ey_plan* plan, void* theta, void* target, void* grad, double step, const void* step_vec, int L,
               const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
               int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted,
               void* stream);

/* HMC.leapfrog(position0, momentum0, x, y) (eeyore/samplers/hmc.py:100-124) for C chains, exactly as the
 * reference runs it: L steps, L+1 gradient evaluations, final momentum negated.  theta [C,P] and p [C,P] are
 * in/out (position_L, momentum_L); target [C] and grad [C,P] receive the log-target and its gradient at
 * position_L.  Used by HMC.init_step (:38-77) and by callers of the public leapfrog method. */
int ey_hmc_leapfrog(ey_plan* plan, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                    int64_t C, void* target, void* grad, void* stream);

/* One MALA.draw (eeyore/samplers/mala.py:46-82) with the default NormalKernel(theta + step/2 grad, sqrt(step))
 * (:35-41; eeyore/kernels/normal_kernel.py:5-23): z [C,P] standard normals (NULL => Philox), u [C].
 * Accept iff log(u) < log_rate (:66).  log_rate [C] output may be NULL. */
int ey_mala_step(ey_plan* plan, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                 const void* step_vec, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                 uint64_t chain_offset, uint32_t flags, void* accepted, void* log_rate, void* stream);

/* One MetropolisHastings.draw (eeyore/samplers/metropolis_hastings.py:41-73), symmetric NormalKernel(theta,
 * scale): prop = theta + scale * z; scale [P] device array.  log_rate = target(prop) - target(theta) (:50). */
int ey_mh_step(ey_plan* plan, void* theta, void* target, const void* z, const void* u, const void* scale,
               const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
               void* accepted, void* log_rate, void* stream);

/* n_iters consecutive MALA.draw / MetropolisHastings.draw iterations inside one launch, with the same records as
 * ey_hmc_run: exactly what n_iters calls of ey_mala_step / ey_mh_step with z = u = NULL do. */
int ey_mala_run(ey_plan* plan, void* theta, void* target, void* grad, double step, const void* step_vec,
                const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted,
                void* stream);
int ey_mh_run(ey_plan* plan, void* theta, void* target, const void* scale, const void* temp, int64_t C, uint64_t seed,
              uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples, void* targets,
              void* accepted_rec, void* accept_count, void* accepted, void* stream);

/* One RAM.draw (eeyore/samplers/ram.py:38-70) for C chains. chol [C,P,P] lower-triangular, in/out; z [C,P], u [C]
 * replace the random draws (NULL => Philox, as ey_mh_step); n = counter.idx + 1 - offset (>= 1); 0 < a < 1.
 * Robust adaptive Metropolis (Vihola 2012): propose theta + chol z, accept iff log(u) < log_rate, then always adapt
 * chol <- chol(chol (I + h (alpha - a) z z^T / |z|^2) chol^T), h = min(1, P n^-g), alpha = min(1, exp(log_rate)) with a
 * NaN log_rate counting as 1.  Only the lower triangle of chol is read or written.  Served by one kernel for every model
 * (whatever ey_plan_kernel reports) with P <= 128 whose factor fits beside its evaluation image in LDS;
 * EY_ERR_UNSUPPORTED otherwise, before any launch.  log_rate [C] output may be NULL. */
int ey_ram_step(ey_plan* plan, void* theta, void* target, void* chol, const void* z, const void* u, double a, double g,
                uint64_t n, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                uint32_t flags, void* accepted, void* log_rate, void* stream);
/* n_iters iterations in one launch (adaptation index n, n+1, ...), records as ey_mh_run; bit-identical to n_iters
 * calls of ey_ram_step with z = u = NULL. */
int ey_ram_run(ey_plan* plan, void* theta, void* target, void* chol, double a, double g, uint64_t n, const void* temp,
               int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters,
               void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream);

/* One MetropolisHastings.draw (eeyore/samplers/metropolis_hastings.py:41-73) whose kernel is a
 * MultivariateNormalKernel(theta, scale_tril): prop = theta + L z with a FIXED lower-triangular factor L, accept iff
 * log(u) < log_rate = target(prop) - target(theta).  z [C,P], u [C] replace the random draws (NULL => Philox, the streams
 * of ey_mh_step: with L = I the proposal is ey_mh_step's with scale = 1).  tril [G,P,P] row-major device array of the
 * plan's dtype, read only; only the lower triangle (j <= i) of a factor is read, the strict upper triangle may hold
 * anything.  Which factor a chain uses: G == 1, the one factor; tril_index == NULL, chain c uses factor c (G == C);
 * otherwise factor tril_index[c] (device int32 [C]), clamped into [0, G) -- checking its range is the caller's business.
 * EY_ERR_INVALID: a null theta / target / tril / accepted, n_iters < 1, G < 1, tril_index == NULL with G neither 1 nor C.
 * Served by one kernel for every model (whatever ey_plan_kernel reports), mixture plans included, with P <= 128 whose
 * factor fits beside its evaluation image in LDS; EY_ERR_UNSUPPORTED otherwise, before any launch and with nothing
 * written.  flags is accepted and ignored.  log_rate [C] output may be NULL. */
int ey_mh_tril_step(ey_plan* plan, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                    const void* z, const void* u, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                    uint64_t chain_offset, uint32_t flags, void* accepted, void* log_rate, void* stream);
/* n_iters iterations in one launch (the factor is staged once), records as ey_mh_run; ey_mh_tril_run is bit-identical to
 * n_iters calls of ey_mh_tril_step with z = u = NULL. */
int ey_mh_tril_run(ey_plan* plan, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                   const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                   int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted,
                   void* stream);

/* One MALA.draw (eeyore/samplers/mala.py:46-82) whose kernel is a MultivariateNormalKernel(loc, scale_tril): with
 * loc = theta + step/2 grad (:35-36) and a FIXED lower-triangular factor L, prop = loc + L z, loc' = prop + step/2 grad(prop),
 * log_rate = target(prop) - target(theta) + |L^-1 (prop - loc)|^2 / 2 - |L^-1 (theta - loc')|^2 / 2 (the proposal is not
 * symmetric; each term one forward substitution), accept iff log(u) < log_rate.  step enters the mean only: the proposal
 * covariance is L L^T as given.  theta, target, grad, z, u, step, step_vec and temp are ey_mala_step's (z = NULL => Philox,
 * its streams); tril, G and tril_index are ey_mh_tril_step's: tril [G,P,P] row-major device array of the plan's dtype, read
 * only; only the lower triangle (j <= i) of a factor is read, the strict upper triangle may hold anything; G == 1 one factor,
 * tril_index == NULL chain c's own (G == C), otherwise factor tril_index[c] (device int32 [C]) clamped into [0, G).
 * EY_ERR_INVALID: a null theta / target / grad / tril / accepted, step <= 0 without step_vec, n_iters < 1, G < 1,
 * tril_index == NULL with G neither 1 nor C.  Served by one kernel for every model (whatever ey_plan_kernel reports),
 * mixture plans included, with P <= 128 whose factor fits beside its evaluation image in LDS; EY_ERR_UNSUPPORTED otherwise,
 * before any launch and with nothing written.  flags is accepted and ignored.  log_rate [C] output may be NULL. */
int ey_mala_tril_step(ey_plan* plan, void* theta, void* target, void* grad, const void* tril, int64_t G,
                      const void* tril_index, const void* z, const void* u, double step, const void* step_vec,
                      const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                      void* accepted, void* log_rate, void* stream);
/* n_iters iterations in one launch (the factor is staged once), records as ey_mala_run; ey_mala_tril_run is bit-identical
 * to n_iters calls of ey_mala_tril_step with z = u = NULL. */
int ey_mala_tril_run(ey_plan* plan, void* theta, void* target, void* grad, const void* tril, int64_t G,
                     const void* tril_index, double step, const void* step_vec, const void* temp, int64_t C, uint64_t seed,
                     uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples, void* targets,
                     void* accepted_rec, void* accept_count, void* accepted, void* stream);

/* The block table of a Gibbs sampler: S sub-steps in visiting order, sub-step s proposing for the parameters
 * blk_idx[blk_off[s] .. blk_off[s+1]) with the Normal scale blk_scale[s].  The table is model-agnostic (blockwise
 * random-walk Metropolis over any list of DISJOINT index sets of [0, P)); the node numbering of an MLP lives with the
 * caller.  blk_off [S+1] and blk_idx [blk_off[S]] int32, blk_scale [S] double: HOST arrays owned by the caller, read
 * during this call only.  The call validates them (EY_ERR_INVALID: S < 1, blk_off[0] != 0, an empty block, an index out of
 * [0, P), an index in two blocks, a scale that is not a positive finite number) and uploads a device copy, converted to
 * `dtype`, which the table object owns until ey_gibbs_table_destroy (call it once no launch that uses it is in flight). */
int ey_gibbs_table_create(ey_gibbs_table** out, int64_t P, int S, const int32_t* blk_off, const int32_t* blk_idx,
                          const double* blk_scale, int dtype, int device_id);
int ey_gibbs_table_destroy(ey_gibbs_table* table);

/* One Gibbs.draw (eeyore/samplers/gibbs.py:67-102) for C chains: S Metropolis sub-steps in the table's order.  Sub-step s
 * adds blk_scale[s] * z[c, i] to the proposal vector for the i of its block, evaluates the log-target of the whole
 * proposal vector, and accepts iff log(u[c, s]) < log_target - target[c] (a NaN rejects).  On accept the block enters the
 * state and target[c] takes the value; on reject the block of the proposal vector is restored from the state, or, with
 * EY_GIBBS_CARRY in flags, left as proposed for the rest of the draw as the reference leaves it.  z [C,P], u [C,S] replace
 * the random draws; NULL => Philox: parameter i uses normal i of the iteration (ey_philox_normal), sub-step s the accept
 * stream at block word s (ey_philox_uniform_blocks; sub-step 0 draws ey_philox_uniform's variate).  accepted [C,S] uint8;
 * log_rate [C,S] may be NULL.  Attached moments: s1, s2 take the state after the draw, acc the accepted fraction of its S
 * sub-steps.  Served by one kernel for every model that fits in LDS with the table beside it (whatever ey_plan_kernel
 * reports), EY_ERR_UNSUPPORTED otherwise; a table built for another P, dtype or device is EY_ERR_INVALID; both before
 * any launch. */
int ey_gibbs_step(ey_plan* plan, const ey_gibbs_table* table, void* theta, void* target, const void* z, const void* u,
                  const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                  void* accepted, void* log_rate, void* stream);
/* n_iters draws in one launch; records samples [n,C,P], targets [n,C], accepted_rec [n,C,S] uint8, accept_count [C,S]
 * int32 (+=), each may be NULL; bit-identical to n_iters calls of ey_gibbs_step with z = u = NULL. */
int ey_gibbs_run(ey_plan* plan, const ey_gibbs_table* table, void* theta, void* target, const void* temp, int64_t C,
                 uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                 void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream);

/* One AM.draw (eeyore/samplers/am.py:61-107, Haario et al.'s adaptive Metropolis) for C chains, with the transform
 * cov -> cov + eps I fused.  State, all in/out: running_mean [C,P], cov_sum [C,P,P], cov [C,P,P] (only j <= i of the two
 * matrices is read or written), num_accepted [C] int32.  cov0 is the TRANSFORMED initial covariance, [P,P] or, with
 * cov0_per_chain != 0, [C,P,P].  With n = idx + 1 - offset (>= 1, idx >= 0): the proposal is theta + c z while n <= t0;
 * afterwards u_mix < l proposes theta + c z and anything else theta + (b chol(cov)) z.  Accept iff log(u) < log_rate;
 * num_accepted counts accepts of idx > 0.  Then running_mean <- ((n-1) running_mean + theta) / n, cov_sum += theta theta^T
 * and, from n >= t0 on, cov <- cov0 while num_accepted == 0, else (cov_sum - n mean mean^T) / (n-1) + eps I.
 * A pivot of the factorisation that is not > 0 (NaN included) makes the draw propose theta + c z and adds one to
 * breakdowns [C] int32.  z [C,P], u_mix [C], u [C] replace the random draws (NULL => Philox: u_mix is word block 1 of
 * the accept stream).  Outputs: accepted [C] uint8; log_rate [C] and branch [C] uint8 (0 isotropic, 1 factor,
 * 2 breakdown) may be NULL.  t0 >= 2, 0 <= l <= 1, b and c finite, eps finite and >= 0: EY_ERR_INVALID otherwise.
 * Served by one kernel for every model (whatever ey_plan_kernel reports) with P <= 128 whose two covariance triangles fit
 * beside its evaluation image in LDS; EY_ERR_UNSUPPORTED otherwise, before any launch. */
int ey_am_step(ey_plan* plan, void* theta, void* target, void* running_mean, void* cov_sum, void* cov, void* num_accepted,
               const void* cov0, int cov0_per_chain, double l, double b, double c, double eps, int64_t t0, int64_t idx,
               int64_t offset, const void* z, const void* u_mix, const void* u, const void* temp, int64_t C,
               uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, void* accepted, void* log_rate,
               void* branch, void* breakdowns, void* stream);
/* n_iters iterations in one launch (idx, idx+1, ...), records as ey_mh_run; bit-identical to n_iters calls of
 * ey_am_step with z = u_mix = u = NULL. */
int ey_am_run(ey_plan* plan, void* theta, void* target, void* running_mean, void* cov_sum, void* cov, void* num_accepted,
              const void* cov0, int cov0_per_chain, double l, double b, double c, double eps, int64_t t0, int64_t idx,
              int64_t offset, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
              uint32_t flags, int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count,
              void* accepted, void* breakdowns, void* stream);

/* ey_am_step / ey_am_run with the transform softabs(cov, a) (below) in place of the ridge, as the reference's AM examples
 * use it: from n >= t0 on, with something accepted, cov <- softabs((cov_sum - n mean mean^T) / (n-1), a), computed inside
 * the kernel by the chain's wave in f64 for both dtypes and rounded once.  cov0 is the TRANSFORMED initial covariance, as
 * there.  A raw covariance with an entry that is not finite stays untransformed; the factorisation of the next draw that
 * needs it reports the breakdown.  a must be finite and > 0 (EY_ERR_INVALID).  The f64 work matrix of softabs follows the
 * two triangles in LDS: ey_am_softabs_fits says whether a plan's model leaves room for it (1) or not (0, and the two
 * calls return EY_ERR_UNSUPPORTED before any launch).  Everything else as ey_am_step / ey_am_run. */
int ey_am_softabs_step(ey_plan* plan, void* theta, void* target, void* running_mean, void* cov_sum, void* cov,
                       void* num_accepted, const void* cov0, int cov0_per_chain, double l, double b, double c, double a,
                       int64_t t0, int64_t idx, int64_t offset, const void* z, const void* u_mix, const void* u,
                       const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                       void* accepted, void* log_rate, void* branch, void* breakdowns, void* stream);
int ey_am_softabs_run(ey_plan* plan, void* theta, void* target, void* running_mean, void* cov_sum, void* cov,
                      void* num_accepted, const void* cov0, int cov0_per_chain, double l, double b, double c, double a,
                      int64_t t0, int64_t idx, int64_t offset, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                      uint64_t chain_offset, uint32_t flags, int n_iters, void* samples, void* targets, void* accepted_rec,
                      void* accept_count, void* accepted, void* breakdowns, void* stream);
int ey_am_softabs_fits(const ey_plan* plan);

/* softabs(A, a) = Q diag(f(lambda)) Q^T with f(x) = x / tanh(a x) and f(0) = 1 / a (eeyore/stats/metrics.py:3-5, which
 * yields NaN at an eigenvalue that is exactly zero) of B dense symmetric [P,P] matrices of `dtype`, one wave each, by
 * one-sided Jacobi in f64; the result is rounded once to `dtype`.  Only the lower triangle of A is read; out [B,P,P]
 * receives the whole symmetric matrix and may be A.  A matrix with an entry that is not finite comes back as it was.
 * sweeps [B] int32 (may be NULL): the Jacobi sweeps taken (0 for P = 1, -1 for a matrix left as it was).  The same device
 * function in the same order as in ey_am_softabs_*: the same bits.  Needs no plan; runs on the current device.
 * a finite and > 0, P >= 1 (EY_ERR_INVALID); P <= 128 (EY_ERR_UNSUPPORTED). */
int ey_softabs(const void* A, int64_t B, int64_t P, int dtype, double a, void* out, void* sweeps, void* stream);

/* PowerPosteriorSampler.between_chain_move (eeyore/samplers/power_posterior_sampler.py:135-163) decision for C
 * chain pairs: log_rate = dlogq + (t_i - t_j) * (ell_j - ell_i) with ell the UNTEMPERED log-target; swap iff
 * log(u) < log_rate (:160).  All arrays [C] of `dtype`; dlogq may be NULL (symmetric partner choice). */
int ey_pt_swap_decide(const void* ell_i, const void* ell_j, const void* t_i, const void* t_j, const void* dlogq,
                      const void* u, int64_t C, int dtype, void* swap /* uint8 [C] */, void* log_rate, void* stream);

/* The ladder of a power-posterior sampler for ey_pt_between: K temperatures t [K] and the partner weights q [K,K], row i
 * the weights with which chain i proposes its partner (diagonal ignored; a row need not be normalised).  HOST arrays owned
 * by the caller, read during this call only and validated before anything touches the device (EY_ERR_INVALID: K < 2, a
 * temperature that is not a positive finite number, a negative or NaN off-diagonal weight, a row whose sum is not positive
 * and finite; EY_ERR_UNSUPPORTED: K > 1024, the kernel's limit).  The object owns a device copy on the CURRENT device: t and
 * log(q[i,j] / row sum) rounded to `dtype`, and per row the running sums of q[i,j] / row sum in index order as doubles (the
 * diagonal adds nothing).  Destroy it once no launch that uses it is in flight. */
int ey_pt_ladder_create(const double* t, const double* q, int K, int dtype, ey_pt_ladder** out);
int ey_pt_ladder_destroy(ey_pt_ladder* ladder);

/* PowerPosteriorSampler.between_chain_moves (eeyore/samplers/power_posterior_sampler.py:128-172) for R replicas of the
 * ladder in one launch.  State row k * R + r is temperature k of replica r: theta [K*R,P], target [K*R] (the TEMPERED
 * log-targets) and grad [K*R,P] (may be NULL) of the ladder's dtype, updated in place.  For i = 0 .. K-1 in order, step i
 * sees the exchanges of the steps before it: partner j, ell_i = target_i / t_i, ell_j = target_j / t_j,
 * log_rate = (log_q[j,i] - log_q[i,j]) + (t_i - t_j) * (ell_j - ell_i) as ey_pt_swap_decide forms it, and iff
 * log(u) < log_rate the theta rows of i and j trade places, target_i <- target_j * (t_i / t_j),
 * target_j <- target_i * (t_j / t_i), and the grad rows trade places with the same two factors.
 * partners [K,R] int32 and u [K,R] of dtype are both given or both NULL (anything else: EY_ERR_INVALID).  A given partner
 * outside [0, K) or equal to its own i is checked in the kernel and faults nothing: that step exchanges nothing and
 * reports swap_out = 0 and a NaN log_rate_out.  NULL => Philox keyed (seed, replica_offset + r, iter, stream 2): block
 * word i gives step i its variates, words 0, 1 a 53-bit double v for the partner (the first index whose running sum
 * exceeds v; the last index other than i when none does), words 2, 3 the accept variate u as ey_philox_uniform_blocks
 * converts words 0, 1 -- a replica's bits depend on (seed, replica_offset + r, iter) alone.
 * rec_theta [K*R,P], rec_target [K*R] (each may be NULL): the record of the draw the move belongs to, which holds the
 * state from before the move; exchanged rows are written there too and rec_target takes every target.
 * partners_out [K,R] int32, u_out [K,R], swap_out [K,R] uint8, log_rate_out [K,R]: each may be NULL. */
int ey_pt_between(const ey_pt_ladder* ladder, void* theta, void* target, void* grad, int64_t R, int64_t P,
                  const int32_t* partners, const void* u, uint64_t seed, uint64_t iter, uint64_t replica_offset,
                  void* rec_theta, void* rec_target, int32_t* partners_out, void* u_out, void* swap_out,
                  void* log_rate_out, void* stream);

/* The in-kernel random streams, exposed so a caller (or a test) can reproduce them:
 *  normal  out[c, i] = N(0,1) for parameter i of chain chain_offset + c at iteration iter (what p0/z = NULL uses)
 *  uniform out[c]    = U[0,1) accept variate of that chain and iteration (what u = NULL uses). */
int ey_philox_normal(void* out, int64_t C, int64_t P, uint64_t seed, uint64_t iter, uint64_t chain_offset, int dtype,
                     void* stream);
int ey_philox_uniform(void* out, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, int dtype,
                      void* stream);
/* out[c, s] = U[0,1) accept variate of sub-step s of that chain and iteration (what ey_gibbs_step's u = NULL uses): the
 * accept stream with Philox block word s, so out[:, 0] is ey_philox_uniform's variate. */
int ey_philox_uniform_blocks(void* out, int64_t C, int64_t S, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                             int dtype, void* stream);
/* One Philox4x32-10 block on the HOST (no device needed): out[4] = philox(counter[4], key[2]), the function the device
 * streams above are built on (Salmon et al. 2011; checked against Random123's known-answer vectors in the tests).
 * counter = (block, chain_lo, iter_lo, iter_hi << 8 | stream | chain_hi << 20), key = (seed_lo, seed_hi), stream 0 =
 * normals, 1 = accept uniform (block 0; block s for sub-step s of a Gibbs draw). */
int ey_philox_block(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* Running per-chain moments for ChainLists.mean / R-hat style summaries (eeyore/chains/chain_lists.py:65-66,
 * eeyore/stats/multi_rhat.py:10-40): s1 += theta, s2 += theta^2 ([C,P] double accumulators), acc += accepted
 * ([C] double; `accepted` uint8 [C]; both may be NULL).  theta [C,P] of `dtype`.  One streaming pass. */
int ey_stats_update(const void* theta, const void* accepted, int64_t C, int64_t P, int dtype, void* s1, void* s2,
                    void* acc, void* stream);

/* Initial-sequence estimate of the asymptotic variance (eeyore/stats/inse_mc_cov.py:9-83) of every column of
 * x [n, S] at once, each column on its own (p = 1): S = chains * parameters of a stored run, n iterations, row-major as a
 * chain buffer [iterations, C, P] is laid out.  sig2 [S] double: the estimate (NaN where the reference raises 'Not
 * enough samples', :45-46); var [S] double: the unbiased sample variance (eeyore/stats/cov.py:5-15), so that multi_ess'
 * n * (det cov / det mc_cov)^(1/p) (eeyore/stats/multi_ess.py:6-14) is n * var / sig2; num_pairs [S] int32 or NULL: lag
 * pairs that entered the sum (-1 where not enough).  The reference's adjust=True changes nothing for p = 1. */
int ey_inse_univariate(const void* x, int64_t n, int64_t S, int dtype, void* sig2, void* var, void* num_pairs,
                       void* stream);

/* The reference's MULTIVARIATE initial-sequence estimator (eeyore/stats/inse_mc_cov.py:9-83, adjust=False) for C
 * chains of p <= 64 parameters at once (up to 16, with n p doubles inside 144 KiB, the chain lies in LDS; beyond that the
 * centred chains go through a workspace the call allocates and frees on the stream -- at most EY_MV_WORKSPACE_MB from the
 * environment, read at every call, 1024 by default, the chains taking as many launches as that needs): x is addressed as x[i * stride_n + c * stride_c + j] (elements; a chain buffer
 * [iterations, C, P] has stride_n = C*P, stride_c = P; [C, n, p] has stride_n = p, stride_c = n*p).  sig [C,p,p]
 * double: the estimate (NaN where the reference raises 'Not enough samples'); cov [C,p,p] double or NULL: the unbiased
 * sample covariance (eeyore/stats/cov.py:5-15); mean [C,p] double or NULL; num_pairs [C] int32 or NULL.  With these,
 * multi_ess (eeyore/stats/multi_ess.py:6-14) and both parts of multi_rhat (eeyore/stats/multi_rhat.py:10-40: W = the
 * mean of sig over chains, B = the covariance of the chain means) follow from [C,p,p]- and [C,p]-sized arrays. */
int ey_inse_multivariate(const void* x, int64_t n, int64_t C, int64_t p, int64_t stride_n, int64_t stride_c, int dtype,
                         void* sig, void* cov, void* mean, void* num_pairs, void* stream);

/* Sums of a homogeneous kernel function over pairs of samples, for C chains and k prefix lengths in one pass: what the
 * reference's Kernel.sum_symm_K / Kernel.sum_K compute with one Python call per pair (eeyore/kernels/kernel.py:64-101), and
 * all that squared_mmd / mmd need (eeyore/stats/discrepancy.py:3-19).  x1 is addressed as x1[i * stride1_n + c * stride1_c + j]
 * (elements; i < n1, c < C, j < p) as in ey_inse_multivariate, x2 likewise with n2 rows; stride2_c = 0: one x2 for all chains
 * (its own sum is then computed once and written to every chain's row).  For chain c and prefix t:
 *   s11[c,t] = sum_symm_K(x1_c[:len1[t]], include_diag)   s22[c,t] = sum_symm_K(x2_c[:len2[t]], include_diag)
 *   s12[c,t] = sum_K(x1_c[:len1[t]], x2_c[:len2[t]])      (each [C,k] double on the device, all three required)
 * kind / params (HOST doubles): 0 IsoSE {scale, l}: scale exp(-d2 / (2 l)) (iso_se_kernel.py:12-13); 1 RQ {scale, l, a}:
 * scale (1 + d2 / (2 a l))^-a (rq_kernel.py:13-14); 2 Periodic {scale, l, p}: scale exp(-2 sin^2(d / p) / l)
 * (periodic_kernel.py:13-14), with d2 = sum_j (a_j - b_j)^2 in the difference form and d = sqrt(d2).  Samples are f32 or f64
 * (`dtype`); arithmetic and sums are f64 for both (an f32 sample is exact in f64; the reference's f32 result is a sequential
 * f32 sum and is not imitated).  len1, len2: HOST arrays of k non-decreasing lengths in [1, n1] / [1, n2], read during the
 * call (with k > 1 the call waits for `stream` once, until they have been copied); both NULL with k = 1: the full lengths.
 * Symmetric sums count a pair below the diagonal twice and add the diagonal when include_diag != 0.  No floating-point
 * atomics: the same call gives the same bits, and so do two chains with the same data in one call.  Where there are few
 * chains their tiles are split over several workgroups, whose partial sums go through a workspace the call allocates and
 * frees on the stream and are added in a fixed order (4 workgroups per CU are aimed at; EY_MMD_SPLIT_TARGET in the
 * environment, read at every call, replaces that number).  Non-finite samples are not checked: they make that chain's
 * sums NaN and no other chain's.  EY_ERR_INVALID, before anything touches the device: n1, n2, C, p or k < 1; unknown kind or
 * dtype; scale, l or a not finite and > 0; Periodic p not finite or 0; exactly one of len1 / len2 NULL (or both with
 * k > 1); lengths decreasing or outside [1, n]; include_diag = 0 with a length < 2; a NULL pointer.  EY_ERR_UNSUPPORTED:
 * k > 1024; p > 2^31 - 17; more than 2^24 - 1 workgroups in one launch (C times the workgroups per chain: C > 16777215). */
int ey_kernel_pair_sums(const void* x1, int64_t n1, int64_t C, int64_t p, int64_t stride1_n, int64_t stride1_c,
                        const void* x2, int64_t n2, int64_t stride2_n, int64_t stride2_c, int dtype, int kind,
                        const double* params, const int64_t* len1, const int64_t* len2, int64_t k, int include_diag,
                        void* s11, void* s22, void* s12, void* stream);

/* Diagnostic (not part of the drop-in surface): the workgroups per chain of the launch that computed s11 / s12 in this
 * thread's last ey_kernel_pair_sums call that reached the device: 1 = every chain in one workgroup, > 1 = the split route. */
int ey_debug_mmd_last_split(void);

/* Attach running-moment accumulators to a plan: from now on every ey_hmc_step / ey_mala_step / ey_mh_step on it also
 * performs, for the state each chain is left in, exactly what ey_stats_update does (s1 += theta, s2 += theta^2,
 * acc += accepted) -- inside the fused kernel where there is one (no extra pass over [C,P]), as a trailing pass on
 * the same stream otherwise.  s1, s2 [C,P] double, acc [C] double, all three required; steps must then be called with
 * that same C.  s1 = NULL detaches.  (The reference keeps every sample and reduces afterwards,
 * eeyore/chains/chain_list.py:64-67, chain_lists.py:65-66; with thousands of chains the moments are kept instead.) */
int ey_plan_attach_moments(ey_plan* plan, void* s1, void* s2, void* acc, int64_t C);

/* Per-chain dual averaging of the HMC step size INSIDE the step kernels (Hoffman & Gelman 2014, algorithm 5: the
 * recurrence of eeyore/tuners/hmcda_tuner.py:43-59, which HMC.draw runs on the host after every burn-in iteration,
 * eeyore/samplers/hmc.py:158-163), so that burn-in too can run as blocks of iterations per launch (ey_hmc_run).
 * state [C,3] double, in/out: (barh, logbare, mu = log(10 e0)) per chain.  step_vec [C] of the plan's dtype: the step
 * every chain takes in its next iteration -- the kernels read it and, after each adapting iteration, write the next
 * one (it replaces the step / step_vec arguments of ey_hmc_step / ey_hmc_run while attached).  table [n,3] double on
 * the device: (1/(t + t0), sqrt(t)/gamma, t^-kappa) for the t = 1st..n-th adapting iteration, worked out by the caller
 * so that host and device agree to the last bit; the plan counts the iterations it has adapted and stops after n.
 * d: target acceptance; log_eub: log of the upper bound on the step or NaN; final_avg != 0: the n-th iteration leaves
 * the AVERAGED step exp(logbare) (hmcda_tuner.py's return_e=False).  The number of leapfrog steps stays what the calls
 * pass.  For as long as a state is attached, step_vec is the step of every HMC launch on the plan -- also after the n
 * adapting iterations are used up (the launches then read it and adapt nothing) -- and the step / step_vec arguments of
 * the calls are ignored; the plan's position in the table advances only past iterations whose launch succeeded.
 * state = NULL detaches.  Served by the fused kernel families (mfma32, fused16); EY_ERR_UNSUPPORTED otherwise. */
int ey_plan_attach_da(ey_plan* plan, void* state, void* step_vec, const void* table, int64_t n, int64_t C, double d,
                      double log_eub, int final_avg);

/* Diagnostic switches for A/B runs and tests (not part of the drop-in surface).  They are state of the PLAN:
 * ey_plan_set_variant changes one plan and returns its previous value; ey_debug_set_variant sets what plans created
 * afterwards start with (also EY_VARIANT in the environment) and returns the previous default.  Bits 0..2: workgroup
 * shape / issue-priority / parking variants of the fused f32 trajectory kernel; 4: f32 plans through the layerwise path;
 * 5, 6, 7: that path without LDS-DMA staging / fused last layer / fused leapfrog update; 8, 9: tiny models never / always
 * through the register-resident evaluation of the generic kernels; 10 (ey_debug_set_variant only): new plans, and
 * ey_debug_bgemm, start with EY_PRODUCTS_EXACT; 11: the layerwise path's bf16x3 products split the data matrix in every
 * workgroup instead of taking it pre-split; 12: the layerwise path's epilogues that read per element (prior gradient, fused
 * leapfrog update, act'(H)) element by element instead of in batches of loads; 3: the fused f32 trajectory kernel's HMC draw with
 * the pipelined tile loop at one wave per SIMD (same bits, slower: DESIGN.md 4.1.3); 13: value + gradient of mid-size models
 * (hidden widths 33 .. 128, at most two hidden layers, d_K <= 16, f32) by the fused workgroup-per-chain kernel instead of one
 * product launch per layer and direction; 14: narrow deeper models (every hidden width <= 32, up to three
 * hidden layers, up to 64 inputs, f32) through those product launches instead of the fused kernel k_mid32 that serves them
 * by default.  Results agree to rounding across them (bit for bit across bits 3, 11 and 12). */
int ey_plan_set_variant(ey_plan* plan, int variant);
int ey_debug_set_variant(int variant);

/* Test / measurement entry of the layerwise path's batched f32 product (not part of the drop-in surface):
 * C[b] = act(A[b] B[b] + bias[b]) for b < batch through the same dispatcher the evaluations use.  Element strides
 * (sAm, sAk), (sBk, sBn), (sCm, sCn), batch strides bA, bB, bC (0 = shared operand); bias may be NULL; act is an
 * EY_ACT_* code.  Parity against torch.bmm: tests/test_gpu_parity.py::test_batched_gemm_vs_torch_bmm. */
int ey_debug_bgemm(const float* A, const float* B, float* C, int M, int N, int K, long sAm, long sAk, long sBk, long sBn,
                   long sCm, long sCn, long bA, long bB, long bC, const float* bias, long bBias, int act, int batch,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEYORE_AMD_H */
