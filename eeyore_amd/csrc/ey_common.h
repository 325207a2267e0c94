// Shared host/device definitions for the eeyore_amd HIP library (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/eeyore_amd_warmup.h"  // includes eeyore_amd.h and eeyore_amd_ext.h

#define EY_MAX_LAYERS 8
#define EY_VERSION 200  // 0.2.0
#define EY_KIND_MLP 0
#define EY_KIND_MIX 1
#define EY_KIND_TILT 2  // sum_i [c_i + a_i theta_i - b_i exp(s_i theta_i)] on theta itself (ey_plan_create_exptilt)
#define EY_MIX_MAX_P 128  // RAM's and AM's limit: lane i owns rows i and i + 64
#define EY_MIX_MAX_M 16

// ----------------------------------------------------------------------------------------------- errors
void ey_set_error(const std::string& msg);
#define EY_FAIL(code, msg) \
  do {                     \
    ey_set_error(msg);     \
    return (code);         \
  } while (0)
#define EY_HIP(call)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      ey_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                            \
      return EY_ERR_HIP;                                                                          \
    }                                                                                             \
  } while (0)

// ----------------------------------------------------------------------------------------------- plan
// Device-visible model description, passed to kernels by value.
struct EyModel {
  int nl;                        // number of layers K
  int dims[EY_MAX_LAYERS + 1];   // d_0..d_K
  int bias[EY_MAX_LAYERS];
  int act[EY_MAX_LAYERS];
  int woff[EY_MAX_LAYERS];       // offset of W_l in theta
  int boff[EY_MAX_LAYERS];       // offset of b_l in theta, -1 if none
  int hoff[EY_MAX_LAYERS + 1];   // first activation row of layer l in the per-tile activation store
  int hrows;                     // sum of d_l
  int dmax;                      // max d_l
  int lik;
  int P;
  int N;                // data rows; EY_KIND_MIX: the number of components M
  int kind;             // EY_KIND_MLP, or a density on theta itself: EY_KIND_MIX (ey_plan_create_mixture), EY_KIND_TILT (_exptilt)
  const void* x;        // [N, d0]; EY_KIND_MIX: mean [M, P]; EY_KIND_TILT: c [P]
  const void* y;        // [N, dK]; EY_KIND_MIX: prec [M, P, P], row-major, symmetric; EY_KIND_TILT: a [P]
  const int* labels;    // [N] argmax(y,1) (CE)
  const void* mu;       // [P]; EY_KIND_MIX: c [M]; EY_KIND_TILT: b [P]
  const void* inv_var;  // [P] 1/sigma^2; EY_PRIOR_LAPLACE: 1/b; EY_PRIOR_STUDENT_T: 1/(nu s^2); EY_KIND_TILT: s [P]
  double prior_const;   // sum_i (-log sigma_i - 0.5 log 2pi); the other families: the table of ey_plan_set_prior_family
  const void* prior_h;  // [P] EY_PRIOR_STUDENT_T: (nu + 1)/2; null otherwise
  int prior_kind;       // EY_PRIOR_NORMAL / _LAPLACE / _STUDENT_T: which loop the tail of eval_target runs (ey_generic.hip)
  // EY_LIK_GAUSS_SUM / _LAPLACE_SUM (ey_plan_set_lik_scale): worked out in double, rounded once to the plan's dtype
  double lik_w;         // 1/s^2 (Gaussian), 1/s (Laplace)
  double lik_c;         // the log-normaliser of one output: -log(s sqrt(2 pi)) (Gaussian), -log(2 s) (Laplace)
};
// the regression codes: served by the generic kernels and the separate layerwise launches only
static inline bool ey_lik_regression(int lik) { return lik >= EY_LIK_GAUSS_SUM; }

struct ey_plan {
  EyModel m;
  int dtype;
  int device;
  bool has_data, has_prior;
  void *d_x, *d_y, *d_mu, *d_inv_var;
  void* d_prior_h = nullptr;  // the third prior table (EyModel::prior_h), allocated on first use
  double lik_scale = 1.0;     // s of EY_LIK_GAUSS_SUM / _LAPLACE_SUM (ey_plan_set_lik_scale)
  bool prior_uniform = false;  // every parameter has the same (mu, sigma)
  double prior_mu0 = 0.0, prior_iv0 = 0.0;
  // running moments attached with ey_plan_attach_moments (caller-owned device memory)
  double *mom_s1 = nullptr, *mom_s2 = nullptr, *mom_acc = nullptr;
  int64_t mom_C = 0;
  // per-chain dual averaging of the HMC step size, attached with ey_plan_attach_da (caller-owned device memory)
  double* da_state = nullptr;        // [C,3]: barh, logbare, mu
  void* da_step = nullptr;           // [C] of the plan's dtype: the step of the next iteration
  const double* da_table = nullptr;  // [da_n,3]: d_w, sqrt(t)/gamma, e_w of the k-th adapting iteration
  int64_t da_n = 0, da_done = 0, da_C = 0;
  double da_d = 0.65, da_logeub = 0.0;
  bool da_has_eub = false, da_final_avg = false;
  int* d_labels;
  // mfma32 path (4-32-32-3-like models, f32): padded/packed data image
  bool mfma32_ok;        // the model is one the fused kernel serves
  int mfma32_kind = 0;   // 1: the headline model; 2: served in the bf16x3 form only (ey_mfma32_kind)
  bool mfma32_data_ok;   // ... and the current batch fits its LDS image (recomputed by every ey_plan_set_data)
  void* d_xpack;
  int64_t cap_N;         // rows the data buffers below were allocated for (they only grow)
  // fused16 path (d0-H-H-dK with H in {16, 32, 64}, f32 and f64): operand-order data image in global memory
  bool fused16_ok = false;
  void* d_xpack16 = nullptr;
  size_t xpack16_bytes = 0;
  int n_cu;
  int variant = 0;   // diagnostic switches (ey_plan_set_variant; bits as documented in include/eeyore_amd.h)
  int products = 0;  // EY_OPT_F32_PRODUCTS: EY_PRODUCTS_BF16X3 (0) or EY_PRODUCTS_EXACT (1)
  int row_waves = 0; // EY_OPT_ROW_WAVES: EY_ROW_WAVES_OFF (0, default), _ON (1), _AUTO (2)
  int max_chunk_chains = 0;  // EY_OPT_MAX_CHUNK_CHAINS: 0 (default) the layerwise path's own rule, k > 0 at most k chains per chunk
  // layerwise batched-GEMM path for models whose parameters do not fit LDS (ey_large.hip): workspace it owns
  void* d_work;
  size_t work_bytes;
  // ... and the data matrix split into bf16 pieces once per batch, in both orientations (ey_large.hip: ensure_xpre)
  void* d_xpre = nullptr;
  size_t xpre_bytes = 0;
  hipEvent_t xpre_event = nullptr;   // recorded behind the split on the stream that ran it: a consumer on another stream waits for it
  hipStream_t xpre_stream = nullptr;
  uint64_t data_version = 0, xpre_version = ~0ull;  // ey_plan_set_data counts; the images remember which batch they hold
  // the fused narrow- and mid-size kernels (ey_mid.hip): k_mid32's parameter -> LDS table [P], built on first use, and
  // whether their LDS limit has been raised
  int* d_mid32_tab = nullptr;
  bool mid32_attr = false, mid_attr = false;
  // the NUTS kernel (ey_nuts.hip): the instantiation whose LDS limit this plan has raised (to 160 KiB, once)
  const void* nuts_attr = nullptr;
  // ... and the tree of k_nuts_ws (ey_nuts_ws.hip) in device memory, attached with ey_plan_attach_nuts_tree (caller-owned),
  // with that kernel's own raised instantiation
  void* nuts_tree = nullptr;
  int64_t nuts_tree_bytes = 0;
  const void* nuts_ws_attr = nullptr;
};

// The diagnostic switches of the plan a C-ABI call is serving, for the dispatch code below the entry points (thread-local:
// plans on different threads are independent; an entry point sets it for its own duration).
extern thread_local int t_ey_variant, t_ey_products;
struct EyVariantScope {
  int old, oldp;
  explicit EyVariantScope(int v, int products = -1) : old(t_ey_variant), oldp(t_ey_products) {
    t_ey_variant = v;
    if (products >= 0) t_ey_products = products;
  }
  explicit EyVariantScope(const struct ey_plan* pl);
  ~EyVariantScope() { t_ey_variant = old; t_ey_products = oldp; }
};
#define EY_VBIT(b) ((t_ey_variant >> (b)) & 1)
int ey_default_variant();   // what plans created now start with (ey_debug_set_variant, EY_VARIANT)
int ey_default_products();  // ... and their EY_OPT_F32_PRODUCTS (EY_F32_PRODUCTS; bit 10 of ey_debug_set_variant: exact)

inline EyVariantScope::EyVariantScope(const ey_plan* pl) : EyVariantScope(pl->variant, pl->products) {}

// what a launch needs of the attached dual averaging: the rows of the table for its iterations
struct EyDA {
  double* state = nullptr;
  void* step = nullptr;
  const double* table = nullptr;  // first row = this launch's first iteration
  int n = 0;                      // adapting iterations in this launch (the rest of the launch keeps the last step)
  int final_it = -1;              // launch-local iteration that stores exp(logbare) instead of exp(loge); -1 = none
  double d = 0.65, logeub = 0.0;
  int has_eub = 0;
};

// One update of the recurrence of eeyore/tuners/hmcda_tuner.py:43-59 for one chain (Hoffman & Gelman 2014, algorithm 5):
// returns the step of the next iteration.  row = (d_w, sqrt(t)/gamma, e_w), worked out on the host for iteration t.
__host__ __device__ inline double ey_da_update(double* st, const double* row, double rate, double d, bool has_eub,
                                               double logeub, bool averaged) {
#pragma clang fp contract(off)  // separate multiplies and adds, as the host form of the recurrence rounds them
  double barh = st[0], logbare = st[1];
  const double m = st[2];
  const double r = rate == rate ? rate : 0.0;  // a NaN rate (a rejected non-finite trajectory) counts as 0
  barh += row[0] * ((d - r) - barh);
  double loge = m - row[1] * barh;
  if (has_eub && loge > logeub) loge = logeub;
  logbare += row[2] * (loge - logbare);
  st[0] = barh;
  st[1] = logbare;
  return exp(averaged ? logbare : loge);
}

// ey_hmc_run: n_iters consecutive draws inside one launch, with optional per-iteration records
struct EyRun {
  int n_iters;
  void* samples;    // [n_iters, C, P] of the plan's dtype, or null
  void* targets;    // [n_iters, C], or null
  void* accepted;   // [n_iters, C] uint8, or null
  int* accept_count;  // [C] int32 (+=), or null
};

// One draw of every chain (or, with `run`, a run of draws) as every sampler launcher takes it: what the entry points of all
// samplers share, named, so that no two of these can change places unnoticed.  HMC writes rate / hcur / hprop instead of
// log_rate; the launchers of the layerwise path queue one iteration and read no `run`.
struct EyDraw {
  const void* temp;  // [C] tempering weights, or null
  int64_t C;
  uint64_t seed, iter, chain_offset;  // the Philox key of the first iteration
  uint32_t flags;
  void* accepted;    // [C] uint8 (Gibbs: [C, S])
  void* log_rate;    // [C] (Gibbs: [C, S]), or null
  hipStream_t s;
  const EyRun* run;  // the records of a *_run call; null: one draw, nothing recorded
};

// the attached moments from the records of a launch, in one streaming pass (ey_api.hip)
int ey_stats_update_run(const void* samples, const void* accepted_rec, int n_it, int64_t C, int64_t P, int dtype, void* s1,
                        void* s2, void* acc, void* stream);

// fused value + gradient of mid-size MLPs, f32 (ey_mid.hip)
bool ey_mid_supports(const ey_plan* pl);
int ey_mid_eval(ey_plan* pl, const float* theta, const float* temp, int C, float* lik_o, float* grad, hipStream_t s);
bool ey_mid32_supports(const ey_plan* pl);  // narrow deeper models: every hidden width <= 32, up to three hidden layers, d_0 <= 64
int ey_mid32_eval(ey_plan* pl, const float* theta, const float* temp, int C, float* lik_o, float* grad, hipStream_t s);

// generic kernels (ey_generic.hip)
int ey_generic_log_target(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* lik, void* prior,
                          void* target, void* grad, hipStream_t s);
void ey_generic_mix_scratch(EyModel& m);  // hrows / dmax of an EY_KIND_MIX model: the evaluation scratch of mix_target
void ey_generic_tilt_scratch(EyModel& m);  // ... of an EY_KIND_TILT model: none
int ey_generic_log_lik_rows(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* rows, hipStream_t s);
int ey_generic_forward(ey_plan* pl, const void* theta, int64_t C, void* out, hipStream_t s);  // out [C, N, dK] (ey_forward)
int ey_generic_hmc(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                   const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop);
int ey_generic_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                        int64_t C, void* target, void* grad, hipStream_t s);
int ey_generic_mala(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                    const void* step_vec, const EyDraw& d);
int ey_generic_mh(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
                  const EyDraw& d);
// robust adaptive Metropolis (k_ram): every model whose factor fits beside the evaluation image, whatever plan.kernel says
size_t ey_generic_ram_lds(const ey_plan* pl);  // dynamic LDS of one chain's workgroup
int ey_generic_ram(ey_plan* pl, void* theta, void* target, void* chol, const void* z, const void* u, double a, double g,
                   uint64_t n, const EyDraw& d);
// MH with a fixed lower-triangular proposal factor (k_mh_tril): as RAM, whatever plan.kernel says
size_t ey_generic_mh_tril_lds(const ey_plan* pl);  // dynamic LDS of one chain's workgroup
int ey_generic_mh_tril(ey_plan* pl, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                       const void* z, const void* u, const EyDraw& d);
// MALA with a fixed lower-triangular proposal factor (k_mala_tril): as k_mh_tril, whatever plan.kernel says
size_t ey_generic_mala_tril_lds(const ey_plan* pl);  // dynamic LDS of one chain's workgroup
int ey_generic_mala_tril(ey_plan* pl, void* theta, void* target, void* grad, const void* tril, int64_t G,
                         const void* tril_index, const void* z, const void* u, double step, const void* step_vec,
                         const EyDraw& d);
// HMC with a fixed metric, EY_METRIC_DIAG or EY_METRIC_TRIL (k_hmc_metric): one wave per chain, whatever plan.kernel says
size_t ey_generic_hmc_metric_lds(const ey_plan* pl, int form);  // dynamic LDS of one chain's workgroup
int ey_generic_hmc_metric(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                          const void* metric_index, const void* v0, const void* u, double step, const void* step_vec, int L,
                          const EyDraw& d, void* rate, void* hcur, void* hprop);
// the warm-up form of the metric draw loop (k_hmc_metric_warmup): what a launch adds to ey_generic_hmc_metric's run of
// draws, every pointer optional.  The dual averaging is EyDA's, as arguments of the call.
struct EyWarm {
  double* da_state;        // [C,3]: barh, logbare, mu; null: no dual averaging
  const double* da_table;  // [da_n,3]: first row = this launch's first draw
  int da_n;                // adapting draws in this launch (the rest of the launch keeps the last step)
  int final_it;            // launch-local draw that stores exp(logbare) instead of exp(loge); -1 = none
  double d, logeub;
  int has_eub;
  double *mean, *M2;       // [C,P] and [C,P] (EY_METRIC_DIAG) or [C,P,P] (EY_METRIC_TRIL, j <= i only); null: no moments
  int64_t count;           // draws already in the moments
  void *steps_rec, *rate_rec;  // [n_iters,C] of the plan's dtype, or null
};
int ey_generic_hmc_metric_warmup(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form,
                                 int64_t G, const void* metric_index, double step, void* step_vec, int L, const EyDraw& d,
                                 const EyWarm& w);

#define EY_AM_RIDGE 0
#define EY_AM_SOFTABS 1
// adaptive Metropolis (k_am): the state and the settings of AM.draw beside theta and target, whatever plan.kernel says
struct EyAm {
  void* mean;           // [C, P] running_mean, in/out
  void* cov_sum;        // [C, P, P] sum of theta theta^T, in/out (j <= i only)
  void* cov;            // [C, P, P] the proposal covariance, in/out (j <= i only)
  int* num_accepted;    // [C] int32, in/out
  const void* cov0;     // [P, P] or [C, P, P]: the transformed initial covariance
  int cov0_per_chain;
  double l, b, c, eps;  // eps: the ridge (EY_AM_RIDGE) or softabs's a (EY_AM_SOFTABS)
  int64_t t0, idx, offset;
  const void *z, *u_mix, *u;  // recorded draws [C, P], [C], [C], or null
  unsigned char* branch;      // [C] 0 isotropic, 1 factor, 2 breakdown; or null
  int* breakdowns;            // [C] int32 (+=)
};
size_t ey_generic_am_lds(const ey_plan* pl, int transform = EY_AM_RIDGE);  // dynamic LDS of one chain's workgroup
bool ey_generic_am_softabs_fits(const ey_plan* pl);  // P <= 128 and the softabs instantiation's LDS fits a CU
// softabs of B dense symmetric [P, P] matrices (k_softabs), the device function k_am's softabs instantiation runs
int ey_generic_softabs(const void* A, int64_t B, int P, int dtype, double a, void* out, void* sweeps, hipStream_t s);
int ey_generic_am(ey_plan* pl, void* theta, void* target, const EyAm& am, const EyDraw& d, int transform);

// node-blocked Metropolis-within-Gibbs (k_gibbs): blockwise random-walk Metropolis over a table of disjoint index sets
struct ey_gibbs_table {
  int64_t P;       // parameters of the model the table was built for
  int S, n_idx;    // sub-steps per draw, indices in all of them together
  int dtype, device;
  int* d_off;      // [S + 1] device: sub-step s owns d_idx[d_off[s] .. d_off[s + 1])
  int* d_idx;      // [n_idx] device
  void* d_scale;   // [S] device, of dtype
};
size_t ey_generic_gibbs_lds(const ey_plan* pl, const ey_gibbs_table* tb);  // dynamic LDS of one chain's workgroup
int ey_generic_gibbs(ey_plan* pl, const ey_gibbs_table* tb, void* theta, void* target, const void* z, const void* u,
                     const EyDraw& d, double* mom_acc);  // EY_GIBBS_CARRY of d.flags: mode 'reference'

// layerwise batched-GEMM kernels for large models, f32 (ey_large.hip)
bool ey_large_needed(const ey_plan* pl, int nvec = 3);  // true when the generic kernels cannot hold the model in LDS
int ey_large_log_target(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* lik, void* prior,
                        void* target, void* grad, hipStream_t s);
int ey_large_hmc(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                 const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop);
int ey_large_mala_mh(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                     const void* step_vec, const void* scale, const EyDraw& d);
int ey_large_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                      int64_t C, void* target, void* grad, hipStream_t s);
int ey_large_log_lik_rows(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* rows, hipStream_t s);
int ey_large_forward(ey_plan* pl, const void* theta, int64_t C, void* out, hipStream_t s);  // out [C, N, dK] (ey_forward)
void ey_large_free(ey_plan* pl);

// mfma32 kernels (ey_mfma32.hip)
bool ey_mfma32_supports(const ey_plan* pl);
int ey_mfma32_kind(const ey_plan* pl);  // 1 the headline model, 2 served in the bf16x3 form only, 0 not served
int ey_mfma32_set_data(ey_plan* pl, hipStream_t s);
int ey_mfma32_hmc(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                  const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop, const EyDA* da);
int ey_mfma32_log_target_grad(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* target, void* grad,
                              hipStream_t s);
int ey_mfma32_mala(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                   const void* step_vec, const EyDraw& d);
int ey_mfma32_mh(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
                 const EyDraw& d);
int ey_mfma32_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                       int64_t C, void* target, void* grad, hipStream_t s);

// fused kernels on 16x16x4 tiles (ey_fused16.hip)
bool ey_fused16_supports(const ey_plan* pl);
int ey_fused16_set_data(ey_plan* pl, hipStream_t s);
int ey_fused16_hmc(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                   const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop, const EyDA* da);
int ey_fused16_mala(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                    const void* step_vec, const EyDraw& d);
int ey_fused16_mh(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
                  const EyDraw& d);
int ey_fused16_log_target(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* lik, void* prior,
                          void* target, void* grad, hipStream_t s);
int ey_fused16_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                        int64_t C, void* target, void* grad, hipStream_t s);

// ----------------------------------------------------------------------------------------------- Philox4x32-10
// Counter-based generator (Salmon et al. 2011).  One call per (element, chain, iteration, stream): the value a
// lane needs never depends on which lane asks, so every kernel layout reproduces the same stream.
#define EY_STREAM_NORMAL 0u
#define EY_STREAM_UNIFORM 1u
#define EY_STREAM_PT 2u  // the between-chain move of a tempering ladder (k_pt_between): Philox block i = step i of the move

struct EyRng {
  uint32_t k0, k1;  // key = seed
  uint32_t c1, c2, c3;  // chain, iter_lo, (iter_hi << 8) | stream
};

__host__ __device__ inline void ey_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1, uint32_t out[4]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__host__ __device__ inline EyRng ey_rng_make(uint64_t seed, uint64_t chain, uint64_t iter, uint32_t stream) {
  EyRng r;
  r.k0 = (uint32_t)seed;
  r.k1 = (uint32_t)(seed >> 32);
  r.c1 = (uint32_t)chain;
  r.c2 = (uint32_t)iter;
  r.c3 = ((uint32_t)(iter >> 32) << 8) | (stream & 0xffu) | ((uint32_t)(chain >> 32) << 20);
  return r;
}

// N(0,1) for the four elements 4b .. 4b+3 of a chain's stream ("block" b): element idx is component idx & 3 of block
// idx >> 2, whoever computes it, so every kernel layout reproduces the same stream.  f32: ONE Philox call per block,
// two Box-Muller pairs on 24-bit uniforms (o0,o1 -> elements 0,1 as r cos, r sin; o2,o3 -> elements 2,3).  f64: two
// calls (counters 2b and 2b+1), one Box-Muller pair on 32+21-bit uniforms each.  The 32-bit integer multiplies of
// Philox are quarter rate and the generator is a visible share of a draw (all of a MALA / MH draw's prologue), so
// producers generate whole blocks.  Contraction is off so that the fused kernels and ey_philox_normal produce
// bit-identical values.
template <typename T>
__device__ inline void ey_rng_normal4(const EyRng& r, uint32_t block, T out[4]);

template <>
__device__ inline void ey_rng_normal4<float>(const EyRng& r, uint32_t block, float out[4]) {
#pragma clang fp contract(off)
  uint32_t o[4];
  ey_philox4x32_10(block, r.c1, r.c2, r.c3, r.k0, r.k1, o);
#pragma unroll
  for (int pair = 0; pair < 2; ++pair) {
    const float u1 = ((float)(o[2 * pair] >> 8) + 0.5f) * 5.9604644775390625e-08f;  // (0,1)
    const float u2 = (float)(o[2 * pair + 1] >> 8) * 5.9604644775390625e-08f;       // [0,1)
    const float rad = sqrtf(-2.0f * logf(u1));
    out[2 * pair] = rad * cospif(2.0f * u2);
    out[2 * pair + 1] = rad * sinpif(2.0f * u2);
  }
}

template <>
__device__ inline void ey_rng_normal4<double>(const EyRng& r, uint32_t block, double out[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int pair = 0; pair < 2; ++pair) {
    uint32_t o[4];
    ey_philox4x32_10(2u * block + (uint32_t)pair, r.c1, r.c2, r.c3, r.k0, r.k1, o);
    const double u1 = ((double)(((uint64_t)o[0] << 21) | (o[2] >> 11)) + 0.5) * 1.1102230246251565e-16;  // 2^-53
    const double u2 = (double)(((uint64_t)o[1] << 21) | (o[3] >> 11)) * 1.1102230246251565e-16;
    const double rad = sqrt(-2.0 * log(u1));
    out[2 * pair] = rad * cospi(2.0 * u2);
    out[2 * pair + 1] = rad * sinpi(2.0 * u2);
  }
}

// one element (for consumers that are handed single indices): the same arithmetic, the other components discarded
template <typename T>
__device__ inline T ey_rng_normal(const EyRng& r, uint32_t idx) {
  T o[4];
  ey_rng_normal4<T>(r, idx >> 2, o);
  return o[idx & 3u];
}

template <typename T>
__device__ inline T ey_rng_uniform(const EyRng& r);

template <>
__device__ inline float ey_rng_uniform<float>(const EyRng& r) {
  uint32_t o[4];
  ey_philox4x32_10(0u, r.c1, r.c2, r.c3, r.k0, r.k1, o);
  return (float)(o[0] >> 8) * 5.9604644775390625e-08f;
}
template <>
__device__ inline double ey_rng_uniform<double>(const EyRng& r) {
  uint32_t o[4];
  ey_philox4x32_10(0u, r.c1, r.c2, r.c3, r.k0, r.k1, o);
  return (double)(((uint64_t)o[0] << 21) | (o[1] >> 11)) * 1.1102230246251565e-16;
}

// The accept stream at block word `block`: Gibbs draws one accept variate per sub-step s of a (chain, iteration) with
// block = s, so sub-step 0 draws ey_rng_uniform's variate (the same arithmetic on the words of Philox block `block`).
template <typename T>
__device__ inline T ey_rng_uniform_at(const EyRng& r, uint32_t block);

template <>
__device__ inline float ey_rng_uniform_at<float>(const EyRng& r, uint32_t block) {
  uint32_t o[4];
  ey_philox4x32_10(block, r.c1, r.c2, r.c3, r.k0, r.k1, o);
  return (float)(o[0] >> 8) * 5.9604644775390625e-08f;
}
template <>
__device__ inline double ey_rng_uniform_at<double>(const EyRng& r, uint32_t block) {
  uint32_t o[4];
  ey_philox4x32_10(block, r.c1, r.c2, r.c3, r.k0, r.k1, o);
  return (double)(((uint64_t)o[0] << 21) | (o[1] >> 11)) * 1.1102230246251565e-16;
}

// The exchange decision of PowerPosteriorSampler.between_chain_move (power_posterior_sampler.py:135-141,160) with
// T_k = t_k * ell:  log_rate = dlogq + (t_i - t_j) * (ell_j - ell_i), swap iff log(u) < log_rate.  k_pt_swap (ey_api.hip) and
// k_pt_between (ey_pt.hip) both decide through this function.  Contraction is off: the product is rounded before dlogq
// is added, as the torch expressions of the host path round it, whichever kernel the function is inlined into.
template <typename T>
__device__ inline bool ey_pt_decide(T ell_i, T ell_j, T t_i, T t_j, const T* dlogq, T u, T* log_rate) {
#pragma clang fp contract(off)
  T lr = (t_i - t_j) * (ell_j - ell_i);
  if (dlogq) lr += *dlogq;
  const T lu = sizeof(T) == 4 ? (T)logf((float)u) : (T)log((double)u);
  *log_rate = lr;
  return lu < lr;  // :160
}
