// C-ABI entry points (include/eeyore_amd.h): argument validation, plan management, dispatch to the kernel
// families.  No torch types cross this boundary.
#include <math.h>

#include <atomic>
#include <cstring>
#include <optional>
#include <vector>

#include "ey_common.h"
#include "ey_nuts.h"
#include "ey_eslice.h"
#include "ey_hmc_metric_mfma.h"

static thread_local std::string g_err;
void ey_set_error(const std::string& msg) { g_err = msg; }

// labels = argmax(y, 1), first maximal index (eeyore/constants/constants.py:17)
template <typename T>
__global__ void k_labels(const T* __restrict__ y, int* __restrict__ labels, int64_t N, int dK) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int best = 0;
  T bv = y[n * dK];
  for (int j = 1; j < dK; ++j) {
    const T v = y[n * dK + j];
    if (v > bv) { bv = v; best = j; }
  }
  labels[n] = best;
}

thread_local int t_ey_variant = 0, t_ey_products = EY_PRODUCTS_BF16X3;
// what a new plan starts with: EY_VARIANT / EY_F32_PRODUCTS in the environment, or ey_debug_set_variant
static std::atomic<int> g_ey_default_variant{[] { const char* e = getenv("EY_VARIANT"); return e ? atoi(e) & 32767 : 0; }()};
int ey_default_variant() { return g_ey_default_variant.load() & (32767 & ~1024); }
int ey_default_products() {
  if (g_ey_default_variant.load() & 1024) return EY_PRODUCTS_EXACT;
  const char* e = getenv("EY_F32_PRODUCTS");
  return (e && (!strcmp(e, "exact") || !strcmp(e, "1"))) ? EY_PRODUCTS_EXACT : EY_PRODUCTS_BF16X3;
}

static size_t esize(const ey_plan* pl) { return pl->dtype == EY_F32 ? 4 : 8; }
// The constants of EY_LIK_GAUSS_SUM / _LAPLACE_SUM for the scale s, in double, rounded once to the plan's dtype (as the prior
// tables are): lik_w = 1/s^2 or 1/s, lik_c = the log-normaliser of one output.  The other codes read neither.
static void set_lik_constants(ey_plan* pl, double s) {
  EyModel& m = pl->m;
  double w = 0.0, c = 0.0;
  if (m.lik == EY_LIK_GAUSS_SUM) { w = 1.0 / (s * s); c = -log(s) - 0.91893853320467274178; }
  if (m.lik == EY_LIK_LAPLACE_SUM) { w = 1.0 / s; c = -log(2.0 * s); }
  if (pl->dtype == EY_F32) { w = (double)(float)w; c = (double)(float)c; }
  m.lik_w = w;
  m.lik_c = c;
  pl->lik_scale = s;
}
// a plan whose target is a density on theta itself (ey_plan_create_mixture, ey_plan_create_exptilt): no data, prior or network
static bool is_mix(const ey_plan* pl) { return pl->m.kind == EY_KIND_MIX || pl->m.kind == EY_KIND_TILT; }
// ... as the messages name it
static std::string mix_noun(const ey_plan* pl) { return pl->m.kind == EY_KIND_MIX ? "a mixture plan" : "a distribution plan"; }

extern "C" {

int ey_version(void) { return EY_VERSION; }
const char* ey_last_error(void) { return g_err.c_str(); }

int ey_plan_create(ey_plan** out, int n_layers, const int* dims, const int* bias, const int* act, int likelihood,
                   int dtype, int device_id) {
  if (!out || !dims || !act) EY_FAIL(EY_ERR_INVALID, "ey_plan_create: null argument");
  // Hyperparameters: len(dims) >= 3 and len(dims) == len(activations)+1 (eeyore/models/mlp.py:15-19).  A
  // single layer (logistic regression, eeyore/models/logistic_regression.py) is accepted as the K=1 case.
  if (n_layers < 1 || n_layers > EY_MAX_LAYERS) EY_FAIL(EY_ERR_INVALID, "ey_plan_create: n_layers must be in 1..8");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_plan_create: dtype must be EY_F32 or EY_F64");
  if (likelihood < EY_LIK_BCE_SUM || likelihood > EY_LIK_POISSON_SUM)
    EY_FAIL(EY_ERR_INVALID, "ey_plan_create: unknown likelihood");
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1) EY_FAIL(EY_ERR_INVALID, "ey_plan_create: dims must be positive");
  for (int l = 0; l < n_layers; ++l)
    if (act[l] < EY_ACT_NONE || act[l] > EY_ACT_RELU) EY_FAIL(EY_ERR_INVALID, "ey_plan_create: unknown activation");
  int ndev = 0;
  EY_HIP(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) EY_FAIL(EY_ERR_INVALID, "ey_plan_create: no such device");
  ey_plan* pl = new ey_plan();
  EyModel& m = pl->m;
  m.nl = n_layers;
  int P = 0, hr = 0, dmax = 0;
  for (int l = 0; l <= n_layers; ++l) {
    m.dims[l] = dims[l];
    m.hoff[l] = hr;
    hr += dims[l];
    if (dims[l] > dmax) dmax = dims[l];
  }
  for (int l = 0; l < n_layers; ++l) {
    m.bias[l] = bias ? (bias[l] != 0) : 1;
    m.act[l] = act[l];
    m.woff[l] = P;
    P += dims[l + 1] * dims[l];
    m.boff[l] = m.bias[l] ? P : -1;
    if (m.bias[l]) P += dims[l + 1];
  }
  m.hrows = hr;
  m.dmax = dmax;
  m.lik = likelihood;
  m.P = P;
  m.N = 0;
  m.kind = EY_KIND_MLP;
  m.x = m.y = m.mu = m.inv_var = nullptr;
  m.labels = nullptr;
  m.prior_const = 0.0;
  m.prior_h = nullptr;
  m.prior_kind = EY_PRIOR_NORMAL;
  pl->dtype = dtype;
  set_lik_constants(pl, 1.0);
  pl->device = device_id;
  pl->has_data = pl->has_prior = false;
  pl->d_x = pl->d_y = pl->d_mu = pl->d_inv_var = nullptr;
  pl->d_labels = nullptr;
  pl->d_xpack = nullptr;
  pl->cap_N = 0;
  pl->mfma32_data_ok = false;
  pl->d_work = nullptr;
  pl->work_bytes = 0;
  hipDeviceProp_t prop;
  EY_HIP(hipGetDeviceProperties(&prop, device_id));
  pl->n_cu = prop.multiProcessorCount;
  pl->variant = g_ey_default_variant.load() & (32767 & ~1024);
  pl->products = (g_ey_default_variant.load() & 1024) ? EY_PRODUCTS_EXACT : ey_default_products();
  {
    const char* e = getenv("EY_ROW_WAVES");
    pl->row_waves = (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : EY_ROW_WAVES_OFF;
  }
  pl->mfma32_kind = ey_mfma32_kind(pl);
  pl->mfma32_ok = pl->mfma32_kind != 0;
  pl->fused16_ok = ey_fused16_supports(pl);  // also the headline model's second choice (batches beyond mfma32's row limit)
  *out = pl;
  return EY_OK;
}

// A Gaussian-mixture target on theta itself (eeyore/models/distribution_model.py with a closure that is a multivariate
// normal or a mixture of them).  Everything is validated on the host before the device is touched.
int ey_plan_create_mixture(ey_plan** out, int64_t P, int M, const double* c, const double* mean, const double* prec,
                           int dtype, int device_id) {
  const char* who = "ey_plan_create_mixture";
  if (!out) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  *out = nullptr;
  if (!c || !mean || !prec) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": dtype must be EY_F32 or EY_F64");
  if (P < 1) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": P must be >= 1");
  if (M < 1) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": M must be >= 1");
  if (P > EY_MIX_MAX_P)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": P = " + std::to_string(P) + " exceeds the limit of " +
                                    std::to_string(EY_MIX_MAX_P) + " parameters");
  if (M > EY_MIX_MAX_M)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": M = " + std::to_string(M) + " exceeds the limit of " +
                                    std::to_string(EY_MIX_MAX_M) + " components");
  for (int k = 0; k < M; ++k) {
    if (!std::isfinite(c[k])) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": c[" + std::to_string(k) + "] is not finite");
    const double* Lk = prec + (size_t)k * P * P;
    for (int64_t i = 0; i < P; ++i) {
      if (!std::isfinite(mean[k * P + i]))
        EY_FAIL(EY_ERR_INVALID, std::string(who) + ": mean of component " + std::to_string(k) + " is not finite");
      for (int64_t j = 0; j < P; ++j)
        if (!std::isfinite(Lk[i * P + j]))
          EY_FAIL(EY_ERR_INVALID, std::string(who) + ": prec of component " + std::to_string(k) + " is not finite");
    }
    for (int64_t i = 0; i < P; ++i) {
      if (!(Lk[i * P + i] > 0.0))
        EY_FAIL(EY_ERR_INVALID, std::string(who) + ": prec of component " + std::to_string(k) +
                                    " has a diagonal entry that is not > 0");
      for (int64_t j = 0; j < i; ++j)
        if (Lk[i * P + j] != Lk[j * P + i])
          EY_FAIL(EY_ERR_INVALID, std::string(who) + ": prec of component " + std::to_string(k) +
                                      " is not exactly symmetric (the kernel reads columns for rows)");
    }
  }
  ey_plan* pl = new ey_plan();
  EyModel& m = pl->m;
  memset(&m, 0, sizeof(m));
  m.kind = EY_KIND_MIX;
  m.nl = 1;
  m.dims[0] = m.dims[1] = 1;
  for (int l = 0; l < EY_MAX_LAYERS; ++l) m.boff[l] = -1;
  m.P = (int)P;
  m.N = M;
  ey_generic_mix_scratch(m);
  pl->dtype = dtype;
  pl->device = device_id;
  pl->has_data = pl->has_prior = true;  // the tables are the data: nothing to attach
  pl->d_x = pl->d_y = pl->d_mu = pl->d_inv_var = nullptr;
  pl->d_labels = nullptr;
  pl->d_xpack = nullptr;
  pl->cap_N = 0;
  pl->mfma32_ok = pl->mfma32_data_ok = false;
  pl->d_work = nullptr;
  pl->work_bytes = 0;
  pl->n_cu = 0;
  // the kernel that needs the most LDS: AM, two packed triangles beside the image
  if (ey_generic_am_lds(pl) > 160 * 1024 || ey_generic_ram_lds(pl) > 160 * 1024) {
    const size_t need = std::max(ey_generic_am_lds(pl), ey_generic_ram_lds(pl));
    delete pl;
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": the evaluation image and AM's covariance triangles (" +
                                    std::to_string(need) + " bytes) do not fit the 160 KiB LDS of a CU");
  }
  // ---- the device from here on
  auto fail = [&](int code, const std::string& msg) {
    (void)hipFree(pl->d_x); (void)hipFree(pl->d_y); (void)hipFree(pl->d_mu);
    delete pl;
    ey_set_error(msg);
    return code;
  };
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return fail(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev) return fail(EY_ERR_INVALID, std::string(who) + ": no such device");
  hipDeviceProp_t prop;
  if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
    return fail(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  pl->n_cu = prop.multiProcessorCount;
  pl->variant = g_ey_default_variant.load() & (32767 & ~1024);
  pl->products = ey_default_products();
  pl->row_waves = EY_ROW_WAVES_OFF;
  // tables of the plan's dtype: computed in double by the caller, rounded once here
  const size_t es = esize(pl), nm = (size_t)M * P, np = nm * P;
  std::vector<float> f32;
  auto upload = [&](void** dst, const double* src, size_t n) -> hipError_t {
    hipError_t r = hipMalloc(dst, es * n);
    if (r != hipSuccess) return r;
    if (es == 8) return hipMemcpy(*dst, src, es * n, hipMemcpyHostToDevice);
    f32.assign(src, src + n);
    return hipMemcpy(*dst, f32.data(), es * n, hipMemcpyHostToDevice);
  };
  if ((e = upload(&pl->d_x, mean, nm)) != hipSuccess || (e = upload(&pl->d_y, prec, np)) != hipSuccess ||
      (e = upload(&pl->d_mu, c, (size_t)M)) != hipSuccess)
    return fail(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  m.x = pl->d_x;
  m.y = pl->d_y;
  m.mu = pl->d_mu;
  *out = pl;
  return EY_OK;
}

// A separable exponential-tilt target on theta itself: log p = sum_i [c_i + a_i theta_i - b_i exp(s_i theta_i)], the densities
// of the reference's Gamma examples (theta = log x, the Jacobian in the closure) and their relatives.
// Everything is validated on the host before the device is touched.
int ey_plan_create_exptilt(ey_plan** out, int64_t P, const double* c, const double* a, const double* b, const double* s,
                           int dtype, int device_id) {
  const char* who = "ey_plan_create_exptilt";
  if (!out) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  *out = nullptr;
  if (!c || !a || !b || !s) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": dtype must be EY_F32 or EY_F64");
  if (P < 1) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": P must be >= 1");
  if (P > EY_MIX_MAX_P)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": P = " + std::to_string(P) + " exceeds the limit of " +
                                    std::to_string(EY_MIX_MAX_P) + " parameters");
  for (int64_t i = 0; i < P; ++i) {
    const std::string at = "[" + std::to_string(i) + "]";
    if (!std::isfinite(c[i])) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": c" + at + " is not finite");
    if (!std::isfinite(a[i])) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": a" + at + " is not finite");
    if (!std::isfinite(b[i])) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": b" + at + " is not finite");
    if (!std::isfinite(s[i])) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": s" + at + " is not finite");
    if (!(b[i] > 0.0)) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": b" + at + " is not > 0");
    if (s[i] == 0.0) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": s" + at + " is 0");
    if (!(a[i] / s[i] > 0.0))
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": a" + at + " / s" + at + " is not > 0 (the density is not proper)");
  }
  ey_plan* pl = new ey_plan();
  EyModel& m = pl->m;
  memset(&m, 0, sizeof(m));
  m.kind = EY_KIND_TILT;
  m.nl = 1;
  m.dims[0] = m.dims[1] = 1;
  for (int l = 0; l < EY_MAX_LAYERS; ++l) m.boff[l] = -1;
  m.P = (int)P;
  m.N = 1;
  ey_generic_tilt_scratch(m);
  pl->dtype = dtype;
  pl->device = device_id;
  pl->has_data = pl->has_prior = true;  // the tables are the data: nothing to attach
  pl->d_x = pl->d_y = pl->d_mu = pl->d_inv_var = nullptr;
  pl->d_labels = nullptr;
  pl->d_xpack = nullptr;
  pl->cap_N = 0;
  pl->mfma32_ok = pl->mfma32_data_ok = false;
  pl->d_work = nullptr;
  pl->work_bytes = 0;
  pl->n_cu = 0;
  // the kernel that needs the most LDS: AM, two packed triangles beside the image
  if (ey_generic_am_lds(pl) > 160 * 1024 || ey_generic_ram_lds(pl) > 160 * 1024) {
    const size_t need = std::max(ey_generic_am_lds(pl), ey_generic_ram_lds(pl));
    delete pl;
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": the evaluation image and AM's covariance triangles (" +
                                    std::to_string(need) + " bytes) do not fit the 160 KiB LDS of a CU");
  }
  // ---- the device from here on
  auto fail = [&](int code, const std::string& msg) {
    (void)hipFree(pl->d_x); (void)hipFree(pl->d_y); (void)hipFree(pl->d_mu); (void)hipFree(pl->d_inv_var);
    delete pl;
    ey_set_error(msg);
    return code;
  };
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return fail(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev) return fail(EY_ERR_INVALID, std::string(who) + ": no such device");
  hipDeviceProp_t prop;
  if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
    return fail(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  pl->n_cu = prop.multiProcessorCount;
  pl->variant = g_ey_default_variant.load() & (32767 & ~1024);
  pl->products = ey_default_products();
  pl->row_waves = EY_ROW_WAVES_OFF;
  // tables of the plan's dtype: computed in double by the caller, rounded once here
  const size_t es = esize(pl);
  std::vector<float> f32;
  auto upload = [&](void** dst, const double* src) -> hipError_t {
    hipError_t r = hipMalloc(dst, es * P);
    if (r != hipSuccess) return r;
    if (es == 8) return hipMemcpy(*dst, src, es * P, hipMemcpyHostToDevice);
    f32.assign(src, src + P);
    return hipMemcpy(*dst, f32.data(), es * P, hipMemcpyHostToDevice);
  };
  if ((e = upload(&pl->d_x, c)) != hipSuccess || (e = upload(&pl->d_y, a)) != hipSuccess ||
      (e = upload(&pl->d_mu, b)) != hipSuccess || (e = upload(&pl->d_inv_var, s)) != hipSuccess)
    return fail(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  m.x = pl->d_x;
  m.y = pl->d_y;
  m.mu = pl->d_mu;
  m.inv_var = pl->d_inv_var;
  *out = pl;
  return EY_OK;
}

int ey_plan_destroy(ey_plan* pl) {
  if (!pl) return EY_OK;
  (void)hipSetDevice(pl->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(pl->d_x);
  (void)hipFree(pl->d_y);
  (void)hipFree(pl->d_mu);
  (void)hipFree(pl->d_inv_var);
  (void)hipFree(pl->d_prior_h);
  (void)hipFree(pl->d_labels);
  (void)hipFree(pl->d_xpack);
  (void)hipFree(pl->d_xpack16);
  ey_large_free(pl);
  delete pl;
  return EY_OK;
}

int ey_plan_num_params(const ey_plan* pl, int64_t* P) {
  if (!pl || !P) EY_FAIL(EY_ERR_INVALID, "ey_plan_num_params: null argument");
  *P = pl->m.P;
  return EY_OK;
}

// Diagnostic switches for A/B runs and tests (not part of the reference-facing surface).  They belong to the plan:
// ey_plan_set_variant changes one plan, ey_debug_set_variant the value plans created afterwards start with (and what
// ey_debug_bgemm, which has no plan, runs under).  Both return the previous value.
extern "C" int ey_debug_set_variant(int v) { return g_ey_default_variant.exchange(v & 32767); }
extern "C" int ey_plan_set_variant(ey_plan* pl, int v) {
  if (!pl) return -1;
  const int old = pl->variant;
  pl->variant = v & (32767 & ~1024);
  return old;
}
extern "C" int ey_plan_set_option(ey_plan* pl, int option, int value) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_option: null plan");
  if (option == EY_OPT_F32_PRODUCTS) {
    if (value != EY_PRODUCTS_BF16X3 && value != EY_PRODUCTS_EXACT)
      EY_FAIL(EY_ERR_INVALID, "ey_plan_set_option: EY_OPT_F32_PRODUCTS takes EY_PRODUCTS_BF16X3 or EY_PRODUCTS_EXACT");
    pl->products = value;
    return EY_OK;
  }
  if (option == EY_OPT_ROW_WAVES) {
    if (value < EY_ROW_WAVES_OFF || value > EY_ROW_WAVES_AUTO)
      EY_FAIL(EY_ERR_INVALID, "ey_plan_set_option: EY_OPT_ROW_WAVES takes EY_ROW_WAVES_OFF, _ON or _AUTO");
    pl->row_waves = value;
    return EY_OK;
  }
  if (option == EY_OPT_MAX_CHUNK_CHAINS) {
    if (value < 0)
      EY_FAIL(EY_ERR_INVALID, "ey_plan_set_option: EY_OPT_MAX_CHUNK_CHAINS takes 0 (the default rule) or a positive chain count");
    pl->max_chunk_chains = value;
    return EY_OK;
  }
  EY_FAIL(EY_ERR_INVALID, "ey_plan_set_option: unknown option");
}
extern "C" int ey_plan_get_option(const ey_plan* pl, int option, int* value) {
  if (!pl || !value) EY_FAIL(EY_ERR_INVALID, "ey_plan_get_option: null argument");
  if (option == EY_OPT_F32_PRODUCTS) { *value = pl->products; return EY_OK; }
  if (option == EY_OPT_ROW_WAVES) { *value = pl->row_waves; return EY_OK; }
  if (option == EY_OPT_MAX_CHUNK_CHAINS) { *value = pl->max_chunk_chains; return EY_OK; }
  EY_FAIL(EY_ERR_INVALID, "ey_plan_get_option: unknown option");
}
// the fused MFMA kernel serves this plan with the batch it currently holds
static bool prior_normal(const ey_plan* pl) { return pl->m.prior_kind == EY_PRIOR_NORMAL; }
static const char* prior_name(const ey_plan* pl) {
  return pl->m.prior_kind == EY_PRIOR_LAPLACE ? "Laplace" : pl->m.prior_kind == EY_PRIOR_STUDENT_T ? "Student-t" : "Normal";
}
static bool use_mfma32(const ey_plan* pl) {
  if (!prior_normal(pl)) return false;  // the fused families carry Normal-prior code only (ey_plan_set_prior_family)
  if (!pl->mfma32_ok || !(pl->mfma32_data_ok || !pl->has_data)) return false;
  if (pl->mfma32_kind == 2)  // the other 4-32-32 models: the bf16x3 form only, whose LDS image holds 16 row tiles
    return pl->products == EY_PRODUCTS_BF16X3 && !(t_ey_variant & 1) && (!pl->has_data || pl->m.N <= 512);
  return true;
}
// nvec: state vectors the generic kernel of the calling operation keeps in LDS (2 value/MH, 3 HMC, 4 MALA)
// The layerwise path is NEEDED when the generic kernel's LDS image does not fit, and PREFERRED for models that fit but
// are wide enough for 32-wide matrix tiles to beat one wave's vector ALUs: measured (tools/route_probe.py, any number
// of chains, any row count) the crossover is at sum_l d_l d_{l+1} ~ 600 in f32 (MLP(4-70-3) 0.9 x, MLP(12-48-6) 2 x,
// MLP(10-100-10) 6-7 x the generic kernel) and below 240 in f64 (MLP(6-24-4) 1.3 x, MLP(4-70-3) 2.3 x).  Re-measured
// over 64 .. 16384 chains with the blocked generic loop (tools/route_probe_chains.py): MLP(10-30-10), sum 600, is
// 1.6-2.9 x faster layerwise in f32 at every chain count, MLP(4-70-3), sum 490, 0.7 x from 1024 chains up: 560.
// EY_FORCE_GENERIC overrides the preference, not the need.
static bool prefer_large(const ey_plan* pl) {
  long w = 0;
  for (int l = 0; l < pl->m.nl; ++l) w += (long)pl->m.dims[l] * pl->m.dims[l + 1];
  return w >= (pl->dtype == EY_F32 ? 560 : 200);
}
static bool use_large(const ey_plan* pl, int nvec = 3, uint32_t flags = 0) {
  if (is_mix(pl)) return false;  // a distribution plan has one family: the generic kernels on its target policy
  if (ey_large_needed(pl, nvec)) return true;
  if (!prior_normal(pl)) return false;  // the generic kernels or nothing (check_ready has refused what does not fit)
  if (flags & EY_FORCE_GENERIC) return false;
  if (EY_VBIT(4) && !pl->mfma32_ok) return true;
  return prefer_large(pl);
}
// the fused 16x16x4 kernels serve this plan (any batch size: their data image lives in global memory)
static bool use_fused16(const ey_plan* pl) {
  return pl->fused16_ok && prior_normal(pl) && !use_mfma32(pl) && !EY_VBIT(4);
}
const char* ey_plan_kernel(const ey_plan* pl) {
  if (!pl) return "generic";
  if (is_mix(pl)) return "dist";
  if (!prior_normal(pl)) return "generic";
  EyVariantScope vs(pl);
  if (use_mfma32(pl)) return "mfma32";
  if (use_fused16(pl)) return "fused16";
  return use_large(pl) ? "bgemm" : "generic";
}

// Asynchronous on `stream` (a sampler calls this once per minibatch, eeyore/samplers/serial_sampler.py:41-46): the
// plan's copies of the batch are written by device-to-device copies and two small kernels ordered on the stream; the
// buffers only grow, so the only synchronisation is the reallocation when a batch is larger than any before it.
int ey_plan_set_data(ey_plan* pl, const void* x, const void* y, int64_t N, void* stream) {
  if (!pl || !x || !y) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_data: null argument");
  if (is_mix(pl)) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_data: " + mix_noun(pl) + " takes no data (its tables are fixed at creation)");
  if (N < 1 || N > (1 << 24)) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_data: N out of range");
  hipStream_t s = (hipStream_t)stream;
  EY_HIP(hipSetDevice(pl->device));
  EyModel& m = pl->m;
  const size_t es = esize(pl);
  const int d0 = m.dims[0], dK = m.dims[m.nl];
  if (N > pl->cap_N) {
    EY_HIP(hipDeviceSynchronize());  // launches on any stream may still read the old buffers
    (void)hipFree(pl->d_x); (void)hipFree(pl->d_y); (void)hipFree(pl->d_labels);
    pl->d_x = pl->d_y = nullptr; pl->d_labels = nullptr;
    pl->cap_N = 0;
    EY_HIP(hipMalloc(&pl->d_x, es * N * d0));
    EY_HIP(hipMalloc(&pl->d_y, es * N * dK));
    EY_HIP(hipMalloc((void**)&pl->d_labels, sizeof(int) * N));
    pl->cap_N = N;
  }
  EY_HIP(hipMemcpyAsync(pl->d_x, x, es * N * d0, hipMemcpyDeviceToDevice, s));
  EY_HIP(hipMemcpyAsync(pl->d_y, y, es * N * dK, hipMemcpyDeviceToDevice, s));
  const dim3 grid((unsigned)((N + 255) / 256));
  if (ey_lik_regression(m.lik)) {}  // no kernel of a regression plan reads labels
  else if (es == 4) hipLaunchKernelGGL(k_labels<float>, grid, dim3(256), 0, s, (const float*)pl->d_y, pl->d_labels, N, dK);
  else hipLaunchKernelGGL(k_labels<double>, grid, dim3(256), 0, s, (const double*)pl->d_y, pl->d_labels, N, dK);
  EY_HIP(hipGetLastError());
  m.N = (int)N;
  ++pl->data_version;
  m.x = pl->d_x;
  m.y = pl->d_y;
  m.labels = pl->d_labels;
  pl->has_data = true;
  if (pl->mfma32_ok) {
    int rc = ey_mfma32_set_data(pl, s);
    if (rc) return rc;
  }
  if (pl->fused16_ok && (pl->mfma32_kind == 2 || !(pl->mfma32_ok && pl->mfma32_data_ok))) {  // kind 2: either may serve
    int rc = ey_fused16_set_data(pl, s);
    if (rc) return rc;
  }
  return EY_OK;
}

int ey_plan_set_prior(ey_plan* pl, const void* mu, const void* sigma, void* stream) {
  if (!pl || !mu || !sigma) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_prior: null argument");
  if (is_mix(pl)) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_prior: " + mix_noun(pl) + " has no prior (the density is the target)");
  hipStream_t s = (hipStream_t)stream;
  EY_HIP(hipSetDevice(pl->device));
  EyModel& m = pl->m;
  const size_t es = esize(pl);
  const int P = m.P;
  std::vector<unsigned char> hs(es * P), hm(es * P);
  EY_HIP(hipMemcpyAsync(hs.data(), sigma, es * P, hipMemcpyDeviceToHost, s));
  EY_HIP(hipMemcpyAsync(hm.data(), mu, es * P, hipMemcpyDeviceToHost, s));
  EY_HIP(hipStreamSynchronize(s));
  // Normal.log_prob = -(v-mu)^2/(2 sigma^2) - log(sigma) - log(sqrt(2 pi)); the theta-independent part is
  // summed once here (in double), the quadratic part is evaluated per call with 1/sigma^2.
  // Everything is validated before the plan is touched, as in ey_plan_set_prior_family: a refused call leaves the prior
  // it had (mu included: the kernels that read the prior per element read d_mu).
  double c = 0.0;
  std::vector<unsigned char> hiv(es * P);
  for (int i = 0; i < P; ++i) {
    const double sg = es == 4 ? (double)((const float*)hs.data())[i] : ((const double*)hs.data())[i];
    if (!(sg > 0.0)) EY_FAIL(EY_ERR_INVALID, "ey_plan_set_prior: sigma must be positive");
    c += -log(sg) - 0.91893853320467274178;
    if (es == 4) ((float*)hiv.data())[i] = 1.0f / ((float)sg * (float)sg);
    else ((double*)hiv.data())[i] = 1.0 / (sg * sg);
  }
  if (!pl->d_mu) EY_HIP(hipMalloc(&pl->d_mu, es * P));
  if (!pl->d_inv_var) EY_HIP(hipMalloc(&pl->d_inv_var, es * P));
  EY_HIP(hipMemcpy(pl->d_mu, hm.data(), es * P, hipMemcpyHostToDevice));  // the stream is idle: synchronised above
  EY_HIP(hipMemcpy(pl->d_inv_var, hiv.data(), es * P, hipMemcpyHostToDevice));
  // one (mu, sigma) for every parameter (the usual N(0, s) prior): the fused kernel then needs no per-element loads
  pl->prior_uniform = P > 0 && memcmp(hm.data(), hm.data() + es, es * (P - 1)) == 0 &&
                      memcmp(hiv.data(), hiv.data() + es, es * (P - 1)) == 0;
  pl->prior_mu0 = es == 4 ? (double)((const float*)hm.data())[0] : ((const double*)hm.data())[0];
  pl->prior_iv0 = es == 4 ? (double)((const float*)hiv.data())[0] : ((const double*)hiv.data())[0];
  m.mu = pl->d_mu;
  m.inv_var = pl->d_inv_var;
  m.prior_const = c;
  m.prior_h = nullptr;
  m.prior_kind = EY_PRIOR_NORMAL;
  pl->has_prior = true;
  return EY_OK;
}

int ey_plan_prior_family(const ey_plan* pl) { return pl ? pl->m.prior_kind : EY_PRIOR_NORMAL; }

double ey_plan_lik_scale(const ey_plan* pl) { return pl ? pl->lik_scale : 1.0; }

int ey_plan_set_lik_scale(ey_plan* pl, double s) {
  const char* who = "ey_plan_set_lik_scale";
  if (!pl) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null plan");
  if (is_mix(pl) || (pl->m.lik != EY_LIK_GAUSS_SUM && pl->m.lik != EY_LIK_LAPLACE_SUM))
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": only a plan of EY_LIK_GAUSS_SUM or EY_LIK_LAPLACE_SUM has a likelihood scale");
  if (!std::isfinite(s) || !(s > 0.0)) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": the scale must be finite and > 0");
  set_lik_constants(pl, s);  // kernel arguments of the launches that follow: nothing on the device changes
  return EY_OK;
}

int ey_plan_set_prior_family(ey_plan* pl, int family, const void* loc, const void* scale, const void* df, void* stream) {
  const char* who = "ey_plan_set_prior_family";
  if (family == EY_PRIOR_NORMAL) return ey_plan_set_prior(pl, loc, scale, stream);
  if (!pl || !loc || !scale) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  if (family != EY_PRIOR_LAPLACE && family != EY_PRIOR_STUDENT_T)
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": family must be EY_PRIOR_NORMAL, EY_PRIOR_LAPLACE or EY_PRIOR_STUDENT_T");
  const bool st = family == EY_PRIOR_STUDENT_T;
  if (st && !df) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": EY_PRIOR_STUDENT_T needs df");
  if (is_mix(pl)) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": " + mix_noun(pl) + " has no prior (the density is the target)");
  hipStream_t s = (hipStream_t)stream;
  EY_HIP(hipSetDevice(pl->device));
  EyModel& m = pl->m;
  const size_t es = esize(pl);
  const int P = m.P;
  std::vector<unsigned char> hl(es * P), hs(es * P), hd(st ? es * P : 0);
  EY_HIP(hipMemcpyAsync(hl.data(), loc, es * P, hipMemcpyDeviceToHost, s));
  EY_HIP(hipMemcpyAsync(hs.data(), scale, es * P, hipMemcpyDeviceToHost, s));
  if (st) EY_HIP(hipMemcpyAsync(hd.data(), df, es * P, hipMemcpyDeviceToHost, s));
  EY_HIP(hipStreamSynchronize(s));
  auto at = [&](const std::vector<unsigned char>& v, int i) {
    return es == 4 ? (double)((const float*)v.data())[i] : ((const double*)v.data())[i];
  };
  // The theta-independent part of the log-density is summed once here and the per-parameter tables are worked out in
  // double, then rounded once to the plan's dtype (as ey_plan_set_prior builds 1/sigma^2):
  //   Laplace.log_prob  = -log(2 b) - |v - loc| / b                                              table 1/b
  //   StudentT.log_prob = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 - log(s) - (nu+1)/2 log1p(((v-loc)/s)^2 / nu)
  //                                                                                 tables 1/(nu s^2), (nu+1)/2
  // Everything is validated before the plan is touched: a refused call leaves the prior it had.
  double c = 0.0;
  std::vector<double> t1(P), t2(st ? P : 0);
  for (int i = 0; i < P; ++i) {
    const double lo = at(hl, i), sc = at(hs, i);
    if (!std::isfinite(lo)) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": loc[" + std::to_string(i) + "] is not finite");
    if (!std::isfinite(sc) || !(sc > 0.0))
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": scale[" + std::to_string(i) + "] must be finite and > 0");
    if (!st) {
      c += -log(2.0 * sc);
      t1[i] = 1.0 / sc;
    } else {
      const double nu = at(hd, i);
      if (!std::isfinite(nu) || !(nu > 0.0))
        EY_FAIL(EY_ERR_INVALID, std::string(who) + ": df[" + std::to_string(i) + "] must be finite and > 0");
      c += lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.14159265358979323846) - log(sc);
      t1[i] = 1.0 / (nu * sc * sc);
      t2[i] = 0.5 * (nu + 1.0);
    }
  }
  EY_HIP(hipDeviceSynchronize());  // launches on any stream may still read the tables of the prior this one replaces
  if (!pl->d_mu) EY_HIP(hipMalloc(&pl->d_mu, es * P));
  if (!pl->d_inv_var) EY_HIP(hipMalloc(&pl->d_inv_var, es * P));
  if (st && !pl->d_prior_h) EY_HIP(hipMalloc(&pl->d_prior_h, es * P));
  std::vector<float> f32;
  auto upload = [&](void* dst, const std::vector<double>& src) -> hipError_t {
    if (es == 8) return hipMemcpy(dst, src.data(), es * P, hipMemcpyHostToDevice);
    f32.assign(src.begin(), src.end());
    return hipMemcpy(dst, f32.data(), es * P, hipMemcpyHostToDevice);
  };
  EY_HIP(hipMemcpy(pl->d_mu, hl.data(), es * P, hipMemcpyHostToDevice));
  EY_HIP(upload(pl->d_inv_var, t1));
  if (st) EY_HIP(upload(pl->d_prior_h, t2));
  pl->prior_uniform = false;  // read by the fused families only, which do not serve this plan
  m.mu = pl->d_mu;
  m.inv_var = pl->d_inv_var;
  m.prior_h = st ? pl->d_prior_h : nullptr;
  m.prior_const = c;
  m.prior_kind = family;
  pl->has_prior = true;
  return EY_OK;
}

extern "C" int ey_stats_update(const void* theta, const void* accepted, int64_t C, int64_t P, int dtype, void* s1,
                               void* s2, void* acc, void* stream);
static int moments_check(const ey_plan* pl, int64_t C, const char* who) {
  if (pl && pl->mom_s1 && pl->mom_C != C) {
    ey_set_error(std::string(who) + ": the attached moments were sized for " + std::to_string(pl->mom_C) +
                 " chains, called with " + std::to_string(C));
    return EY_ERR_INVALID;
  }
  return EY_OK;
}
// trailing pass for the kernel families that do not fuse the accumulation
static int moments_trailing(ey_plan* pl, int rc, const void* theta, const void* accepted, int64_t C, void* stream) {
  if (rc != EY_OK || !pl->mom_s1) return rc;
  return ey_stats_update(theta, accepted, C, pl->m.P, pl->dtype, pl->mom_s1, pl->mom_s2, pl->mom_acc, stream);
}

// The window of the attached dual averaging that a launch of n_iters HMC iterations covers (nothing once the table is
// used up); `advance` moves the plan's position in the table past it.
static EyDA da_window(ey_plan* pl, int n_iters) {
  EyDA w;
  if (!pl->da_state) return w;
  w.step = pl->da_step;  // the attached step vector stays the step of every launch until it is detached
  if (pl->da_done >= pl->da_n) return w;  // the table is used up: nothing adapts any more
  w.state = pl->da_state;
  w.table = pl->da_table + 3 * pl->da_done;
  w.n = (int)std::min<int64_t>(n_iters, pl->da_n - pl->da_done);
  w.final_it = (pl->da_final_avg && pl->da_done + n_iters >= pl->da_n) ? (int)(pl->da_n - 1 - pl->da_done) : -1;
  w.d = pl->da_d;
  w.logeub = pl->da_logeub;
  w.has_eub = pl->da_has_eub ? 1 : 0;
  return w;
}
static int da_check(const ey_plan* pl, int64_t C, bool fused, const char* who) {
  if (!pl->da_state) return EY_OK;
  if (pl->da_C != C)
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": the attached dual averaging was sized for " + std::to_string(pl->da_C) +
                            " chains, called with " + std::to_string(C));
  if (!fused && pl->da_done < pl->da_n)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": in-kernel dual averaging needs one of the fused kernel families "
                                                   "(mfma32, fused16); detach it and adapt on the host for this plan");
  return EY_OK;
}

// A prior family other than Normal lives in the generic kernels alone: a model whose LDS image they cannot hold (nvec state
// vectors, as use_large counts them) has no kernel.
static int prior_fits(const ey_plan* pl, int nvec, const char* who) {
  if (prior_normal(pl) || is_mix(pl) || !ey_large_needed(pl, nvec)) return EY_OK;
  EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": a " + prior_name(pl) + " prior is served only for models the generic "
                              "kernels can hold in the 160 KiB LDS of a CU; this model needs the layerwise kernels, "
                              "which have a Normal prior only");
}
static int check_ready(const ey_plan* pl, int64_t C, const char* who, int nvec = 2) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null plan");
  if (!pl->has_data) EY_FAIL(EY_ERR_STATE, std::string(who) + ": ey_plan_set_data has not been called");
  if (!pl->has_prior) EY_FAIL(EY_ERR_STATE, std::string(who) + ": ey_plan_set_prior has not been called");
  if (int rcp = prior_fits(pl, nvec, who)) return rcp;
  if (C < 0 || C > 0x7fffffffLL) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": chain count out of range");
  return C == 0 ? 1 : EY_OK;  // 1 = nothing to do (an empty chain batch has null buffers)
}

int ey_log_target(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* log_lik, void* log_prior,
                  void* stream) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_log_target: null plan");
  EyVariantScope vs(pl);
  // log_prior alone (bayesian_model.py:46-50) needs no data: with no rows attached the likelihood sum is empty
  if (!log_lik && !pl->has_data && pl->has_prior) {
    if (!theta) EY_FAIL(EY_ERR_INVALID, "ey_log_target: null theta");
    if (C <= 0) return EY_OK;
    if (int rcp = prior_fits(pl, 3, "ey_log_target")) return rcp;
    EY_HIP(hipSetDevice(pl->device));
    return ey_generic_log_target(pl, theta, temp, C, nullptr, log_prior, nullptr, nullptr, (hipStream_t)stream);
  }
  int rc = check_ready(pl, C, "ey_log_target", 3);
  if (rc) return rc < 0 ? rc : EY_OK;
  if (!theta) EY_FAIL(EY_ERR_INVALID, "ey_log_target: null theta");
  if (C == 0) return EY_OK;
  EY_HIP(hipSetDevice(pl->device));
  if (use_fused16(pl)) return ey_fused16_log_target(pl, theta, temp, C, log_lik, log_prior, nullptr, nullptr, (hipStream_t)stream);
  if (use_large(pl)) return ey_large_log_target(pl, theta, temp, C, log_lik, log_prior, nullptr, nullptr, (hipStream_t)stream);
  return ey_generic_log_target(pl, theta, temp, C, log_lik, log_prior, nullptr, nullptr, (hipStream_t)stream);
}

int ey_log_lik_rows(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* rows, void* stream) {
  if (pl && is_mix(pl)) EY_FAIL(EY_ERR_UNSUPPORTED, "ey_log_lik_rows: " + mix_noun(pl) + " has no data rows");
  int rc = check_ready(pl, C, "ey_log_lik_rows", 3);
  if (rc) return rc < 0 ? rc : EY_OK;
  EyVariantScope vs(pl);
  if (!theta || !rows) EY_FAIL(EY_ERR_INVALID, "ey_log_lik_rows: null argument");
  if (C == 0) return EY_OK;
  EY_HIP(hipSetDevice(pl->device));
  if (use_large(pl)) return ey_large_log_lik_rows(pl, theta, temp, C, rows, (hipStream_t)stream);
  return ey_generic_log_lik_rows(pl, theta, temp, C, rows, (hipStream_t)stream);
}

int ey_forward(ey_plan* pl, const void* theta, int64_t C, void* out, void* stream) {
  if (pl && is_mix(pl)) EY_FAIL(EY_ERR_INVALID, "ey_forward: " + mix_noun(pl) + " has no network");
  // (not check_ready: a prior family the layerwise kernels do not serve is no obstacle, their forward products read no prior)
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_forward: null plan");
  if (!pl->has_data) EY_FAIL(EY_ERR_STATE, "ey_forward: ey_plan_set_data has not been called");
  if (!pl->has_prior) EY_FAIL(EY_ERR_STATE, "ey_forward: ey_plan_set_prior has not been called");
  if (C < 0 || C > 0x7fffffffLL) EY_FAIL(EY_ERR_INVALID, "ey_forward: chain count out of range");
  if (C == 0) return EY_OK;
  EyVariantScope vs(pl);
  if (!theta || !out) EY_FAIL(EY_ERR_INVALID, "ey_forward: null argument");
  EY_HIP(hipSetDevice(pl->device));
  // whatever family serves the plan's draws: the generic value kernel when its LDS image (two state vectors) holds the
  // model, the layerwise forward products otherwise; the fused families have no such output
  if (ey_large_needed(pl, 2)) return ey_large_forward(pl, theta, C, out, (hipStream_t)stream);
  return ey_generic_forward(pl, theta, C, out, (hipStream_t)stream);
}

int ey_log_target_grad(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* target, void* grad,
                       void* stream) {
  int rc = check_ready(pl, C, "ey_log_target_grad", 3);
  if (rc) return rc < 0 ? rc : EY_OK;
  EyVariantScope vs(pl);
  if (!theta || !target || !grad) EY_FAIL(EY_ERR_INVALID, "ey_log_target_grad: null argument");
  if (C == 0) return EY_OK;
  EY_HIP(hipSetDevice(pl->device));
  if (use_mfma32(pl)) return ey_mfma32_log_target_grad(pl, theta, temp, C, target, grad, (hipStream_t)stream);
  if (use_fused16(pl)) return ey_fused16_log_target(pl, theta, temp, C, nullptr, nullptr, target, grad, (hipStream_t)stream);
  if (use_large(pl)) return ey_large_log_target(pl, theta, temp, C, nullptr, nullptr, target, grad, (hipStream_t)stream);
  return ey_generic_log_target(pl, theta, temp, C, nullptr, nullptr, target, grad, (hipStream_t)stream);
}

__global__ void k_count_accepts(const unsigned char* __restrict__ accepted, int* __restrict__ count, int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C && accepted[c]) count[c] += 1;
}

int ey_hmc_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                    int64_t C, void* target, void* grad, void* stream) {
  int rc = check_ready(pl, C, "ey_hmc_leapfrog", 3);
  if (rc) return rc < 0 ? rc : EY_OK;
  EyVariantScope vs(pl);
  if (!theta || !p || !target || !grad) EY_FAIL(EY_ERR_INVALID, "ey_hmc_leapfrog: null argument");
  if (L < 1) EY_FAIL(EY_ERR_INVALID, "ey_hmc_leapfrog: num_steps must be >= 1");
  if (C == 0) return EY_OK;
  EY_HIP(hipSetDevice(pl->device));
  if (use_mfma32(pl)) return ey_mfma32_leapfrog(pl, theta, p, step, step_vec, L, temp, C, target, grad, (hipStream_t)stream);
  if (use_fused16(pl)) return ey_fused16_leapfrog(pl, theta, p, step, step_vec, L, temp, C, target, grad, (hipStream_t)stream);
  if (use_large(pl)) return ey_large_leapfrog(pl, theta, p, step, step_vec, L, temp, C, target, grad, (hipStream_t)stream);
  return ey_generic_leapfrog(pl, theta, p, step, step_vec, L, temp, C, target, grad, (hipStream_t)stream);
}

// the kernel families that do not fuse attached moments replay them from the per-iteration records of a *_run call
static int moments_replay_check(const ey_plan* pl, const EyRun* run, const char* who) {
  if (pl->mom_s1 && run && run->n_iters > 1 && (!run->samples || !run->accepted))
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": attached moments with n_iters > 1 need the samples and accepted "
                                                   "records on this kernel family");
  return EY_OK;
}
static int moments_replay(ey_plan* pl, const EyRun* run, const void* theta, const void* accepted, int64_t C,
                          const char* who, void* stream) {
  if (!pl->mom_s1) return EY_OK;
  if (!run || run->n_iters == 1) return ey_stats_update(theta, accepted, C, pl->m.P, pl->dtype, pl->mom_s1, pl->mom_s2,
                                                        pl->mom_acc, stream);
  int rcc = moments_replay_check(pl, run, who);
  if (rcc) return rcc;
  return ey_stats_update_run(run->samples, run->accepted, run->n_iters, C, pl->m.P, pl->dtype, pl->mom_s1, pl->mom_s2,
                             pl->mom_acc, stream);
}

// copy the state after one iteration of a host-looped run into the per-iteration records
static int record_iteration(ey_plan* pl, const EyRun* run, int it, const void* theta, const void* target,
                            const void* accepted, int64_t C, hipStream_t s) {
  const size_t es = esize(pl);
  if (run->samples)
    EY_HIP(hipMemcpyAsync((char*)run->samples + (size_t)it * C * pl->m.P * es, theta, (size_t)C * pl->m.P * es,
                          hipMemcpyDeviceToDevice, s));
  if (run->targets)
    EY_HIP(hipMemcpyAsync((char*)run->targets + (size_t)it * C * es, target, (size_t)C * es, hipMemcpyDeviceToDevice, s));
  if (run->accepted)
    EY_HIP(hipMemcpyAsync((char*)run->accepted + (size_t)it * C, accepted, (size_t)C, hipMemcpyDeviceToDevice, s));
  if (run->accept_count)
    hipLaunchKernelGGL(k_count_accepts, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s,
                       (const unsigned char*)accepted, run->accept_count, C);
  return EY_OK;
}

}  // extern "C": the frame below holds templates

// ---- the sampler entry points.  Each is its *_impl with the ABI's arguments packed, and every *_impl
// runs in one frame:  begin()  ->  the sampler's own argument checks  ->  ready()  ->  the launch  ->  finish().
#define EY_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)
struct EyCall {
  ey_plan* pl;
  const EyDraw& d;
  const char* who;
  std::optional<EyVariantScope> vs;

  // the plan can serve the batch (nvec: the state vectors its generic kernel keeps in LDS), under the plan's variant;
  // 1 = an empty batch, which is answered OK before any buffer is looked at (done())
  int begin(int nvec = 2) {
    const int rc = check_ready(pl, d.C, who, nvec);
    if (rc == EY_OK) vs.emplace(pl);
    return rc;
  }
  // the attached moments fit the call -- replayed: on a family that replays them from the records, which must then
  // exist (before the launch: a failure leaves the chains alone) -- and the plan's device is current
  int ready(bool replayed) {
    EY_TRY(moments_check(pl, d.C, who));
    if (replayed) EY_TRY(moments_replay_check(pl, d.run, who));
    EY_HIP(hipSetDevice(pl->device));
    return EY_OK;
  }
  // the moments of a family that does not fuse them, from the state (one draw) or the records (a run) the launch left
  int finish(int rc, const void* theta) {
    return rc ? rc : moments_replay(pl, d.run, theta, d.accepted, d.C, who, d.s);
  }
  int refuse(const char* what) const { EY_FAIL(EY_ERR_INVALID, std::string(who) + ": " + what); }
  int n_iters() const { return d.run && d.run->n_iters < 1 ? refuse("n_iters must be >= 1") : EY_OK; }
  int step(double step, const void* step_vec) const {
    return !(step > 0.0) && !step_vec ? refuse("step must be positive") : EY_OK;
  }
  int factors(int64_t G, const void* tril_index) const {
    if (G < 1) return refuse("the number of factors G must be >= 1");
    return !tril_index && G != 1 && G != d.C ? refuse("without tril_index, G must be 1 or the number of chains") : EY_OK;
  }
};
static int done(int rc) { return rc < 0 ? rc : EY_OK; }

// the kernel family that serves a draw of this plan (nvec as in use_large)
enum EyFamily { FAM_MFMA32, FAM_FUSED16, FAM_GENERIC, FAM_LARGE };
static EyFamily family_of(const ey_plan* pl, int nvec, uint32_t flags) {
  if (use_mfma32(pl) && !(flags & EY_FORCE_GENERIC)) return FAM_MFMA32;
  if (use_fused16(pl) && !(flags & EY_FORCE_GENERIC)) return FAM_FUSED16;
  return use_large(pl, nvec, flags) ? FAM_LARGE : FAM_GENERIC;
}
static bool replays_moments(EyFamily f) { return f == FAM_FUSED16 || f == FAM_GENERIC; }  // mfma32 fuses, large trails

// Models beyond LDS: the layerwise path has no in-kernel iteration loop.  launch(one) queues one iteration; its records
// and the trailing moments pass follow it on the stream, iteration by iteration.
template <typename F>
static int large_loop(ey_plan* pl, const EyDraw& d, const void* theta, const void* target, F launch) {
  EyDraw one = d;
  one.run = nullptr;
  for (int it = 0, n = d.run ? d.run->n_iters : 1; it < n; ++it) {
    one.iter = d.iter + it;
    EY_TRY(launch(one));
    if (d.run) EY_TRY(record_iteration(pl, d.run, it, theta, target, d.accepted, d.C, d.s));
    EY_TRY(moments_trailing(pl, EY_OK, theta, d.accepted, d.C, d.s));
  }
  EY_HIP(hipGetLastError());
  return EY_OK;
}

static int hmc_impl(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                    const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin(3)) return done(rc);
  if (!theta || !target || !grad || !d.accepted) return f.refuse("null argument");
  if (L < 1) return f.refuse("num_steps must be >= 1");
  EY_TRY(f.n_iters());
  const EyFamily fam = family_of(pl, 3, d.flags);
  // the dual averaging is checked between the moments and their records, as it always was: ready() stops before
  // the records
  EY_TRY(f.ready(false));
  EY_TRY(da_check(pl, d.C, fam == FAM_MFMA32 || fam == FAM_FUSED16, who));
  if (replays_moments(fam)) EY_TRY(moments_replay_check(pl, d.run, who));
  const EyDA da = da_window(pl, d.run ? d.run->n_iters : 1);
  if (da.step) step_vec = da.step;  // every kernel family: the attached step vector is the step
  if (fam == FAM_LARGE)
    return large_loop(pl, d, theta, target, [&](const EyDraw& one) {
      return ey_large_hmc(pl, theta, target, grad, p0, u, step, step_vec, L, one, rate, hcur, hprop);
    });
  if (fam == FAM_GENERIC)
    return f.finish(ey_generic_hmc(pl, theta, target, grad, p0, u, step, step_vec, L, d, rate, hcur, hprop), theta);
  const int rc = (fam == FAM_MFMA32 ? ey_mfma32_hmc : ey_fused16_hmc)(pl, theta, target, grad, p0, u, step, step_vec, L, d,
                                                                     rate, hcur, hprop, &da);
  if (rc == EY_OK && da.state) pl->da_done += da.n;  // the table advances only past iterations that were launched
  return fam == FAM_MFMA32 ? rc : f.finish(rc, theta);  // mfma32 accumulates attached moments itself
}

static int mala_impl(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                     const void* step_vec, const EyDraw& d, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin(4)) return done(rc);  // k_mala carves four state vectors from LDS
  if (!theta || !target || !grad || !d.accepted) return f.refuse("null argument");
  EY_TRY(f.step(step, step_vec));
  EY_TRY(f.n_iters());
  const EyFamily fam = family_of(pl, 4, d.flags);
  EY_TRY(f.ready(replays_moments(fam)));
  if (fam == FAM_MFMA32) return ey_mfma32_mala(pl, theta, target, grad, z, u, step, step_vec, d);
  if (fam == FAM_LARGE)
    return large_loop(pl, d, theta, target, [&](const EyDraw& one) {
      return ey_large_mala_mh(pl, theta, target, grad, z, u, step, step_vec, nullptr, one);
    });
  return f.finish((fam == FAM_FUSED16 ? ey_fused16_mala : ey_generic_mala)(pl, theta, target, grad, z, u, step, step_vec, d),
                  theta);
}

static int mh_impl(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
                   const EyDraw& d, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !scale || !d.accepted) return f.refuse("null argument");
  EY_TRY(f.n_iters());
  const EyFamily fam = family_of(pl, 2, d.flags);
  EY_TRY(f.ready(replays_moments(fam)));
  if (fam == FAM_MFMA32) return ey_mfma32_mh(pl, theta, target, z, u, scale, d);
  if (fam == FAM_LARGE)
    return large_loop(pl, d, theta, target, [&](const EyDraw& one) {
      return ey_large_mala_mh(pl, theta, target, nullptr, z, u, 0.0, nullptr, scale, one);
    });
  return f.finish((fam == FAM_FUSED16 ? ey_fused16_mh : ey_generic_mh)(pl, theta, target, z, u, scale, d), theta);
}

// RAM, MH and MALA with a fixed factor, and AM run on their own kernels of ey_generic.hip for every model, whatever
// plan.kernel says: the fused families have nowhere to keep a factor, let alone adapt one
static int ram_impl(ey_plan* pl, void* theta, void* target, void* chol, const void* z, const void* u, double a, double g,
                    uint64_t n, const EyDraw& d, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !chol || !d.accepted) return f.refuse("null argument");
  EY_TRY(f.n_iters());
  if (n == 0) return f.refuse("the adaptation index n must be >= 1");
  if (!(a > 0.0 && a < 1.0)) return f.refuse("the target acceptance a must lie in (0, 1)");
  if (!std::isfinite(g)) return f.refuse("the decay exponent g must be finite");
  EY_TRY(f.ready(true));
  return f.finish(ey_generic_ram(pl, theta, target, chol, z, u, a, g, n, d), theta);
}

static int mh_tril_impl(ey_plan* pl, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                        const void* z, const void* u, const EyDraw& d, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !tril || !d.accepted) return f.refuse("null argument");
  EY_TRY(f.n_iters());
  EY_TRY(f.factors(G, tril_index));
  EY_TRY(f.ready(true));
  return f.finish(ey_generic_mh_tril(pl, theta, target, tril, G, tril_index, z, u, d), theta);
}

static int mala_tril_impl(ey_plan* pl, void* theta, void* target, void* grad, const void* tril, int64_t G,
                          const void* tril_index, const void* z, const void* u, double step, const void* step_vec,
                          const EyDraw& d, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !grad || !tril || !d.accepted) return f.refuse("null argument");
  EY_TRY(f.step(step, step_vec));
  EY_TRY(f.n_iters());
  EY_TRY(f.factors(G, tril_index));
  EY_TRY(f.ready(true));
  return f.finish(ey_generic_mala_tril(pl, theta, target, grad, tril, G, tril_index, z, u, step, step_vec, d), theta);
}

// EY_HMC_METRIC_FUSED (include/eeyore_amd_hmc_metric_fused.h): what a call with the bit is refused for, after every refusal
// of a call without it and before ready().  `fused` says whether the call runs on k_hmc_metric_mfma.
static int hmc_metric_fused(EyCall& f, const ey_plan* pl, int form, uint32_t flags, const char* who, bool& fused) {
  fused = (flags & EY_HMC_METRIC_FUSED) != 0;
  if (!fused) return EY_OK;
  if (form != EY_METRIC_DIAG) return f.refuse("EY_HMC_METRIC_FUSED: diagonal metric only (form EY_METRIC_DIAG)");
  if (flags & EY_FORCE_GENERIC) return f.refuse("EY_HMC_METRIC_FUSED and EY_FORCE_GENERIC contradict each other");
  if (is_mix(pl) || !use_mfma32(pl))
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": EY_HMC_METRIC_FUSED serves the plans of the mfma32 family with the "
                                "batch they hold; this plan's kernel (ey_plan_kernel) is \"" + ey_plan_kernel(pl) + "\"");
  return EY_OK;
}

// HMC with a fixed metric: one kernel of ey_generic.hip for every model, as the samplers with a factor above -- and, with
// EY_HMC_METRIC_FUSED, k_hmc_metric_mfma for the plans of the mfma32 family.  An attached
// dual averaging is refused, not ignored: this kernel does not consume the table, and hmc_impl's callers rely on it.
static int hmc_metric_impl(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                           const void* metric_index, const void* v0, const void* u, double step, const void* step_vec,
                           int L, const EyDraw& d, void* rate, void* hcur, void* hprop, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !grad || !metric || !d.accepted) return f.refuse("null argument");
  if (form != EY_METRIC_DIAG && form != EY_METRIC_TRIL)
    return f.refuse("form must be EY_METRIC_DIAG or EY_METRIC_TRIL");
  if (L < 1) return f.refuse("num_steps must be >= 1");
  EY_TRY(f.step(step, step_vec));
  EY_TRY(f.n_iters());
  EY_TRY(f.factors(G, metric_index));
  if (pl->da_state)
    return f.refuse("a dual-averaging table is attached (ey_plan_attach_da), which HMC with a metric does not consume; "
                    "detach it and adapt on the host");
  bool fused;
  EY_TRY(hmc_metric_fused(f, pl, form, d.flags, who, fused));
  EY_TRY(f.ready(true));
  if (fused)
    return f.finish(ey_hmc_metric_mfma_launch(pl, theta, target, grad, metric, G, metric_index, v0, u, step,
                                              const_cast<void*>(step_vec), L, d, rate, hcur, hprop, EyWarm{}), theta);
  return f.finish(ey_generic_hmc_metric(pl, theta, target, grad, metric, form, G, metric_index, v0, u, step, step_vec, L,
                                        d, rate, hcur, hprop), theta);
}

// NUTS under a metric (include/eeyore_amd_nuts.h): hmc_metric_impl's frame and refusals on k_nuts (ey_nuts.hip), then those
// of the depth cap, the uniform table and the two warm-up epilogues (ey_hmc_metric_warmup's): all of them before ready(), so
// a refused call has launched and written nothing.
static int nuts_impl(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                     const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                     void* da_state, const void* da_table, int da_n, double da_d, double log_eub, int final_avg, void* mean,
                     void* M2, int64_t count, void* steps_rec, void* rate_rec, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !grad || !metric || !d.accepted) return f.refuse("null argument");
  if (form != EY_METRIC_DIAG && form != EY_METRIC_TRIL)
    return f.refuse("form must be EY_METRIC_DIAG or EY_METRIC_TRIL");
  if (nu.max_depth < 1 || nu.max_depth > EY_NUTS_MAX_DEPTH)
    return f.refuse("max_depth must lie in [1, 10] (EY_NUTS_MAX_DEPTH)");
  if (nu.u && nu.S < 1 + 2 * EY_NUTS_MAX_DEPTH + ((int64_t)1 << nu.max_depth))
    return f.refuse("the uniform table u [C, S] needs S >= 21 + 2^max_depth words");
  EY_TRY(f.step(step, step_vec));
  EY_TRY(f.n_iters());
  EY_TRY(f.factors(G, metric_index));
  if (pl->da_state)
    return f.refuse("a dual-averaging table is attached (ey_plan_attach_da), which NUTS does not consume; detach it and "
                    "adapt on the host, or pass the dual averaging as arguments of ey_nuts_warmup");
  const int n_iters = d.run ? d.run->n_iters : 1;
  if (da_state && !da_table) return f.refuse("a dual-averaging state (da_state) needs its table (da_table)");
  if (da_state && !step_vec) return f.refuse("a dual-averaging state (da_state) needs step_vec, the steps it adapts");
  if (da_state && (da_n < 1 || da_n > n_iters)) return f.refuse("da_n must lie in [1, n_iters]");
  if (da_state && !std::isfinite(da_d)) return f.refuse("the target acceptance d must be finite");
  if (!mean != !M2) return f.refuse("mean and M2 go together: exactly one of them is null");
  if (mean && count < 0) return f.refuse("count must be >= 0");
  // the tree in device memory (include/eeyore_amd_nuts_tree.h): an undersized workspace would be stores out of bounds
  // EY_NUTS_FUSED (include/eeyore_amd_nuts_fused.h): the same workspace, the draw on k_nuts_mfma
  const bool fused = (d.flags & EY_NUTS_FUSED) != 0;
  if (fused) {
    if (form != EY_METRIC_DIAG) return f.refuse("EY_NUTS_FUSED serves the diagonal metric only (form EY_METRIC_DIAG)");
    if (d.flags & EY_FORCE_GENERIC) return f.refuse("EY_NUTS_FUSED and EY_FORCE_GENERIC contradict each other");
  }
  const bool tree_ws = fused || (d.flags & EY_NUTS_TREE_DEVICE) != 0;
  if (tree_ws) {
    if (form != EY_METRIC_DIAG)
      return f.refuse("EY_NUTS_TREE_DEVICE serves the diagonal metric only (form EY_METRIC_DIAG)");
    if (!pl->nuts_tree)
      return f.refuse("EY_NUTS_TREE_DEVICE needs a workspace for the tree (ey_plan_attach_nuts_tree)");
    const int64_t need = ey_nuts_ws_bytes(pl, d.C, nu.max_depth);
    if (pl->nuts_tree_bytes < need)
      return f.refuse(("the attached workspace of " + std::to_string(pl->nuts_tree_bytes) + " bytes is smaller than the " +
                       std::to_string(need) + " bytes the tree of this call needs (ey_nuts_tree_bytes)").c_str());
  }
  if (fused && !use_mfma32(pl))
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": EY_NUTS_FUSED serves the plans of the mfma32 family with the batch "
                                "they hold; this plan's kernel (ey_plan_kernel) is \"" + ey_plan_kernel(pl) + "\"");
  EY_TRY(f.ready(true));
  EyWarm w;
  w.da_state = (double*)da_state;
  w.da_table = (const double*)da_table;
  w.da_n = da_state ? da_n : 0;
  w.final_it = da_state && final_avg ? da_n - 1 : -1;
  w.d = da_d;
  w.has_eub = log_eub == log_eub ? 1 : 0;  // NaN: no upper bound (ey_plan_attach_da)
  w.logeub = w.has_eub ? log_eub : 0.0;
  w.mean = (double*)mean;
  w.M2 = (double*)M2;
  w.count = count;
  w.steps_rec = steps_rec;
  w.rate_rec = rate_rec;
  if (fused)
    return f.finish(ey_nuts_mfma_launch(pl, theta, target, grad, metric, G, metric_index, step, step_vec, d, nu, w), theta);
  if (tree_ws)
    return f.finish(ey_nuts_ws_launch(pl, theta, target, grad, metric, G, metric_index, step, step_vec, d, nu, w), theta);
  return f.finish(ey_nuts_launch(pl, theta, target, grad, metric, form, G, metric_index, step, step_vec, d, nu, w), theta);
}

// Elliptical slice sampling (include/eeyore_amd_eslice.h): one kernel of ey_eslice.hip on the generic evaluation for every
// model, as the samplers above -- and, for the plans the mfma32 family serves, its fused form on the matrix cores
// (ey_eslice_mfma.hip) unless the call asks for the generic kernels.  Every refusal is the same on both and
// fires before the choice.  What is refused about the base, before anything else is looked at:
static int eslice_base(const ey_plan* pl, const void* base_loc, const void* base_scale, const char* who) {
  if (!base_loc != !base_scale)
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": base_loc and base_scale go together: exactly one of them is null");
  if (!base_loc && is_mix(pl))
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": " + mix_noun(pl) + " has no prior to slice under; give the Gaussian base "
                                               "(base_loc, base_scale)");
  if (!base_loc && !prior_normal(pl))
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": without a base the plan's prior must be Normal (it is " + prior_name(pl) +
                                               "); give the Gaussian base (base_loc, base_scale)");
  return EY_OK;
}

// the fused form serves the call (under the plan's variant scope: use_mfma32 reads it)
static bool eslice_fused(const ey_plan* pl, uint32_t flags) { return use_mfma32(pl) && !(flags & EY_FORCE_GENERIC); }

static int eslice_impl(ey_plan* pl, void* theta, void* target, const EyEslice& es, const EyDraw& d, const char* who) {
  EyCall f{pl, d, who};
  if (int rc = f.begin(4)) return done(rc);  // k_eslice carves four state vectors from LDS
  if (!theta || !target || !es.ell || !d.accepted) return f.refuse("null argument");
  EY_TRY(eslice_base(pl, es.base_loc, es.base_scale, who));
  if (es.max_shrinks < 1 || es.max_shrinks > EY_ESLICE_MAX_SHRINKS)
    return f.refuse("max_shrinks must lie in [1, 64] (EY_ESLICE_MAX_SHRINKS)");
  if (es.u && es.S < 2 + (int64_t)es.max_shrinks)
    return f.refuse("the uniform table u [C, S] needs S >= 2 + max_shrinks words");
  EY_TRY(f.n_iters());
  if (pl->da_state)
    return f.refuse("a dual-averaging table is attached (ey_plan_attach_da), which elliptical slice sampling does not "
                    "consume (it has no step); detach it");
  EY_TRY(f.ready(true));
  // (the generic kernel's LDS limit, checked in ey_eslice_launch, cannot bind on a plan of the mfma32 family: P <= 1315;
  // the fused kernel's tile and LDS limits are those use_mfma32 has enforced.  Moments are replayed from the records.)
  if (eslice_fused(pl, d.flags)) return f.finish(ey_eslice_mfma_launch(pl, theta, target, es, d), theta);
  return f.finish(ey_eslice_launch(pl, theta, target, es, d), theta);
}

static int am_impl(ey_plan* pl, void* theta, void* target, const EyAm& am, const EyDraw& d, const char* who,
                   int transform) {
  EyCall f{pl, d, who};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !am.mean || !am.cov_sum || !am.cov || !am.num_accepted || !am.cov0 || !d.accepted ||
      !am.breakdowns)
    return f.refuse("null argument");
  EY_TRY(f.n_iters());
  if (am.t0 < 2) return f.refuse("t0 must be >= 2 (the covariance divides by n - 1)");
  if (!(am.l >= 0.0 && am.l <= 1.0)) return f.refuse("the mixture weight l must lie in [0, 1]");
  if (!std::isfinite(am.b) || !std::isfinite(am.c)) return f.refuse("b and c must be finite");
  if (transform == EY_AM_SOFTABS) {  // am.eps carries a
    if (!(std::isfinite(am.eps) && am.eps > 0.0)) return f.refuse("a must be finite and > 0");
  } else if (!(std::isfinite(am.eps) && am.eps >= 0.0)) {
    return f.refuse("eps must be finite and >= 0");
  }
  if (am.idx < 0 || am.idx + 1 - am.offset < 1)
    return f.refuse("idx must be >= 0 and the adaptation index idx + 1 - offset >= 1");
  EY_TRY(f.ready(true));
  return f.finish(ey_generic_am(pl, theta, target, am, d, transform), theta);
}
// the state and the settings of the four AM entry points (eps: the ridge, or softabs's a)
static EyAm make_am(void* running_mean, void* cov_sum, void* cov, void* num_accepted, const void* cov0, int cov0_per_chain,
                    double l, double b, double c, double eps, int64_t t0, int64_t idx, int64_t offset, void* breakdowns,
                    const void* z = nullptr, const void* u_mix = nullptr, const void* u = nullptr, void* branch = nullptr) {
  return {running_mean, cov_sum, cov, (int*)num_accepted, cov0, cov0_per_chain, l, b, c, eps, t0, idx, offset,
          z, u_mix, u, (unsigned char*)branch, (int*)breakdowns};
}

extern "C" {

int ey_hmc_step(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                const void* step_vec, int L, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                uint64_t chain_offset, uint32_t flags, void* accepted, void* accept_rate, void* H_cur, void* H_prop,
                void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, nullptr};
  return hmc_impl(pl, theta, target, grad, p0, u, step, step_vec, L, d, accept_rate, H_cur, H_prop, "ey_hmc_step");
}

int ey_hmc_run(ey_plan* pl, void* theta, void* target, void* grad, double step, const void* step_vec, int L,
               const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
               int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted,
               void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return hmc_impl(pl, theta, target, grad, nullptr, nullptr, step, step_vec, L, d, nullptr, nullptr, nullptr, "ey_hmc_run");
}

int ey_mala_step(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                 const void* step_vec, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                 uint64_t chain_offset, uint32_t flags, void* accepted, void* log_rate, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return mala_impl(pl, theta, target, grad, z, u, step, step_vec, d, "ey_mala_step");
}

int ey_mala_run(ey_plan* pl, void* theta, void* target, void* grad, double step, const void* step_vec, const void* temp,
                int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters,
                void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return mala_impl(pl, theta, target, grad, nullptr, nullptr, step, step_vec, d, "ey_mala_run");
}

int ey_mh_step(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
               const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
               void* accepted, void* log_rate, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return mh_impl(pl, theta, target, z, u, scale, d, "ey_mh_step");
}

int ey_mh_run(ey_plan* pl, void* theta, void* target, const void* scale, const void* temp, int64_t C, uint64_t seed,
              uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples, void* targets,
              void* accepted_rec, void* accept_count, void* accepted, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return mh_impl(pl, theta, target, nullptr, nullptr, scale, d, "ey_mh_run");
}

int ey_ram_step(ey_plan* pl, void* theta, void* target, void* chol, const void* z, const void* u, double a, double g,
                uint64_t n, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                uint32_t flags, void* accepted, void* log_rate, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return ram_impl(pl, theta, target, chol, z, u, a, g, n, d, "ey_ram_step");
}

int ey_ram_run(ey_plan* pl, void* theta, void* target, void* chol, double a, double g, uint64_t n, const void* temp,
               int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters,
               void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return ram_impl(pl, theta, target, chol, nullptr, nullptr, a, g, n, d, "ey_ram_run");
}

int ey_mh_tril_step(ey_plan* pl, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                    const void* z, const void* u, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                    uint64_t chain_offset, uint32_t flags, void* accepted, void* log_rate, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return mh_tril_impl(pl, theta, target, tril, G, tril_index, z, u, d, "ey_mh_tril_step");
}

int ey_mh_tril_run(ey_plan* pl, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                   const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                   int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count, void* accepted,
                   void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return mh_tril_impl(pl, theta, target, tril, G, tril_index, nullptr, nullptr, d, "ey_mh_tril_run");
}

int ey_mala_tril_step(ey_plan* pl, void* theta, void* target, void* grad, const void* tril, int64_t G,
                      const void* tril_index, const void* z, const void* u, double step, const void* step_vec,
                      const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                      void* accepted, void* log_rate, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return mala_tril_impl(pl, theta, target, grad, tril, G, tril_index, z, u, step, step_vec, d, "ey_mala_tril_step");
}

int ey_mala_tril_run(ey_plan* pl, void* theta, void* target, void* grad, const void* tril, int64_t G,
                     const void* tril_index, double step, const void* step_vec, const void* temp, int64_t C, uint64_t seed,
                     uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples, void* targets,
                     void* accepted_rec, void* accept_count, void* accepted, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return mala_tril_impl(pl, theta, target, grad, tril, G, tril_index, nullptr, nullptr, step, step_vec, d,
                        "ey_mala_tril_run");
}

// (declared in include/eeyore_amd_ext.h)
int ey_hmc_metric_step(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                       const void* metric_index, const void* v0, const void* u, double step, const void* step_vec, int L,
                       const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                       void* accepted, void* accept_rate, void* H_cur, void* H_prop, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, nullptr};
  return hmc_metric_impl(pl, theta, target, grad, metric, form, G, metric_index, v0, u, step, step_vec, L, d, accept_rate,
                         H_cur, H_prop, "ey_hmc_metric_step");
}

int ey_hmc_metric_run(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                      const void* metric_index, double step, const void* step_vec, int L, const void* temp, int64_t C,
                      uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                      void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return hmc_metric_impl(pl, theta, target, grad, metric, form, G, metric_index, nullptr, nullptr, step, step_vec, L, d,
                         nullptr, nullptr, nullptr, "ey_hmc_metric_run");
}

// (declared in include/eeyore_amd_warmup.h)  ey_hmc_metric_run's frame and refusals, then those of the two epilogues: all of
// them before ready(), so a refused call has touched nothing.
int ey_hmc_metric_warmup(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                         const void* metric_index, double step, void* step_vec, int L, const void* temp, int64_t C,
                         uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                         void* targets, void* accepted_rec, void* accept_count, void* accepted, void* da_state,
                         const void* da_table, int da_n, double d, double log_eub, int final_avg, void* mean, void* M2,
                         int64_t count, void* steps_rec, void* rate_rec, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw dr = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  EyCall f{pl, dr, "ey_hmc_metric_warmup"};
  if (int rc = f.begin()) return done(rc);
  if (!theta || !target || !grad || !metric || !accepted) return f.refuse("null argument");
  if (form != EY_METRIC_DIAG && form != EY_METRIC_TRIL)
    return f.refuse("form must be EY_METRIC_DIAG or EY_METRIC_TRIL");
  if (L < 1) return f.refuse("num_steps must be >= 1");
  EY_TRY(f.step(step, step_vec));
  EY_TRY(f.n_iters());
  EY_TRY(f.factors(G, metric_index));
  if (pl->da_state)
    return f.refuse("a dual-averaging table is attached (ey_plan_attach_da), which HMC with a metric does not consume; "
                    "detach it and pass the dual averaging as arguments of this call");
  if (da_state && !da_table) return f.refuse("a dual-averaging state (da_state) needs its table (da_table)");
  if (da_state && !step_vec) return f.refuse("a dual-averaging state (da_state) needs step_vec, the steps it adapts");
  if (da_state && (da_n < 1 || da_n > n_iters)) return f.refuse("da_n must lie in [1, n_iters]");
  if (da_state && !std::isfinite(d)) return f.refuse("the target acceptance d must be finite");
  if (!mean != !M2) return f.refuse("mean and M2 go together: exactly one of them is null");
  if (mean && count < 0) return f.refuse("count must be >= 0");
  bool fused;
  EY_TRY(hmc_metric_fused(f, pl, form, flags, "ey_hmc_metric_warmup", fused));
  EY_TRY(f.ready(true));
  EyWarm w;
  w.da_state = (double*)da_state;
  w.da_table = (const double*)da_table;
  w.da_n = da_state ? da_n : 0;
  w.final_it = da_state && final_avg ? da_n - 1 : -1;
  w.d = d;
  w.has_eub = log_eub == log_eub ? 1 : 0;  // NaN: no upper bound (ey_plan_attach_da)
  w.logeub = w.has_eub ? log_eub : 0.0;
  w.mean = (double*)mean;
  w.M2 = (double*)M2;
  w.count = count;
  w.steps_rec = steps_rec;
  w.rate_rec = rate_rec;
  if (fused)
    return f.finish(ey_hmc_metric_mfma_launch(pl, theta, target, grad, metric, G, metric_index, nullptr, nullptr, step,
                                              step_vec, L, dr, nullptr, nullptr, nullptr, w), theta);
  return f.finish(ey_generic_hmc_metric_warmup(pl, theta, target, grad, metric, form, G, metric_index, step, step_vec, L,
                                               dr, w), theta);
}

// (declared in include/eeyore_amd_nuts.h)  accept_stat travels as the draw's log_rate: record_draw writes it
int ey_nuts_step(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                 const void* metric_index, const void* v0, const void* u, int64_t S, double step, const void* step_vec,
                 int max_depth, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                 uint32_t flags, void* accepted, void* depth, void* n_leapfrog, void* divergent, void* accept_stat,
                 void* energy, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, accept_stat, (hipStream_t)stream, nullptr};
  const EyNuts nu = {v0, u, S, max_depth, (int*)depth, (int*)n_leapfrog, (unsigned char*)divergent, energy, nullptr, nullptr};
  return nuts_impl(pl, theta, target, grad, metric, form, G, metric_index, step, const_cast<void*>(step_vec), d, nu, nullptr,
                   nullptr, 0, 0.0, 0.0, 0, nullptr, nullptr, 0, nullptr, nullptr, "ey_nuts_step");
}

int ey_nuts_run(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                const void* metric_index, double step, const void* step_vec, int max_depth, const void* temp, int64_t C,
                uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                void* targets, void* accepted_rec, void* accept_count, void* accepted, void* depth, void* n_leapfrog,
                void* divergent, void* accept_stat, void* energy, void* depth_rec, void* divergent_rec, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, accept_stat, (hipStream_t)stream, &run};
  const EyNuts nu = {nullptr, nullptr, 0, max_depth, (int*)depth, (int*)n_leapfrog, (unsigned char*)divergent, energy,
                     (int*)depth_rec, (unsigned char*)divergent_rec};
  return nuts_impl(pl, theta, target, grad, metric, form, G, metric_index, step, const_cast<void*>(step_vec), d, nu, nullptr,
                   nullptr, 0, 0.0, 0.0, 0, nullptr, nullptr, 0, nullptr, nullptr, "ey_nuts_run");
}

int ey_nuts_warmup(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                   const void* metric_index, double step, void* step_vec, int max_depth, const void* temp, int64_t C,
                   uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                   void* targets, void* accepted_rec, void* accept_count, void* accepted, void* depth, void* n_leapfrog,
                   void* divergent, void* accept_stat, void* energy, void* depth_rec, void* divergent_rec, void* da_state,
                   const void* da_table, int da_n, double d, double log_eub, int final_avg, void* mean, void* M2,
                   int64_t count, void* steps_rec, void* rate_rec, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw dr = {temp, C, seed, iter, chain_offset, flags, accepted, accept_stat, (hipStream_t)stream, &run};
  const EyNuts nu = {nullptr, nullptr, 0, max_depth, (int*)depth, (int*)n_leapfrog, (unsigned char*)divergent, energy,
                     (int*)depth_rec, (unsigned char*)divergent_rec};
  return nuts_impl(pl, theta, target, grad, metric, form, G, metric_index, step, step_vec, dr, nu, da_state, da_table, da_n,
                   d, log_eub, final_avg, mean, M2, count, steps_rec, rate_rec, "ey_nuts_warmup");
}

// (declared in include/eeyore_amd_nuts_fused.h)
const char* ey_nuts_kernel(const ey_plan* pl, uint32_t flags) {
  if (!pl || is_mix(pl)) return "generic";
  EyVariantScope vs(pl);
  return (flags & EY_NUTS_FUSED) && !(flags & EY_FORCE_GENERIC) && use_mfma32(pl) ? "mfma32" : "generic";
}

// (declared in include/eeyore_amd_hmc_metric_fused.h)
const char* ey_hmc_metric_kernel(const ey_plan* pl, uint32_t flags) {
  if (!pl || is_mix(pl)) return "generic";
  EyVariantScope vs(pl);
  return (flags & EY_HMC_METRIC_FUSED) && !(flags & EY_FORCE_GENERIC) && use_mfma32(pl) ? "mfma32" : "generic";
}

// (declared in include/eeyore_amd_eslice.h)
int ey_eslice_ell(ey_plan* pl, const void* theta, const void* base_loc, const void* base_scale, const void* temp, int64_t C,
                  void* ell, void* target, void* stream) {
  int rc = check_ready(pl, C, "ey_eslice_ell", 4);
  if (rc) return rc < 0 ? rc : EY_OK;
  EyVariantScope vs(pl);
  if (!theta) EY_FAIL(EY_ERR_INVALID, "ey_eslice_ell: null argument");
  if ((rc = eslice_base(pl, base_loc, base_scale, "ey_eslice_ell"))) return rc;
  EY_HIP(hipSetDevice(pl->device));
  // no flags here: the plan alone decides, so a carried ell comes from the kernel a plain step compares it in
  if (eslice_fused(pl, 0)) return ey_eslice_mfma_ell_launch(pl, theta, base_loc, base_scale, temp, C, ell, target, (hipStream_t)stream);
  return ey_eslice_ell_launch(pl, theta, base_loc, base_scale, temp, C, ell, target, (hipStream_t)stream);
}

// (declared in include/eeyore_amd_eslice_fused.h)
const char* ey_eslice_kernel(const ey_plan* pl, uint32_t flags) {
  if (!pl || is_mix(pl)) return "generic";
  EyVariantScope vs(pl);
  return eslice_fused(pl, flags) ? "mfma32" : "generic";
}

int ey_eslice_step(ey_plan* pl, void* theta, void* target, void* ell, const void* base_loc, const void* base_scale,
                   const void* z, const void* u, int64_t S, int max_shrinks, const void* temp, int64_t C, uint64_t seed,
                   uint64_t iter, uint64_t chain_offset, uint32_t flags, void* accepted, void* n_evals, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, nullptr};
  const EyEslice es = {base_loc, base_scale, z, u, S, max_shrinks, ell, (int*)n_evals, nullptr};
  return eslice_impl(pl, theta, target, es, d, "ey_eslice_step");
}

int ey_eslice_run(ey_plan* pl, void* theta, void* target, void* ell, const void* base_loc, const void* base_scale,
                  int max_shrinks, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                  uint32_t flags, int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count,
                  void* accepted, void* n_evals, void* n_evals_rec, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  const EyEslice es = {base_loc, base_scale, nullptr, nullptr, 0, max_shrinks, ell, (int*)n_evals, (int*)n_evals_rec};
  return eslice_impl(pl, theta, target, es, d, "ey_eslice_run");
}

int ey_am_step(ey_plan* pl, void* theta, void* target, void* running_mean, void* cov_sum, void* cov, void* num_accepted,
               const void* cov0, int cov0_per_chain, double l, double b, double c, double eps, int64_t t0, int64_t idx,
               int64_t offset, const void* z, const void* u_mix, const void* u, const void* temp, int64_t C,
               uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, void* accepted, void* log_rate,
               void* branch, void* breakdowns, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return am_impl(pl, theta, target, make_am(running_mean, cov_sum, cov, num_accepted, cov0, cov0_per_chain, l, b, c, eps, t0,
                                            idx, offset, breakdowns, z, u_mix, u, branch), d, "ey_am_step", EY_AM_RIDGE);
}

int ey_am_run(ey_plan* pl, void* theta, void* target, void* running_mean, void* cov_sum, void* cov, void* num_accepted,
              const void* cov0, int cov0_per_chain, double l, double b, double c, double eps, int64_t t0, int64_t idx,
              int64_t offset, const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset,
              uint32_t flags, int n_iters, void* samples, void* targets, void* accepted_rec, void* accept_count,
              void* accepted, void* breakdowns, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return am_impl(pl, theta, target, make_am(running_mean, cov_sum, cov, num_accepted, cov0, cov0_per_chain, l, b, c, eps, t0,
                                            idx, offset, breakdowns), d, "ey_am_run", EY_AM_RIDGE);
}

// AM with the transform softabs(cov, a) in place of the ridge: k_am's softabs instantiation
int ey_am_softabs_step(ey_plan* pl, void* theta, void* target, void* running_mean, void* cov_sum, void* cov,
                       void* num_accepted, const void* cov0, int cov0_per_chain, double l, double b, double c, double a,
                       int64_t t0, int64_t idx, int64_t offset, const void* z, const void* u_mix, const void* u,
                       const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                       void* accepted, void* log_rate, void* branch, void* breakdowns, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return am_impl(pl, theta, target, make_am(running_mean, cov_sum, cov, num_accepted, cov0, cov0_per_chain, l, b, c, a, t0,
                                            idx, offset, breakdowns, z, u_mix, u, branch), d, "ey_am_softabs_step",
                 EY_AM_SOFTABS);
}

int ey_am_softabs_run(ey_plan* pl, void* theta, void* target, void* running_mean, void* cov_sum, void* cov,
                      void* num_accepted, const void* cov0, int cov0_per_chain, double l, double b, double c, double a,
                      int64_t t0, int64_t idx, int64_t offset, const void* temp, int64_t C, uint64_t seed, uint64_t iter,
                      uint64_t chain_offset, uint32_t flags, int n_iters, void* samples, void* targets, void* accepted_rec,
                      void* accept_count, void* accepted, void* breakdowns, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return am_impl(pl, theta, target, make_am(running_mean, cov_sum, cov, num_accepted, cov0, cov0_per_chain, l, b, c, a, t0,
                                            idx, offset, breakdowns), d, "ey_am_softabs_run", EY_AM_SOFTABS);
}

int ey_am_softabs_fits(const ey_plan* pl) { return pl && ey_generic_am_softabs_fits(pl) ? 1 : 0; }

int ey_softabs(const void* A, int64_t B, int64_t P, int dtype, double a, void* out, void* sweeps, void* stream) {
  if (!A || !out) EY_FAIL(EY_ERR_INVALID, "ey_softabs: null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_softabs: bad dtype");
  if (B < 0 || B > 0x7fffffffLL || P < 1) EY_FAIL(EY_ERR_INVALID, "ey_softabs: B or P out of range");
  if (!(std::isfinite(a) && a > 0.0)) EY_FAIL(EY_ERR_INVALID, "ey_softabs: a must be finite and > 0");
  if (P > 128)
    EY_FAIL(EY_ERR_UNSUPPORTED, "ey_softabs: P = " + std::to_string(P) + " exceeds the limit of 128 (the f64 work matrix "
                                "of one wave lives in LDS)");
  if (B == 0) return EY_OK;
  return ey_generic_softabs(A, B, (int)P, dtype, a, out, sweeps, (hipStream_t)stream);
}

// ---- Gibbs: blockwise random-walk Metropolis on k_gibbs (ey_generic.hip) for every model, whatever plan.kernel says
int ey_gibbs_table_create(ey_gibbs_table** out, int64_t P, int S, const int32_t* blk_off, const int32_t* blk_idx,
                          const double* blk_scale, int dtype, int device_id) {
  const char* who = "ey_gibbs_table_create";
  if (!out) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  *out = nullptr;
  if (!blk_off || !blk_idx || !blk_scale) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": bad dtype");
  if (P < 1 || P > 0x7fffffffLL) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": P out of range");
  if (S < 1) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": a table needs at least one block (S >= 1)");
  if (blk_off[0] != 0) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": blk_off[0] must be 0");
  std::vector<char> seen((size_t)P, 0);
  for (int s = 0; s < S; ++s) {
    if (blk_off[s + 1] <= blk_off[s])
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": block " + std::to_string(s) + " is empty (blk_off must increase)");
    if ((int64_t)blk_off[s + 1] > P)  // disjoint blocks of [0, P) hold at most P indices: nothing beyond is read
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": the blocks hold more than P indices, so they overlap");
    if (!(blk_scale[s] > 0.0) || !std::isfinite(blk_scale[s]))
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": the scale of block " + std::to_string(s) +
                                  " must be a positive finite number");
    for (int j = blk_off[s]; j < blk_off[s + 1]; ++j) {
      const int i = blk_idx[j];
      if (i < 0 || i >= P)
        EY_FAIL(EY_ERR_INVALID, std::string(who) + ": index " + std::to_string(i) + " of block " + std::to_string(s) +
                                    " is outside [0, " + std::to_string(P) + ")");
      if (seen[i])
        EY_FAIL(EY_ERR_INVALID, std::string(who) + ": parameter " + std::to_string(i) + " is in two blocks (block " +
                                    std::to_string(s) + " is the second)");
      seen[i] = 1;
    }
  }
  EY_HIP(hipSetDevice(device_id));
  ey_gibbs_table* tb = new ey_gibbs_table();
  tb->P = P; tb->S = S; tb->n_idx = blk_off[S]; tb->dtype = dtype; tb->device = device_id;
  tb->d_off = tb->d_idx = nullptr; tb->d_scale = nullptr;
  const size_t esz = dtype == EY_F32 ? 4 : 8;
  std::vector<float> sf(blk_scale, blk_scale + S);
  hipError_t e = hipMalloc((void**)&tb->d_off, sizeof(int) * (S + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&tb->d_idx, sizeof(int) * tb->n_idx);
  if (e == hipSuccess) e = hipMalloc(&tb->d_scale, esz * S);
  if (e == hipSuccess) e = hipMemcpy(tb->d_off, blk_off, sizeof(int) * (S + 1), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(tb->d_idx, blk_idx, sizeof(int) * tb->n_idx, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(tb->d_scale, dtype == EY_F32 ? (const void*)sf.data() : (const void*)blk_scale, esz * S,
                  hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    ey_gibbs_table_destroy(tb);
    EY_FAIL(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  *out = tb;
  return EY_OK;
}

int ey_gibbs_table_destroy(ey_gibbs_table* tb) {
  if (!tb) return EY_OK;
  if (tb->d_off) (void)hipFree(tb->d_off);
  if (tb->d_idx) (void)hipFree(tb->d_idx);
  if (tb->d_scale) (void)hipFree(tb->d_scale);
  delete tb;
  return EY_OK;
}

// Not in the frame of the other samplers (EyCall), because its order is its own: a mixture plan is refused first, the table
// and its LDS image are checked before an empty batch is answered and the buffers after it, and the kernel itself adds the
// accepted fractions to the attached acc, so that the moments are replayed without accept flags.
static int gibbs_impl(ey_plan* pl, const ey_gibbs_table* tb, void* theta, void* target, const void* z, const void* u,
                      const EyDraw& d, const char* who) {
  const EyRun* run = d.run;
  if (pl && is_mix(pl))
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": Gibbs blocks are the nodes of an MLP; " + mix_noun(pl) + " has none");
  int rc = check_ready(pl, d.C, who);
  if (rc < 0) return rc;
  if (!tb) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null block table");
  if (tb->P != pl->m.P || tb->dtype != pl->dtype || tb->device != pl->device)
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": the block table was built for another model size, dtype or device");
  if (run && run->n_iters < 1) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": n_iters must be >= 1");
  if (ey_generic_gibbs_lds(pl, tb) > 160 * 1024)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": the model's evaluation image and the block table do not fit the "
                                                   "160 KiB LDS of a CU");
  if (rc) return EY_OK;  // C == 0
  EyVariantScope vs(pl);
  if (!theta || !target || !d.accepted) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  if ((rc = moments_check(pl, d.C, who))) return rc;
  if (pl->mom_s1 && run && run->n_iters > 1 && !run->samples)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": attached moments with n_iters > 1 need the samples record");
  EY_HIP(hipSetDevice(pl->device));
  rc = ey_generic_gibbs(pl, tb, theta, target, z, u, d, pl->mom_s1 ? pl->mom_acc : nullptr);
  if (rc || !pl->mom_s1) return rc;
  // s1, s2 from the state(s) the draws left; the kernel has added the accepted fractions to acc
  if (!run || run->n_iters == 1)
    return ey_stats_update(theta, nullptr, d.C, pl->m.P, pl->dtype, pl->mom_s1, pl->mom_s2, nullptr, d.s);
  return ey_stats_update_run(run->samples, nullptr, run->n_iters, d.C, pl->m.P, pl->dtype, pl->mom_s1, pl->mom_s2, nullptr,
                             d.s);
}

int ey_gibbs_step(ey_plan* pl, const ey_gibbs_table* tb, void* theta, void* target, const void* z, const void* u,
                  const void* temp, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags,
                  void* accepted, void* log_rate, void* stream) {
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, log_rate, (hipStream_t)stream, nullptr};
  return gibbs_impl(pl, tb, theta, target, z, u, d, "ey_gibbs_step");
}

int ey_gibbs_run(ey_plan* pl, const ey_gibbs_table* tb, void* theta, void* target, const void* temp, int64_t C,
                 uint64_t seed, uint64_t iter, uint64_t chain_offset, uint32_t flags, int n_iters, void* samples,
                 void* targets, void* accepted_rec, void* accept_count, void* accepted, void* stream) {
  const EyRun run = {n_iters, samples, targets, accepted_rec, (int*)accept_count};
  const EyDraw d = {temp, C, seed, iter, chain_offset, flags, accepted, nullptr, (hipStream_t)stream, &run};
  return gibbs_impl(pl, tb, theta, target, nullptr, nullptr, d, "ey_gibbs_run");
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------- small kernels
template <typename T>
__global__ void k_pt_swap(const T* ell_i, const T* ell_j, const T* t_i, const T* t_j, const T* dlogq, const T* u,
                          int64_t C, unsigned char* swap, T* log_rate) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  T lr;
  swap[c] = ey_pt_decide<T>(ell_i[c], ell_j[c], t_i[c], t_j[c], dlogq ? dlogq + c : nullptr, u[c], &lr) ? 1 : 0;
  if (log_rate) log_rate[c] = lr;
}

template <typename T>
__global__ void k_philox_normal(T* out, int64_t C, int64_t P, uint64_t seed, uint64_t iter, uint64_t chain_offset) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t nb = (P + 3) / 4;  // blocks of four stream elements per chain
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < C * nb; k += stride) {
    const int64_t c = k / nb, b = k - c * nb;
    const EyRng r = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    T o[4];
    ey_rng_normal4<T>(r, (uint32_t)b, o);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * b + j < P) out[c * P + 4 * b + j] = o[j];
  }
}

template <typename T>
__global__ void k_philox_uniform(T* out, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const EyRng r = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
  out[c] = ey_rng_uniform<T>(r);
}

template <typename T>
__global__ void k_philox_uniform_blocks(T* out, int64_t C, int64_t S, uint64_t seed, uint64_t iter, uint64_t chain_offset) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < C * S; k += stride) {
    const int64_t c = k / S, s = k - c * S;
    const EyRng r = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    out[k] = ey_rng_uniform_at<T>(r, (uint32_t)s);
  }
}

extern "C" {

int ey_philox_uniform_blocks(void* out, int64_t C, int64_t S, uint64_t seed, uint64_t iter, uint64_t chain_offset,
                             int dtype, void* stream) {
  if (!out) EY_FAIL(EY_ERR_INVALID, "ey_philox_uniform_blocks: null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_philox_uniform_blocks: bad dtype");
  if (C <= 0 || S <= 0) return EY_OK;
  const int64_t nblk = (C * S + 255) / 256;
  const dim3 grid((unsigned)(nblk < 65536 ? nblk : 65536));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EY_F32)
    hipLaunchKernelGGL(k_philox_uniform_blocks<float>, grid, dim3(256), 0, s, (float*)out, C, S, seed, iter, chain_offset);
  else
    hipLaunchKernelGGL(k_philox_uniform_blocks<double>, grid, dim3(256), 0, s, (double*)out, C, S, seed, iter,
                       chain_offset);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

int ey_pt_swap_decide(const void* ell_i, const void* ell_j, const void* t_i, const void* t_j, const void* dlogq,
                      const void* u, int64_t C, int dtype, void* swap, void* log_rate, void* stream) {
  if (!ell_i || !ell_j || !t_i || !t_j || !u || !swap) EY_FAIL(EY_ERR_INVALID, "ey_pt_swap_decide: null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_pt_swap_decide: bad dtype");
  if (C <= 0) return EY_OK;
  const unsigned nb = (unsigned)((C + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EY_F32)
    hipLaunchKernelGGL(k_pt_swap<float>, dim3(nb), dim3(256), 0, s, (const float*)ell_i, (const float*)ell_j,
                       (const float*)t_i, (const float*)t_j, (const float*)dlogq, (const float*)u, C,
                       (unsigned char*)swap, (float*)log_rate);
  else
    hipLaunchKernelGGL(k_pt_swap<double>, dim3(nb), dim3(256), 0, s, (const double*)ell_i, (const double*)ell_j,
                       (const double*)t_i, (const double*)t_j, (const double*)dlogq, (const double*)u, C,
                       (unsigned char*)swap, (double*)log_rate);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

int ey_philox_normal(void* out, int64_t C, int64_t P, uint64_t seed, uint64_t iter, uint64_t chain_offset, int dtype,
                     void* stream) {
  if (!out) EY_FAIL(EY_ERR_INVALID, "ey_philox_normal: null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_philox_normal: bad dtype");
  if (C <= 0 || P <= 0) return EY_OK;
  const int64_t nblk = (C * P + 255) / 256;
  const dim3 grid((unsigned)(nblk < 65536 ? nblk : 65536));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EY_F32)
    hipLaunchKernelGGL(k_philox_normal<float>, grid, dim3(256), 0, s, (float*)out, C, P, seed, iter, chain_offset);
  else
    hipLaunchKernelGGL(k_philox_normal<double>, grid, dim3(256), 0, s, (double*)out, C, P, seed, iter, chain_offset);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

int ey_philox_block(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  if (!counter || !key || !out) EY_FAIL(EY_ERR_INVALID, "ey_philox_block: null argument");
  ey_philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
  return EY_OK;
}

int ey_philox_uniform(void* out, int64_t C, uint64_t seed, uint64_t iter, uint64_t chain_offset, int dtype,
                      void* stream) {
  if (!out) EY_FAIL(EY_ERR_INVALID, "ey_philox_uniform: null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_philox_uniform: bad dtype");
  if (C <= 0) return EY_OK;
  const unsigned nb = (unsigned)((C + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EY_F32)
    hipLaunchKernelGGL(k_philox_uniform<float>, dim3(nb), dim3(256), 0, s, (float*)out, C, seed, iter, chain_offset);
  else
    hipLaunchKernelGGL(k_philox_uniform<double>, dim3(nb), dim3(256), 0, s, (double*)out, C, seed, iter, chain_offset);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------- chain moments
// Running per-chain sums for ChainLists.mean / multi_rhat-style summaries (eeyore/chains/chain_lists.py:65-66,
// eeyore/stats/multi_rhat.py): s1 += theta, s2 += theta^2 in double, acc += accepted; one streaming pass.
template <typename T>
__global__ void k_stats_update(const T* __restrict__ theta, double* __restrict__ s1, double* __restrict__ s2,
                               int64_t n4, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int64_t b = 4 * i;
    if (b + 3 < n && sizeof(T) == 4) {
      const float4 t = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(theta) + b);
      double2* p1 = reinterpret_cast<double2*>(s1 + b);
      double2* p2 = reinterpret_cast<double2*>(s2 + b);
      double2 a0 = p1[0], a1 = p1[1], q0 = p2[0], q1 = p2[1];
      a0.x += t.x; a0.y += t.y; a1.x += t.z; a1.y += t.w;
      q0.x += (double)t.x * t.x; q0.y += (double)t.y * t.y; q1.x += (double)t.z * t.z; q1.y += (double)t.w * t.w;
      p1[0] = a0; p1[1] = a1; p2[0] = q0; p2[1] = q1;
    } else {
      for (int64_t k = b; k < n && k < b + 4; ++k) {
        const double t = (double)theta[k];
        s1[k] += t;
        s2[k] += t * t;
      }
    }
  }
}

__global__ void k_acc_update(const unsigned char* __restrict__ accepted, double* __restrict__ acc, int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) acc[c] += (double)accepted[c];
}

// The same sums over the n_it recorded iterations of a launch in ONE pass: every element's accumulators are read once,
// take the element's n_it states in iteration order (the additions ey_stats_update would make launch after launch, or the
// step kernel draw after draw: the same bits) and are written once -- the record buffer streams through (4 bytes per
// state) instead of the f64 accumulators being read and written once per iteration (32 bytes per state).
template <typename T>
__global__ void k_stats_update_run(const T* __restrict__ samples, int n_it, double* __restrict__ s1, double* __restrict__ s2,
                                   int64_t n4, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int64_t b = 4 * i;
    if (b + 3 < n && sizeof(T) == 4 && (n & 3) == 0) {
      double2* p1 = reinterpret_cast<double2*>(s1 + b);
      double2* p2 = reinterpret_cast<double2*>(s2 + b);
      double2 a0 = p1[0], a1 = p1[1], q0 = p2[0], q1 = p2[1];
      const float* src = reinterpret_cast<const float*>(samples) + b;
      int it = 0;
      for (; it + 4 <= n_it; it += 4) {  // four iterations' loads in flight
        float4 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = *reinterpret_cast<const float4*>(src + (int64_t)(it + k) * n);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          a0.x += t[k].x; a0.y += t[k].y; a1.x += t[k].z; a1.y += t[k].w;
          q0.x += (double)t[k].x * t[k].x; q0.y += (double)t[k].y * t[k].y;
          q1.x += (double)t[k].z * t[k].z; q1.y += (double)t[k].w * t[k].w;
        }
      }
      for (; it < n_it; ++it) {
        const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)it * n);
        a0.x += t.x; a0.y += t.y; a1.x += t.z; a1.y += t.w;
        q0.x += (double)t.x * t.x; q0.y += (double)t.y * t.y; q1.x += (double)t.z * t.z; q1.y += (double)t.w * t.w;
      }
      p1[0] = a0; p1[1] = a1; p2[0] = q0; p2[1] = q1;
    } else {
      for (int64_t k = b; k < n && k < b + 4; ++k) {
        double a = s1[k], q = s2[k];
        for (int it = 0; it < n_it; ++it) {
          const double t = (double)samples[(int64_t)it * n + k];
          a += t;
          q += t * t;
        }
        s1[k] = a;
        s2[k] = q;
      }
    }
  }
}
__global__ void k_acc_update_run(const unsigned char* __restrict__ accepted, int n_it, double* __restrict__ acc, int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = acc[c];
  for (int it = 0; it < n_it; ++it) a += (double)accepted[(int64_t)it * C + c];
  acc[c] = a;
}
int ey_stats_update_run(const void* samples, const void* accepted_rec, int n_it, int64_t C, int64_t P, int dtype, void* s1,
                        void* s2, void* acc, void* stream) {
  if (!samples || !s1 || !s2) EY_FAIL(EY_ERR_INVALID, "ey_stats_update_run: null argument");
  if (C <= 0 || P <= 0 || n_it <= 0) return EY_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = C * P, n4 = (n + 3) / 4;
  const unsigned nb = (unsigned)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  if (dtype == EY_F32)
    hipLaunchKernelGGL(k_stats_update_run<float>, dim3(nb), dim3(256), 0, s, (const float*)samples, n_it, (double*)s1,
                       (double*)s2, n4, n);
  else
    hipLaunchKernelGGL(k_stats_update_run<double>, dim3(nb), dim3(256), 0, s, (const double*)samples, n_it, (double*)s1,
                       (double*)s2, n4, n);
  if (accepted_rec && acc)
    hipLaunchKernelGGL(k_acc_update_run, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s,
                       (const unsigned char*)accepted_rec, n_it, (double*)acc, C);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

extern "C" int ey_stats_update(const void* theta, const void* accepted, int64_t C, int64_t P, int dtype, void* s1,
                               void* s2, void* acc, void* stream) {
  if (!theta || !s1 || !s2) EY_FAIL(EY_ERR_INVALID, "ey_stats_update: null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_stats_update: bad dtype");
  if (C <= 0 || P <= 0) return EY_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = C * P, n4 = (n + 3) / 4;
  const unsigned nb = (unsigned)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
  if (dtype == EY_F32)
    hipLaunchKernelGGL(k_stats_update<float>, dim3(nb), dim3(256), 0, s, (const float*)theta, (double*)s1, (double*)s2,
                       n4, n);
  else
    hipLaunchKernelGGL(k_stats_update<double>, dim3(nb), dim3(256), 0, s, (const double*)theta, (double*)s1,
                       (double*)s2, n4, n);
  if (accepted && acc)
    hipLaunchKernelGGL(k_acc_update, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s,
                       (const unsigned char*)accepted, (double*)acc, C);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

extern "C" int ey_plan_attach_da(ey_plan* pl, void* state, void* step_vec, const void* table, int64_t n, int64_t C,
                                 double d, double log_eub, int final_avg) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_da: null plan");
  if (!state) {
    pl->da_state = nullptr; pl->da_step = nullptr; pl->da_table = nullptr;
    pl->da_n = pl->da_done = pl->da_C = 0;
    return EY_OK;
  }
  if (is_mix(pl))
    EY_FAIL(EY_ERR_UNSUPPORTED, "ey_plan_attach_da: in-kernel dual averaging needs one of the fused kernel families; "
                                "adapt on the host for " + mix_noun(pl));
  if (!step_vec || !table || n <= 0 || C <= 0)
    EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_da: state, step_vec, table, n > 0 and C > 0 are required");
  if (!(d > 0.0 && d < 1.0)) EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_da: the target acceptance must lie in (0, 1)");
  pl->da_state = (double*)state;
  pl->da_step = step_vec;
  pl->da_table = (const double*)table;
  pl->da_n = n;
  pl->da_done = 0;
  pl->da_C = C;
  pl->da_d = d;
  pl->da_has_eub = log_eub == log_eub;  // NaN = no upper bound
  pl->da_logeub = pl->da_has_eub ? log_eub : 0.0;
  pl->da_final_avg = final_avg != 0;
  return EY_OK;
}

// (declared in include/eeyore_amd_nuts_tree.h)
extern "C" int64_t ey_nuts_tree_bytes(const ey_plan* pl, int64_t C, int max_depth) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_nuts_tree_bytes: null plan");
  if (C < 0) EY_FAIL(EY_ERR_INVALID, "ey_nuts_tree_bytes: C must be >= 0");
  if (max_depth < 1 || max_depth > EY_NUTS_MAX_DEPTH)
    EY_FAIL(EY_ERR_INVALID, "ey_nuts_tree_bytes: max_depth must lie in [1, 10] (EY_NUTS_MAX_DEPTH)");
  return ey_nuts_ws_bytes(pl, C, max_depth);
}

extern "C" int ey_plan_attach_nuts_tree(ey_plan* pl, void* ws, int64_t bytes) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_nuts_tree: null plan");
  if (!ws) {
    pl->nuts_tree = nullptr;
    pl->nuts_tree_bytes = 0;
    return EY_OK;
  }
  if (bytes <= 0) EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_nuts_tree: a workspace needs bytes > 0");
  if ((uintptr_t)ws % (pl->dtype == EY_F32 ? 4 : 8))
    EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_nuts_tree: the workspace must be aligned to the plan's dtype");
  pl->nuts_tree = ws;
  pl->nuts_tree_bytes = bytes;
  return EY_OK;
}

extern "C" int ey_plan_attach_moments(ey_plan* pl, void* s1, void* s2, void* acc, int64_t C) {
  if (!pl) EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_moments: null plan");
  if (!s1) {
    pl->mom_s1 = pl->mom_s2 = pl->mom_acc = nullptr;
    pl->mom_C = 0;
    return EY_OK;
  }
  if (!s2 || !acc || C <= 0) EY_FAIL(EY_ERR_INVALID, "ey_plan_attach_moments: s1, s2, acc and C > 0 are required");
  pl->mom_s1 = (double*)s1;
  pl->mom_s2 = (double*)s2;
  pl->mom_acc = (double*)acc;
  pl->mom_C = C;
  return EY_OK;
}
