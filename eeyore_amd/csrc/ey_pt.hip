// The between-chain move of a tempering ladder in one launch (PowerPosteriorSampler.between_chain_moves,
// eeyore/samplers/power_posterior_sampler.py:128-172): k_pt_between and the ladder object it reads.  DESIGN.md 4.13.
#include <cmath>
#include <vector>

#include "ey_common.h"

#define PT_WAVES 4     // replicas (waves) per workgroup
#define PT_KMAX 1024   // temperatures: PT_WAVES * PT_KMAX tempered targets of the widest dtype are 32 KiB of LDS

struct ey_pt_ladder {
  int K, dtype, device;
  void* d_t;      // [K] of dtype: the temperatures
  void* d_logq;   // [K,K] of dtype: log of the row-normalised partner probabilities (diagonal 0)
  double* d_cdf;  // [K,K]: running sums of row i's normalised probabilities in index order, the diagonal adding nothing
};

// Where a lane sends a store it must not make (a row element beyond P, an output only lane 0 publishes): its own 8 bytes,
// which nobody reads -- no memory operation behind a per-lane branch (g_f16_junk of ey_fused16.hip).
static __device__ double g_pt_junk[64];
template <typename U>
__device__ __forceinline__ U* pt_junk(int lane) { return reinterpret_cast<U*>(g_pt_junk + lane); }

template <typename T>
struct PtArgs {
  const T* t;
  const T* logq;
  const double* cdf;
  int K;
  T *theta, *target, *grad;
  int64_t R, P;
  const int32_t* partners;
  const T* u;
  uint64_t seed, iter, replica_offset;
  T *rec_theta, *rec_target;
  int32_t* partners_out;
  T* u_out;
  unsigned char* swap_out;
  T* log_rate_out;
};

// words 2, 3 of a Philox block as ey_rng_uniform_at<T> converts words 0, 1
template <typename T>
__device__ __forceinline__ T pt_accept_variate(uint32_t w2, uint32_t w3);
template <>
__device__ __forceinline__ float pt_accept_variate<float>(uint32_t w2, uint32_t) {
  return (float)(w2 >> 8) * 5.9604644775390625e-08f;
}
template <>
__device__ __forceinline__ double pt_accept_variate<double>(uint32_t w2, uint32_t w3) {
  return (double)(((uint64_t)w2 << 21) | (w3 >> 11)) * 1.1102230246251565e-16;
}

// Rows a and b trade places: a <- b * fa, b <- a * fb (theta: no factors), and the record rows ra, rb (or null) take the
// new values too.  Element p belongs to lane p % 64 in every step of the move, so a lane only ever meets what it wrote
// itself.  The trip count is wave-uniform; a lane beyond P loads element 0, drops it, and stores to its junk slot.
template <typename T, bool SCALE>
__device__ __forceinline__ void pt_exchange_rows(T* a, T* b, T* ra, T* rb, int64_t P, T fa, T fb, int lane) {
  T* const junk = pt_junk<T>(lane);
  for (int64_t p0 = 0; p0 < P; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool ok = p < P;
    const int64_t q = ok ? p : 0;
    const T va = a[q], vb = b[q];
    const T na = SCALE ? vb * fa : vb, nb = SCALE ? va * fb : va;
    *(ok ? a + q : junk) = na;
    *(ok ? b + q : junk) = nb;
    if (ra) {  // (wave-uniform)
      *(ok ? ra + q : junk) = na;
      *(ok ? rb + q : junk) = nb;
    }
  }
}

// One wave per replica r; state row k * R + r is temperature k of replica r.  The K tempered targets of the replica live
// in the wave's LDS region for the whole move: every lane takes the same decisions from the same values and every lane
// writes the same update to the same slot, so after the barrier behind the fill a lane reads nothing that it has not
// written itself.  The decision is made wave-uniform explicitly (readfirstlane): the row exchanges sit behind a scalar
// branch.
template <typename T>
__global__ __launch_bounds__(64 * PT_WAVES) void k_pt_between(const PtArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pt_smem[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int K = a.K, KP = (K + 63) & ~63;
  const int64_t R = a.R, P = a.P;
  T* tg = reinterpret_cast<T*>(pt_smem) + (size_t)w * KP;
  const int64_t r = (int64_t)blockIdx.x * PT_WAVES + w;
  const bool live = r < R;  // (the last workgroup may hold fewer than PT_WAVES replicas)
  if (live)
    for (int k0 = 0; k0 < KP; k0 += 64) {
      const int k = k0 + lane;
      tg[k] = a.target[(int64_t)(k < K ? k : 0) * R + r];  // (slots K .. KP-1 hold a copy of target 0 that nothing reads)
    }
  __syncthreads();
  if (!live) return;

  const EyRng rng = ey_rng_make(a.seed, a.replica_offset + (uint64_t)r, a.iter, EY_STREAM_PT);
  const bool l0 = lane == 0;
  for (int i = 0; i < K; ++i) {
    const int64_t o = (int64_t)i * R + r;
    int j;
    T u;
    if (a.partners) {
      j = a.partners[o];
      u = a.u[o];
    } else {
      uint32_t wd[4];
      ey_philox4x32_10((uint32_t)i, rng.c1, rng.c2, rng.c3, rng.k0, rng.k1, wd);
      const double v = (double)(((uint64_t)wd[0] << 21) | (wd[1] >> 11)) * 1.1102230246251565e-16;
      u = pt_accept_variate<T>(wd[2], wd[3]);
      // the first index whose cumulative probability exceeds v (never i: the diagonal adds nothing); v beyond the
      // rounded total goes to the last index that is not i
      const double* row = a.cdf + (size_t)i * K;
      int lo = 0, hi = K;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] > v) hi = mid; else lo = mid + 1;
      }
      j = lo < K ? lo : (i == K - 1 ? K - 2 : K - 1);
    }
    j = __builtin_amdgcn_readfirstlane(j);
    const bool valid = j >= 0 && j < K && j != i;  // a given partner may be anything: such a step exchanges nothing
    const int jv = valid ? j : i;
    const T ti = a.t[i], tj = a.t[jv];
    const T tgi = tg[i], tgj = tg[jv];
    const T dlogq = a.logq[(size_t)jv * K + i] - a.logq[(size_t)i * K + jv];
    T lr;
    const bool dec = ey_pt_decide<T>(tgi / ti, tgj / tj, ti, tj, &dlogq, u, &lr);
    const bool swap = __builtin_amdgcn_readfirstlane((int)(valid && dec)) != 0;
    if (a.partners_out) *(l0 ? a.partners_out + o : pt_junk<int32_t>(lane)) = j;
    if (a.u_out) *(l0 ? a.u_out + o : pt_junk<T>(lane)) = u;
    if (a.swap_out) *(l0 ? a.swap_out + o : pt_junk<unsigned char>(lane)) = swap ? 1 : 0;
    if (a.log_rate_out) *(l0 ? a.log_rate_out + o : pt_junk<T>(lane)) = valid ? lr : (T)NAN;
    if (swap) {
      // the host path's operations in its order: one division per factor, one multiplication per element
      const T fi = ti / tj, fj = tj / ti;
      const int64_t oi = o * P, oj = ((int64_t)j * R + r) * P;
      pt_exchange_rows<T, false>(a.theta + oi, a.theta + oj, a.rec_theta ? a.rec_theta + oi : nullptr,
                                 a.rec_theta ? a.rec_theta + oj : nullptr, P, T(1), T(1), lane);
      if (a.grad) pt_exchange_rows<T, true>(a.grad + oi, a.grad + oj, (T*)nullptr, (T*)nullptr, P, fi, fj, lane);
      tg[i] = tgj * fi;
      tg[j] = tgi * fj;
    }
  }
  for (int k0 = 0; k0 < KP; k0 += 64) {
    const int k = k0 + lane;
    const bool ok = k < K;
    const int64_t o = (int64_t)(ok ? k : 0) * R + r;
    const T v = tg[k];
    *(ok ? a.target + o : pt_junk<T>(lane)) = v;
    if (a.rec_target) *(ok ? a.rec_target + o : pt_junk<T>(lane)) = v;
  }
}

template <typename T>
static int pt_launch(const ey_pt_ladder* ld, void* theta, void* target, void* grad, int64_t R, int64_t P,
                     const int32_t* partners, const void* u, uint64_t seed, uint64_t iter, uint64_t replica_offset,
                     void* rec_theta, void* rec_target, int32_t* partners_out, void* u_out, void* swap_out,
                     void* log_rate_out, hipStream_t s) {
  PtArgs<T> a;
  a.t = (const T*)ld->d_t; a.logq = (const T*)ld->d_logq; a.cdf = ld->d_cdf; a.K = ld->K;
  a.theta = (T*)theta; a.target = (T*)target; a.grad = (T*)grad;
  a.R = R; a.P = P;
  a.partners = partners; a.u = (const T*)u;
  a.seed = seed; a.iter = iter; a.replica_offset = replica_offset;
  a.rec_theta = (T*)rec_theta; a.rec_target = (T*)rec_target;
  a.partners_out = partners_out; a.u_out = (T*)u_out; a.swap_out = (unsigned char*)swap_out;
  a.log_rate_out = (T*)log_rate_out;
  const size_t lds = (size_t)PT_WAVES * ((ld->K + 63) & ~63) * sizeof(T);
  const unsigned grid = (unsigned)((R + PT_WAVES - 1) / PT_WAVES);
  hipLaunchKernelGGL(k_pt_between<T>, dim3(grid), dim3(64 * PT_WAVES), lds, s, a);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

extern "C" {

int ey_pt_ladder_create(const double* t, const double* q, int K, int dtype, ey_pt_ladder** out) {
  const char* who = "ey_pt_ladder_create";
  if (!out) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  *out = nullptr;
  if (!t || !q) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": bad dtype");
  if (K < 2) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": a ladder needs at least two temperatures (K >= 2)");
  if (K > PT_KMAX)
    EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": k_pt_between keeps a replica's tempered targets in LDS and serves up to " +
                                    std::to_string(PT_KMAX) + " temperatures");
  const size_t n = (size_t)K, nn = n * n;
  std::vector<double> logq(nn, 0.0), cdf(nn, 0.0);
  for (size_t i = 0; i < n; ++i) {
    if (!(t[i] > 0.0) || !std::isfinite(t[i]))
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": temperature " + std::to_string(i) + " must be a positive finite number");
    double sum = 0.0;
    for (size_t j = 0; j < n; ++j) {
      if (j == i) continue;
      if (!(q[i * n + j] >= 0.0))
        EY_FAIL(EY_ERR_INVALID, std::string(who) + ": q[" + std::to_string(i) + "," + std::to_string(j) +
                                    "] must be a probability weight >= 0");
      sum += q[i * n + j];
    }
    if (!(sum > 0.0) || !std::isfinite(sum))
      EY_FAIL(EY_ERR_INVALID, std::string(who) + ": row " + std::to_string(i) + " of q must have a positive finite sum");
    double run = 0.0;
    for (size_t j = 0; j < n; ++j) {
      if (j != i) {
        const double p = q[i * n + j] / sum;
        logq[i * n + j] = std::log(p);
        run += p;
      }
      cdf[i * n + j] = run;
    }
  }
  ey_pt_ladder* ld = new ey_pt_ladder();
  ld->K = K; ld->dtype = dtype; ld->device = 0;
  ld->d_t = ld->d_logq = nullptr; ld->d_cdf = nullptr;
  const size_t esz = dtype == EY_F32 ? 4 : 8;
  std::vector<float> tf(t, t + n), lf(logq.begin(), logq.end());
  hipError_t e = hipGetDevice(&ld->device);
  if (e == hipSuccess) e = hipMalloc(&ld->d_t, esz * n);
  if (e == hipSuccess) e = hipMalloc(&ld->d_logq, esz * nn);
  if (e == hipSuccess) e = hipMalloc((void**)&ld->d_cdf, sizeof(double) * nn);
  if (e == hipSuccess)
    e = hipMemcpy(ld->d_t, dtype == EY_F32 ? (const void*)tf.data() : (const void*)t, esz * n, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(ld->d_logq, dtype == EY_F32 ? (const void*)lf.data() : (const void*)logq.data(), esz * nn,
                  hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ld->d_cdf, cdf.data(), sizeof(double) * nn, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    ey_pt_ladder_destroy(ld);
    EY_FAIL(EY_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  *out = ld;
  return EY_OK;
}

int ey_pt_ladder_destroy(ey_pt_ladder* ld) {
  if (!ld) return EY_OK;
  if (ld->d_t) (void)hipFree(ld->d_t);
  if (ld->d_logq) (void)hipFree(ld->d_logq);
  if (ld->d_cdf) (void)hipFree(ld->d_cdf);
  delete ld;
  return EY_OK;
}

int ey_pt_between(const ey_pt_ladder* ld, void* theta, void* target, void* grad, int64_t R, int64_t P,
                  const int32_t* partners, const void* u, uint64_t seed, uint64_t iter, uint64_t replica_offset,
                  void* rec_theta, void* rec_target, int32_t* partners_out, void* u_out, void* swap_out,
                  void* log_rate_out, void* stream) {
  const char* who = "ey_pt_between";
  if (!ld) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null ladder");
  if (R < 0 || P < 1 || P > 0x7fffffffLL) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": R or P out of range");
  if ((partners == nullptr) != (u == nullptr))
    EY_FAIL(EY_ERR_INVALID, std::string(who) + ": partners and u are given together or not at all");
  if ((R + PT_WAVES - 1) / PT_WAVES > 0x7fffffffLL) EY_FAIL(EY_ERR_UNSUPPORTED, std::string(who) + ": too many replicas");
  if (R == 0) return EY_OK;
  if (!theta || !target) EY_FAIL(EY_ERR_INVALID, std::string(who) + ": null argument");
  EY_HIP(hipSetDevice(ld->device));
  if (ld->dtype == EY_F32)
    return pt_launch<float>(ld, theta, target, grad, R, P, partners, u, seed, iter, replica_offset, rec_theta, rec_target,
                            partners_out, u_out, swap_out, log_rate_out, (hipStream_t)stream);
  return pt_launch<double>(ld, theta, target, grad, R, P, partners, u, seed, iter, replica_offset, rec_theta, rec_target,
                           partners_out, u_out, swap_out, log_rate_out, (hipStream_t)stream);
}

}  // extern "C"
