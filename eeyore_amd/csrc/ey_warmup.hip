// ey_metric_from_moments (include/eeyore_amd_warmup.h): a metric table from the running moments ey_hmc_metric_warmup leaves,
// Stan's regularised estimate as eeyore_amd/samplers/metric.py defines it for draws.
//
// One workgroup of 256 threads per ENTRY of the table: the one pooled estimate, or one chain's.  Everything is worked in
// double.  A thread owns elements of the (lower triangle of the) total; a pooled element is summed over the chains in index
// order, so the result depends on nothing but the inputs.  EY_METRIC_TRIL: the shrunk covariance is built in LDS as a packed
// lower triangle (row i at i (i + 1) / 2; P <= 128: 66 KB) and factored there column by column, thread i owning row i and
// summing over k = 0 .. j - 1 in that order; the pivot of a column is read by every thread, so a pivot that is not
// positive ends the factorisation in all of them at once.  The table is written only after the entry has come out fine:
// rounded once to its dtype, the strict upper triangle as zero.
#include "ey_common.h"

#include <cmath>

#define MM_THREADS 256
#define MM_MAX_P 128
#define MM_REG 1e-3    // samplers/metric.py: _REG
#define MM_REG_N 5.0   // ... and _REG_N

__device__ static inline bool mm_finite(double x) { return x - x == 0.0; }

// the regularised estimate of one element from its total: N / (N + 5) total / (N - 1), the diagonal + 1e-3 5 / (N + 5)
__device__ static inline double mm_shrink(double total, double N, bool diagonal) {
#pragma clang fp contract(off)  // the products and the sum rounded as metric.py's torch expressions round them
  const double s = (N / (N + MM_REG_N)) * (total / (N - 1.0));
  return diagonal ? s + MM_REG * (MM_REG_N / (N + MM_REG_N)) : s;
}

template <typename T, int FORM>
__global__ void __launch_bounds__(MM_THREADS) k_metric_from_moments(const double* mean, const double* M2, double n,
                                                                    int64_t C, int P, int pooled, T* table, int* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mm_smem[];
  double* gm = reinterpret_cast<double*>(mm_smem);  // [P] the grand mean (pooled)
  double* A = gm + P;                               // EY_METRIC_TRIL: the packed lower triangle
  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;                     // the entry
  const int64_t c0 = pooled ? 0 : e, c1 = pooled ? C : e + 1;
  const double N = pooled ? (double)C * n : n;
  const int64_t msz = FORM == EY_METRIC_TRIL ? (int64_t)P * P : (int64_t)P;
  int bad = 0;
  for (int i = tid; i < P; i += MM_THREADS) {
    double s = 0.0;
    for (int64_t c = c0; c < c1; ++c) s += mean[c * P + i];
    bad |= !mm_finite(s);
    gm[i] = s / (double)(c1 - c0);  // per chain: the chain's own mean, whose deviation is zero
  }
  __syncthreads();
  if constexpr (FORM == EY_METRIC_DIAG) {
    T* out = table + e * P;
    // (two passes: every thread must reach the vote below before any writes)
    for (int i = tid; i < P; i += MM_THREADS) {
      double s1 = 0.0, s2 = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const double dm = mean[c * P + i] - gm[i];
        s1 += M2[c * msz + i];
        s2 += dm * dm;
      }
      const double est = mm_shrink(s1 + n * s2, N, true);
      bad |= !(mm_finite(est) && est > 0.0);
    }
    if (__syncthreads_or(bad)) {
      if (tid == 0) status[e] = 1;
      return;
    }
    for (int i = tid; i < P; i += MM_THREADS) {
      double s1 = 0.0, s2 = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const double dm = mean[c * P + i] - gm[i];
        s1 += M2[c * msz + i];
        s2 += dm * dm;
      }
      out[i] = (T)sqrt(mm_shrink(s1 + n * s2, N, true));
    }
    if (tid == 0) status[e] = 0;
  } else {
    T* out = table + e * (int64_t)P * P;
    const int tri = P * (P + 1) / 2;
    for (int k = tid; k < tri; k += MM_THREADS) {
      int i = (int)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);  // the row of packed element k, corrected below
      while ((i + 1) * (i + 2) / 2 <= k) ++i;
      while (i * (i + 1) / 2 > k) --i;
      const int j = k - i * (i + 1) / 2;
      double s1 = 0.0, s2 = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        s1 += M2[c * msz + (int64_t)i * P + j];
        s2 += (mean[c * P + i] - gm[i]) * (mean[c * P + j] - gm[j]);
      }
      const double est = mm_shrink(s1 + n * s2, N, i == j);
      bad |= !mm_finite(est);
      A[k] = est;
    }
    if (__syncthreads_or(bad)) {
      if (tid == 0) status[e] = 1;
      return;
    }
    // Cholesky-Crout, column by column: A[i][j] <- (A[i][j] - sum_{k < j} L[i][k] L[j][k]) / L[j][j]
    for (int j = 0; j < P; ++j) {
      const int i = tid;
      if (i >= j && i < P) {
        double s = A[i * (i + 1) / 2 + j];
        for (int k = 0; k < j; ++k) s -= A[i * (i + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
        A[i * (i + 1) / 2 + j] = s;
      }
      __syncthreads();
      const double piv = A[j * (j + 1) / 2 + j];  // the same value in every thread
      __syncthreads();
      if (!(mm_finite(piv) && piv > 0.0)) {
        if (tid == 0) status[e] = 1;
        return;
      }
      const double dj = sqrt(piv);
      if (i >= j && i < P) A[i * (i + 1) / 2 + j] = i == j ? dj : A[i * (i + 1) / 2 + j] / dj;
      __syncthreads();
    }
    for (int k = tid; k < P * P; k += MM_THREADS) {
      const int i = k / P, j = k - i * P;
      out[k] = j <= i ? (T)A[i * (i + 1) / 2 + j] : T(0);
    }
    if (tid == 0) status[e] = 0;
  }
}

template <typename T, int FORM>
static int mm_launch(const void* mean, const void* M2, int64_t n, int64_t C, int P, int pooled, void* table, void* status,
                     hipStream_t s) {
  const size_t bytes = sizeof(double) * ((size_t)P + (FORM == EY_METRIC_TRIL ? (size_t)P * (P + 1) / 2 : 0));
  auto kernel = k_metric_from_moments<T, FORM>;
  if (bytes > 48 * 1024)
    EY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes));
  hipLaunchKernelGGL(kernel, dim3((unsigned)(pooled ? 1 : C)), dim3(MM_THREADS), bytes, s, (const double*)mean,
                     (const double*)M2, (double)n, C, P, pooled, (T*)table, (int*)status);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

extern "C" int ey_metric_from_moments(const void* mean, const void* M2, int64_t n, int64_t C, int64_t P, int form,
                                      int pooled, int dtype, void* table, void* status, void* stream) {
  const std::string who = "ey_metric_from_moments: ";
  if (!mean || !M2 || !table || !status) EY_FAIL(EY_ERR_INVALID, who + "null argument");
  if (form != EY_METRIC_DIAG && form != EY_METRIC_TRIL)
    EY_FAIL(EY_ERR_INVALID, who + "form must be EY_METRIC_DIAG or EY_METRIC_TRIL");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, who + "bad dtype");
  if (C < 1 || C > 0x7fffffffLL || P < 1 || P > 0x7fffffffLL) EY_FAIL(EY_ERR_INVALID, who + "C or P out of range");
  if (n < 1 || n > (1LL << 52)) EY_FAIL(EY_ERR_INVALID, who + "the count n is out of range");
  const double N = pooled ? (double)C * (double)n : (double)n;
  if (N < 2.0)
    EY_FAIL(EY_ERR_INVALID, who + "an estimate needs at least two draws (N = " + std::to_string((long long)N) + ")");
  if (form == EY_METRIC_TRIL && P > MM_MAX_P)
    EY_FAIL(EY_ERR_UNSUPPORTED, who + "P = " + std::to_string(P) + " exceeds the limit of " + std::to_string(MM_MAX_P) +
                                    " parameters of a dense metric (the factorisation lives in LDS)");
  hipStream_t s = (hipStream_t)stream;
  const int p = (int)P;
  pooled = pooled ? 1 : 0;
  if (form == EY_METRIC_TRIL)
    return dtype == EY_F32 ? mm_launch<float, EY_METRIC_TRIL>(mean, M2, n, C, p, pooled, table, status, s)
                           : mm_launch<double, EY_METRIC_TRIL>(mean, M2, n, C, p, pooled, table, status, s);
  return dtype == EY_F32 ? mm_launch<float, EY_METRIC_DIAG>(mean, M2, n, C, p, pooled, table, status, s)
                         : mm_launch<double, EY_METRIC_DIAG>(mean, M2, n, C, p, pooled, table, status, s);
}
