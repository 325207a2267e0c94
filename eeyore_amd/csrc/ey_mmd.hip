// Sums of a homogeneous kernel function over the pairs of two samples, for every chain and every prefix length at once
// (ey_kernel_pair_sums): what the reference's Kernel.sum_symm_K / sum_K compute with a Python loop per pair
// (eeyore/kernels/kernel.py:64-101) and its squared_mmd / mmd combine (eeyore/stats/discrepancy.py:3-19).  DESIGN.md 4.15.
//
// One workgroup of 256 lanes works through a list of 64 x 64 tiles of pairs of ONE chain: both row tiles are staged in LDS
// as f64, 16 columns at a time; lane (ty, tx) holds the 4 x 4 squared distances of rows ty + 16 r against rows tx + 16 s in
// registers, summed in the difference form over all columns, then applies the kernel function.  Nothing n x n is written.
// Every sum is formed in an order fixed by the shapes alone (no floating-point atomics): the same call gives the same bits.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "ey_common.h"

#define MM_T 64        // tile edge (rows of either operand per tile)
#define MM_PK 16       // columns staged per chunk
#define MM_LD 65       // row length of the transposed LDS images [MM_PK][MM_LD]: the pad spreads the staging writes over banks
#define MM_THREADS 256
#define MM_KMAX 1024
#define MM_S11 1
#define MM_S22 2
#define MM_S12 4

struct MmArgs {
  const void *x1, *x2;
  int64_t n1, n2;            // rows that take part: the last prefix length of either sample
  int64_t sn1, sc1, sn2, sc2;
  int p, k, kind, include_diag, mask, S;
  double scale, c1, c2;      // IsoSE: c1 = 1/(2l).  RQ: c1 = 1/(2al), c2 = -a.  Periodic: c1 = p, c2 = -2/l.
  const int64_t* lens;       // device [2, k] (len1 then len2), or null: k = 1 with the lengths n1, n2
  int64_t T11, T12, T22, nt2;
  double *o11, *o22, *o12;   // [*, k] outputs (the unsplit route writes them itself)
  double* part;              // [chains, S, 3, k] bucket sums of every workgroup (the split route)
  int64_t bcast;             // rows of the outputs that receive this launch's chain 0 (a shared x2: its s22 for every chain)
};

template <int KIND>
__device__ inline double mm_kfun(double d2, double scale, double c1, double c2) {
  if (KIND == 0) return scale * exp(-(d2 * c1));
  if (KIND == 1) return scale * pow(1.0 + d2 * c1, c2);
  const double s = sin(sqrt(d2) / c1);
  return scale * exp(c2 * (s * s));
}

// the sum of v over the workgroup in a fixed order, valid in thread 0 (two barriers; every lane must call it)
__device__ inline double mm_block_sum(double v, double* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // red is free again
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// first t with i < len[t]; k when there is none (the row lies beyond the last prefix)
__device__ inline int mm_bucket(const int64_t* len, int k, int64_t i) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (i < len[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// acc [3][k] bucket sums in LDS -> prefix sums -> the outputs of chain c (or of `bcast` chains)
__device__ inline void mm_emit(double* acc, const MmArgs& a, int64_t c, int tid) {
  __syncthreads();
  if (tid < 3 && ((a.mask >> tid) & 1)) {
    double run = 0.0;
    for (int t = 0; t < a.k; ++t) {
      run += acc[tid * a.k + t];
      acc[tid * a.k + t] = run;
    }
  }
  __syncthreads();
  const int64_t rows = a.bcast > 0 ? a.bcast : 1;
  const int64_t r0 = a.bcast > 0 ? 0 : c;
  for (int q = 0; q < 3; ++q) {
    if (!((a.mask >> q) & 1)) continue;
    double* o = q == 0 ? a.o11 : q == 1 ? a.o22 : a.o12;
    for (int64_t e = tid; e < rows * a.k; e += MM_THREADS) o[r0 * a.k + e] = acc[q * a.k + (int)(e % a.k)];
  }
}

template <typename T, int KIND>
__global__ __launch_bounds__(MM_THREADS) void k_mmd_tiles(const MmArgs a) {
  extern __shared__ double mm_dyn[];  // [3][k] bucket sums of this workgroup
  __shared__ double As[MM_PK * MM_LD], Bs[MM_PK * MM_LD];
  __shared__ double red[4];
  __shared__ int bkA[MM_T], bkB[MM_T], blist[2 * MM_T], bcount;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t c = blockIdx.x / a.S;
  const int slice = (int)(blockIdx.x - c * a.S);
  const int k = a.k;
  for (int e = tid; e < 3 * k; e += MM_THREADS) mm_dyn[e] = 0.0;
  __syncthreads();

  const T* x1 = (const T*)a.x1 + c * a.sc1;
  const T* x2 = (const T*)a.x2 + c * a.sc2;
  const int64_t Tall = a.T11 + a.T12 + a.T22;
  double run = 0.0;   // this lane's share of consecutive tiles that all belong to one (sum, bucket)
  int run_slot = -1;  // q * k + bucket of `run`

  for (int64_t tau = slice; tau < Tall; tau += a.S) {
    // ---- which tile
    int q;              // 0 s11, 1 s22, 2 s12
    int64_t ti, tj;
    if (tau < a.T11 + a.T22) {
      q = tau < a.T11 ? 0 : 1;
      const int64_t u = q == 0 ? tau : tau - a.T11;
      ti = (int64_t)((sqrt(8.0 * (double)u + 1.0) - 1.0) * 0.5);
      while (ti * (ti + 1) / 2 > u) --ti;
      while ((ti + 1) * (ti + 2) / 2 <= u) ++ti;
      tj = u - ti * (ti + 1) / 2;  // tj <= ti: tiles on or below the diagonal
    } else {
      q = 2;
      const int64_t u = tau - a.T11 - a.T22;
      ti = u / a.nt2;
      tj = u - ti * a.nt2;
    }
    const bool symm = q != 2, diag = symm && ti == tj;
    const T* xa = q == 1 ? x2 : x1;
    const T* xb = q == 0 ? x1 : x2;
    const int64_t sna = q == 1 ? a.sn2 : a.sn1, snb = q == 0 ? a.sn1 : a.sn2;
    const int64_t na = q == 1 ? a.n2 : a.n1, nb = q == 0 ? a.n1 : a.n2;
    const int64_t* lena = a.lens ? a.lens + (q == 1 ? k : 0) : nullptr;
    const int64_t* lenb = a.lens ? a.lens + (q == 0 ? 0 : k) : nullptr;
    const int64_t ra0 = ti * MM_T, rb0 = tj * MM_T;

    // ---- buckets of the tile's rows (k = 1: every row that takes part is in bucket 0)
    __syncthreads();  // the previous tile's epilogue has read its buckets
    if (tid < MM_T) {
      const int64_t i = ra0 + tid;
      bkA[tid] = i >= na ? k : lena ? mm_bucket(lena, k, i) : 0;
    } else if (tid < 2 * MM_T) {
      const int64_t j = rb0 + tid - MM_T;
      bkB[tid - MM_T] = j >= nb ? k : lenb ? mm_bucket(lenb, k, j) : 0;
    }

    // ---- squared distances, MM_PK columns at a time
    double d2[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) d2[r][s] = 0.0;
    for (int j0 = 0; j0 < a.p; j0 += MM_PK) {
      const int pw = min(MM_PK, a.p - j0);
      __syncthreads();  // the previous chunk has been read (first chunk: the previous tile's epilogue is over)
      for (int e = tid; e < MM_T * pw; e += MM_THREADS) {
        const int row = pw == MM_PK ? e >> 4 : e / pw, j = e - row * pw;
        const int64_t ia = ra0 + row, ib = rb0 + row;
        As[j * MM_LD + row] = ia < na ? (double)xa[ia * sna + j0 + j] : 0.0;
        Bs[j * MM_LD + row] = ib < nb ? (double)xb[ib * snb + j0 + j] : 0.0;
      }
      __syncthreads();
      if (pw == MM_PK) {
#pragma unroll
        for (int j = 0; j < MM_PK; ++j) {
          double av[4], bv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) av[r] = As[j * MM_LD + ty + 16 * r];
#pragma unroll
          for (int s = 0; s < 4; ++s) bv[s] = Bs[j * MM_LD + tx + 16 * s];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const double d = av[r] - bv[s];
              d2[r][s] = fma(d, d, d2[r][s]);
            }
        }
      } else {
        for (int j = 0; j < pw; ++j) {
          double av[4], bv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) av[r] = As[j * MM_LD + ty + 16 * r];
#pragma unroll
          for (int s = 0; s < 4; ++s) bv[s] = Bs[j * MM_LD + tx + 16 * s];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const double d = av[r] - bv[s];
              d2[r][s] = fma(d, d, d2[r][s]);
            }
        }
      }
    }

    // ---- kernel function and weights: symmetric sums count a pair below the diagonal twice, the diagonal once or not at all
    double val[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t i = ra0 + ty + 16 * r, j = rb0 + tx + 16 * s;
        double w = symm ? 2.0 : 1.0;
        if (diag) w = i > j ? 2.0 : i == j ? (a.include_diag ? 1.0 : 0.0) : 0.0;
        const bool on = i < na && j < nb && w != 0.0;
        const double kv = mm_kfun<KIND>(d2[r][s], a.scale, a.c1, a.c2);
        val[r][s] = on ? w * kv : 0.0;
      }

    // ---- into the buckets.  (bkA / bkB were written before the barriers of the chunk loop: p >= 1, so they are visible.)
    const int64_t la = min(na, ra0 + MM_T) - 1 - ra0, lb = min(nb, rb0 + MM_T) - 1 - rb0;  // last rows that take part
    const bool uniform = bkA[0] == bkA[la] && bkB[0] == bkB[lb];
    if (uniform) {  // the common case: no lookup per pair
      const int slot = q * k + max(bkA[0], bkB[0]);
      if (slot != run_slot) {
        if (run_slot >= 0) {
          const double t = mm_block_sum(run, red, tid);
          if (tid == 0) mm_dyn[run_slot] += t;
        }
        run = 0.0;
        run_slot = slot;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) run += val[r][s];
    } else {
      if (tid == 0) {  // the distinct buckets of the tile's rows, ascending (both lists are non-decreasing)
        int ia = 0, ib = 0, nl = 0;
        while (ia <= la || ib <= lb) {
          const int va = ia <= la ? bkA[ia] : 0x7fffffff, vb = ib <= lb ? bkB[ib] : 0x7fffffff;
          const int v = min(va, vb);
          if (nl == 0 || blist[nl - 1] != v) blist[nl++] = v;
          if (va == v) ++ia;
          if (vb == v) ++ib;
        }
        bcount = nl;
      }
      __syncthreads();
      const int nl = bcount;
      for (int m = 0; m < nl; ++m) {
        const int b = blist[m];
        double part = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int s = 0; s < 4; ++s) part += max(bkA[ty + 16 * r], bkB[tx + 16 * s]) == b ? val[r][s] : 0.0;
        const double t = mm_block_sum(part, red, tid);
        if (tid == 0) mm_dyn[q * k + b] += t;
      }
    }
  }
  if (run_slot >= 0) {  // (uniform over the workgroup: every lane sees the same tiles)
    const double t = mm_block_sum(run, red, tid);
    if (tid == 0) mm_dyn[run_slot] += t;
  }
  __syncthreads();
  if (a.part) {
    double* dst = a.part + (int64_t)blockIdx.x * 3 * k;
    for (int e = tid; e < 3 * k; e += MM_THREADS) dst[e] = mm_dyn[e];
  } else {
    mm_emit(mm_dyn, a, c, tid);
  }
}

// the split route: the bucket sums of a chain's S workgroups, added in the order of the workgroups
__global__ __launch_bounds__(MM_THREADS) void k_mmd_final(const MmArgs a) {
  extern __shared__ double mm_dyn[];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  for (int e = tid; e < 3 * a.k; e += MM_THREADS) {
    double v = 0.0;
    for (int s = 0; s < a.S; ++s) v += a.part[((c * a.S + s) * 3) * a.k + e];
    mm_dyn[e] = v;
  }
  mm_emit(mm_dyn, a, c, tid);
}

// Workgroups a launch should at least have before a chain's tiles stay in one workgroup: 4 per CU (8 fit by their waves
// and LDS), or EY_MMD_SPLIT_TARGET (read at every call: the tests name their chain counts from it).
static int64_t mm_split_target(int n_cu) {
  const char* e = getenv("EY_MMD_SPLIT_TARGET");
  if (e && atoll(e) > 0) return atoll(e);
  return 4 * (int64_t)n_cu;
}

static thread_local int t_mm_last_split = 0;
extern "C" int ey_debug_mmd_last_split(void) { return t_mm_last_split; }

static int mm_launch(MmArgs a, int64_t chains, int dtype, int64_t target, hipStream_t s) {
  const int64_t Tall = a.T11 + a.T12 + a.T22;
  int64_t S = 1;
  if (chains < target) S = std::max<int64_t>(1, std::min<int64_t>(Tall, (target + chains - 1) / chains));
  if (chains * S > 0xffffff) EY_FAIL(EY_ERR_UNSUPPORTED, "ey_kernel_pair_sums: too many chains for one launch");
  a.S = (int)S;
  if (a.mask & MM_S12) t_mm_last_split = (int)S;
  const size_t lds = (size_t)3 * a.k * sizeof(double);
  double* part = nullptr;
  if (S > 1) EY_HIP(hipMallocAsync((void**)&part, (size_t)chains * S * 3 * a.k * sizeof(double), s));
  a.part = part;
  // (nothing returns between the allocation and its release)
  const dim3 grid((unsigned)(chains * S)), block(MM_THREADS);
#define MM_GO(T, KIND) hipLaunchKernelGGL((k_mmd_tiles<T, KIND>), grid, block, lds, s, a)
  if (dtype == EY_F32) {
    if (a.kind == 0) MM_GO(float, 0); else if (a.kind == 1) MM_GO(float, 1); else MM_GO(float, 2);
  } else {
    if (a.kind == 0) MM_GO(double, 0); else if (a.kind == 1) MM_GO(double, 1); else MM_GO(double, 2);
  }
#undef MM_GO
  hipError_t le = hipGetLastError();
  if (S > 1) {
    if (le == hipSuccess) {
      hipLaunchKernelGGL(k_mmd_final, dim3((unsigned)chains), dim3(MM_THREADS), lds, s, a);
      le = hipGetLastError();
    }
    (void)hipFreeAsync(part, s);
  }
  EY_HIP(le);
  return EY_OK;
}

extern "C" int ey_kernel_pair_sums(const void* x1, int64_t n1, int64_t C, int64_t p, int64_t stride1_n, int64_t stride1_c,
                                   const void* x2, int64_t n2, int64_t stride2_n, int64_t stride2_c, int dtype, int kind,
                                   const double* params, const int64_t* len1, const int64_t* len2, int64_t k,
                                   int include_diag, void* s11, void* s22, void* s12, void* stream) {
  // ---- everything is checked before anything touches the device
  if (!x1 || !x2) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: null sample pointer");
  if (!s11 || !s22 || !s12) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: null output pointer");
  if (n1 < 1 || n2 < 1 || C < 1 || p < 1 || k < 1) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: n1, n2, C, p and k must be >= 1");
  if (dtype != EY_F32 && dtype != EY_F64) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: bad dtype");
  if (kind < 0 || kind > 2) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: kind must be 0 (IsoSE), 1 (RQ) or 2 (Periodic)");
  if (!params) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: null params");
  const double scale = params[0], l = params[1];
  if (!(std::isfinite(scale) && scale > 0.0) || !(std::isfinite(l) && l > 0.0))
    EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: scale and l must be finite and > 0");
  if (kind == 1 && !(std::isfinite(params[2]) && params[2] > 0.0)) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: RQ's a must be finite and > 0");
  if (kind == 2 && !(std::isfinite(params[2]) && params[2] != 0.0)) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: Periodic's p must be finite and not 0");
  if (k > MM_KMAX) EY_FAIL(EY_ERR_UNSUPPORTED, "ey_kernel_pair_sums: at most 1024 prefix lengths per call");
  if ((len1 == nullptr) != (len2 == nullptr)) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: len1 and len2 come together or not at all");
  if (!len1 && k != 1) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: k > 1 needs len1 and len2");
  if (p > 0x7fffffff - MM_PK) EY_FAIL(EY_ERR_UNSUPPORTED, "ey_kernel_pair_sums: p too large");
  std::vector<int64_t> lens(2 * (size_t)k);
  for (int64_t t = 0; t < k; ++t) {
    lens[t] = len1 ? len1[t] : n1;
    lens[k + t] = len2 ? len2[t] : n2;
  }
  for (int w = 0; w < 2; ++w) {
    const int64_t n = w ? n2 : n1;
    for (int64_t t = 0; t < k; ++t) {
      const int64_t v = lens[w * k + t];
      if (v < 1 || v > n) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: a prefix length lies outside [1, n]");
      if (t && v < lens[w * k + t - 1]) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: prefix lengths must be non-decreasing");
      if (!include_diag && v < 2) EY_FAIL(EY_ERR_INVALID, "ey_kernel_pair_sums: include_diag = 0 needs prefix lengths >= 2");
    }
  }

  // ---- the device
  hipStream_t s = (hipStream_t)stream;
  int dev = 0, n_cu = 0;
  EY_HIP(hipGetDevice(&dev));
  EY_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  const int64_t target = mm_split_target(n_cu);

  MmArgs a{};
  a.x1 = x1; a.x2 = x2;
  a.n1 = lens[k - 1]; a.n2 = lens[2 * k - 1];  // rows beyond the last prefix take no part
  a.sn1 = stride1_n; a.sc1 = stride1_c; a.sn2 = stride2_n; a.sc2 = stride2_c;
  a.p = (int)p; a.k = (int)k; a.kind = kind; a.include_diag = include_diag ? 1 : 0;
  a.scale = scale;
  if (kind == 0) { a.c1 = 1.0 / (2.0 * l); a.c2 = 0.0; }
  else if (kind == 1) { a.c1 = 1.0 / (2.0 * params[2] * l); a.c2 = -params[2]; }
  else { a.c1 = params[2]; a.c2 = -2.0 / l; }
  a.o11 = (double*)s11; a.o22 = (double*)s22; a.o12 = (double*)s12;
  const int64_t nt1 = (a.n1 + MM_T - 1) / MM_T, nt2 = (a.n2 + MM_T - 1) / MM_T;
  a.nt2 = nt2;

  int64_t* d_lens = nullptr;
  if (k > 1) {  // (k = 1: the lengths are a.n1, a.n2 themselves)
    EY_HIP(hipMallocAsync((void**)&d_lens, lens.size() * sizeof(int64_t), s));
    const hipError_t ce = hipMemcpyAsync(d_lens, lens.data(), lens.size() * sizeof(int64_t), hipMemcpyHostToDevice, s);
    // `lens` is pageable host memory of this call: the copy has left it before the call returns
    const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(s) : ce;
    if (se != hipSuccess) {
      (void)hipFreeAsync(d_lens, s);
      EY_HIP(se);
    }
  }
  a.lens = d_lens;

  int rc = EY_OK;
  const bool shared2 = stride2_c == 0;
  if (shared2) {  // one x2 for all chains: its own sums once, written to every chain's row
    MmArgs b = a;
    b.mask = MM_S22; b.T11 = 0; b.T12 = 0; b.T22 = nt2 * (nt2 + 1) / 2;
    b.bcast = C;
    rc = mm_launch(b, 1, dtype, target, s);
    a.mask = MM_S11 | MM_S12;
    a.T22 = 0;
  } else {
    a.mask = MM_S11 | MM_S22 | MM_S12;
    a.T22 = nt2 * (nt2 + 1) / 2;
  }
  if (rc == EY_OK) {
    a.T11 = nt1 * (nt1 + 1) / 2;
    a.T12 = nt1 * nt2;
    a.bcast = 0;
    rc = mm_launch(a, C, dtype, target, s);
  }
  if (d_lens) (void)hipFreeAsync(d_lens, s);
  return rc;
}
