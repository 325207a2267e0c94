// Generic chain-batched kernels: any MLP (dims/bias/activations/likelihood of the plan), f32 and f64.
// One wavefront (64 lanes) per chain; theta, momentum and gradient live in LDS for the whole step.
//
// Reference path restated (paths relative to papamarkou/eeyore):
//   MLP.forward                eeyore/models/mlp.py:45-50
//   BCE-sum / CE-sum           eeyore/constants/constants.py:15-18, eeyore/stats/loss.py:1-11
//   log_lik/log_prior/target   eeyore/models/bayesian_model.py:30-56
//   gradient (autograd there)  eeyore/models/log_target_model.py:15-23
//   HMC leapfrog / draw        eeyore/samplers/hmc.py:100-156
//   MALA draw                  eeyore/samplers/mala.py:46-82
//   MH draw                    eeyore/samplers/metropolis_hastings.py:41-73
//
// Data rows are processed in tiles of 64 (lane <-> row).  Forward is row-parallel (weights broadcast from
// LDS); the weight gradient is parameter-parallel (lane <-> parameter, contraction over the tile's rows);
// the input gradient is row-parallel again.  Tile columns use a stride of 65 elements so that the
// parameter-parallel reads (different rows j, same column n) hit different LDS banks.
#include <atomic>
#include <type_traits>

#include "ey_common.h"

// EY_GEN_PART: ey_nuts.hip includes this file with EY_GEN_PART 1 for what its kernel shares with the kernels here (the
// evaluation, the LDS image, the sweeps and leapfrog halves under a metric, the launch helpers): every entry point, and
// with them every kernel instantiation of this unit, is then left out.  0 (this file as it stands) = the whole unit.
#ifndef EY_GEN_PART
#define EY_GEN_PART 0
#endif

#define TS 65
#define WAVE 64

template <typename T>
struct Num;
template <>
struct Num<float> {
  static __device__ float exp(float v) { return expf(v); }
  static __device__ float log(float v) { return logf(v); }
  static __device__ float tanh(float v) { return tanhf(v); }
  static __device__ float sqrt(float v) { return sqrtf(v); }
  static __device__ float log1p(float v) { return log1pf(v); }
  static __device__ float abs(float v) { return fabsf(v); }
};
template <>
struct Num<double> {
  static __device__ double exp(double v) { return ::exp(v); }
  static __device__ double log(double v) { return ::log(v); }
  static __device__ double tanh(double v) { return ::tanh(v); }
  static __device__ double sqrt(double v) { return ::sqrt(v); }
  static __device__ double log1p(double v) { return ::log1p(v); }
  static __device__ double abs(double v) { return ::fabs(v); }
};

template <typename T>
__device__ inline T act_fn(int code, T g) {
  switch (code) {
    case EY_ACT_SIGMOID: return T(1) / (T(1) + Num<T>::exp(-g));
    case EY_ACT_TANH: return Num<T>::tanh(g);
    case EY_ACT_RELU: return g > T(0) ? g : T(0);
    default: return g;
  }
}
template <typename T>
__device__ inline T dact_fn(int code, T h) {
  switch (code) {
    case EY_ACT_SIGMOID: return h * (T(1) - h);
    case EY_ACT_TANH: return T(1) - h * h;
    case EY_ACT_RELU: return h > T(0) ? T(1) : T(0);
    default: return T(1);
  }
}

// The per-output likelihood terms, written once for tiny_rows and eval_target (the arithmetic is the same by construction).
// They, and the steps the kernels share further down, are macros in the style of EY_LANE_PASS below: this compiler schedules
// and allocates a kernel differently around an inlined function, and a macro leaves its code as it was.
// EY_REG_TERM: one output's term of a regression log-likelihood and its derivative in the output (include/eeyore_amd.h:
// enum ey_lik): r = out - y, lw = 1/s^2 or 1/s, lc the log-normaliser of one output.  `lik` is a kernel argument: the
// branches are scalar.  It DECLARES the two names the caller passes as `term` and `d` (so it stands where a declaration
// may) and leaves nothing else in the caller's scope; beside its arguments it reads T alone.
#define EY_REG_TERM(lik, o, yy, lw, lc, term, d)                                                                     \
  T term, d;                                                                                                         \
  do {                                                                                                               \
    const T ey_r_ = (o) - (yy);                                                                                      \
    if ((lik) == EY_LIK_GAUSS_SUM) {                                                                                 \
      term = (lc) - T(0.5) * ey_r_ * ey_r_ * (lw);                                                                   \
      d = -ey_r_ * (lw);                                                                                             \
    } else if ((lik) == EY_LIK_LAPLACE_SUM) {                                                                        \
      term = (lc) - Num<T>::abs(ey_r_) * (lw);                                                                       \
      d = ey_r_ > T(0) ? -(lw) : (ey_r_ < T(0) ? (lw) : T(0)); /* -sign(r) / s with sign(0) = 0 */                   \
    } else { /* EY_LIK_POISSON_SUM: out is the log-rate; nothing clamped (an overflowing exp gives a -inf target) */ \
      const T ey_e_ = Num<T>::exp(o);                                                                                \
      term = (yy) * (o) - ey_e_;                                                                                     \
      d = (yy) - ey_e_;                                                                                              \
    }                                                                                                                \
  } while (0)

// ... and of the BCE sum: naive logs exactly as eeyore/stats/loss.py:2 (NaN once a sigmoid saturates)
#define EY_BCE_TERM(o, yy) (Num<T>::log(o) * (yy) + Num<T>::log(T(1) - (o)) * (T(1) - (yy)))
#define EY_BCE_DOUT(o, yy) ((yy) / (o) - (T(1) - (yy)) / (T(1) - (o)))
// A lane-strided pass over n elements with the SAME trip count in every lane: index i = lane + 64 k clamped to n - 1, `on`
// saying whether the lane's element exists.  A lane beyond n in the last round repeats the work of element n - 1's owner --
// the same inputs, hence the same bits to the same address -- and must keep its terms out of sums (select the term's
// INPUT to zero, so that the expression contracts as it did).  No memory operation behind a per-lane branch, no
// loop-carried register under a partial EXEC mask.
#define EY_LANE_PASS(n, i, on)                                                                               \
  for (int ey_k_ = 0, ey_n_ = (n), i = lane < ey_n_ ? lane : ey_n_ - 1, on = lane < ey_n_; ey_k_ < (ey_n_ + WAVE - 1) / WAVE; \
       ++ey_k_, on = lane + ey_k_ * WAVE < ey_n_, i = on ? lane + ey_k_ * WAVE : ey_n_ - 1)

template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// LDS carve for one chain
template <typename T>
struct Lds {
  T* th;   // [P] position
  T* gr;   // [P] gradient at th
  T* a;    // [P] momentum (HMC) / proposal (MALA, MH)
  T* b;    // [P] gradient at the proposal (MALA)
  T* act;  // [hrows * TS] activations of the current row tile, all layers
  T* dl;   // [2 * dmax * TS] delta ping-pong
};

template <typename T>
__device__ inline Lds<T> carve(const EyModel& m, unsigned char* smem, int nvec) {
  Lds<T> l;
  T* p = reinterpret_cast<T*>(smem);
  const int Ppad = (m.P + 3) & ~3;
  l.th = p; p += Ppad;
  l.gr = p; p += Ppad;
  l.a = p; if (nvec > 2) p += Ppad;
  l.b = p; if (nvec > 3) p += Ppad;
  l.act = p; p += m.hrows * TS;
  l.dl = p;
  return l;
}

__host__ __device__ static size_t lds_bytes(const EyModel& m, int nvec, size_t esz) {
  const size_t Ppad = (m.P + 3) & ~3;
  return esz * (nvec * Ppad + (size_t)m.hrows * TS + 2 * (size_t)m.dmax * TS);
}

// ROW WAVES.  A workgroup is one chain.  With the register-resident evaluation (tiny models) and a batch of several 64-row
// tiles, the tiles of one evaluation are independent until the gradient is summed: the workgroup then has up to four
// waves, every wave runs the WHOLE kernel on its own LDS copy of the chain's state (same inputs, same instructions: the
// same bits in every wave -- random draws, proposals, accept decisions), but takes only every NW-th row tile inside an
// evaluation; the waves' partial gradients and log-likelihoods meet in LDS and every wave adds them in the order wave 0,
// 1, 2, 3, so all waves continue with identical totals.  Only wave 0 writes to global memory; the workgroup barriers the
// kernels already have order those writes before the other waves' next reads (one CU, one vector cache).  The number of
// waves is a plan option (EY_OPT_ROW_WAVES): the order in which a gradient is summed differs between one wave and several, so
// a caller who needs a chain's bits to be independent of how many chains share its launch pins it on or off.
#define RW_MAX 4
struct RowWaves {
  int wave, nw;
  void* part;  // exchange buffer [P + 1][nw][64 lanes] of per-lane partial sums, then [P + 4] totals
};
template <typename T>
__device__ inline RowWaves row_waves(const EyModel& m, unsigned char* smem, int nvec) {
  RowWaves rw;
  rw.wave = threadIdx.x >> 6;
  rw.nw = blockDim.x >> 6;
  rw.part = smem + (size_t)rw.nw * lds_bytes(m, nvec, sizeof(T));
  return rw;
}
static size_t row_waves_exchange(const EyModel& m, size_t esz, int nw) {
  return nw > 1 ? esz * ((size_t)(m.P + 1) * nw * WAVE + m.P + 4) : 0;
}
// EY_OPT_ROW_WAVES: off, on (whenever the batch has two row tiles or more), or auto = on while one wave per chain would
// leave SIMDs idle (C <= 4 x CUs: at 256 chains MALA on MLP(2-3-2-1), N = 256, takes 5.4 us per draw instead of 7.7; with
// the chip full of chains the waves' repeated scalar work costs 3 x in throughput, so there it stays off).
static int row_waves_for(const ey_plan* pl, bool tiny, int64_t C) {
  if (!tiny || pl->m.N < 2 * WAVE || pl->row_waves == EY_ROW_WAVES_OFF) return 1;
  if (pl->row_waves == EY_ROW_WAVES_AUTO && C > 4 * (int64_t)(pl->n_cu > 0 ? pl->n_cu : 256)) return 1;
  int nw = std::min(RW_MAX, (pl->m.N + WAVE - 1) / WAVE);
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  while (nw > 1 && row_waves_exchange(pl->m, esz, nw) > 32768) --nw;  // several chains per CU must still fit
  return nw;
}
static size_t lds_total(const EyModel& m, int nvec, size_t esz, int nw) {
  return nw * lds_bytes(m, nvec, esz) + row_waves_exchange(m, esz, nw);
}

// ------------------------------------------------------------------ register-resident evaluation of tiny models
// The models of the reference's own tests and examples are tiny (MLP(2-2-1), (2-3-2-1), (4-3-3): P = 9 .. 27).  The
// tile loop of eval_target below walks such a model through LDS one dependent round trip after the other (a (j, i)
// loop nest of runtime extents, every load behind the previous store): ~20 000 cycles per 64-row tile of MLP(2-3-2-1).
// For at most three layers, at most 8 inputs and every other width at most 4, the same arithmetic fits in registers:
// lane <-> row, the weights as wave-uniform register copies (read once per evaluation from the position in LDS), a row's
// activations and deltas in registers, the weight gradient accumulated PER LANE over the lane's rows and summed over
// the lanes once per evaluation (DPP adds in a fixed order: deterministic).  Every loop is unrolled to its maximum
// extent with wave-uniform guards, so all register arrays are indexed by constants.
#define TINY_D0 8
#define TINY_DH 4
static bool ey_generic_tiny_ok(const EyModel& m) {
  if (m.nl < 1 || m.nl > 3 || m.dims[0] > TINY_D0) return false;
  for (int k = 1; k <= m.nl; ++k)
    if (m.dims[k] > TINY_DH) return false;
  return true;
}

// Shape policies of the evaluation below: TinyDyn reads the extents from the model at run time (every unrolled
// iteration behind a wave-uniform guard: ~300 scalar branches per tile of MLP(2-3-2-1)); TinyFix<...> states them at
// compile time, so the guards fold away and only the registers the shape needs remain.  TinyFix exists for the shapes
// the reference's own tests and examples use (mlp.py's default 1-2-1, XOR 2-2-1 and 2-3-2-1, 2-3-3-2, Iris 4-3-3 and
// 4-3-2-3, the banknotes logistic regression 4-1).
struct TinyOff {
  static constexpr bool on = false;
};
struct TinyDyn {
  static constexpr bool on = true;
  static __device__ __forceinline__ int nl(const EyModel& m) { return m.nl; }
  static __device__ __forceinline__ int dim(const EyModel& m, int k) { return m.dims[k]; }
};
template <int NL, int D0, int D1, int D2, int D3>
struct TinyFix {
  static constexpr bool on = true;
  static __device__ __forceinline__ constexpr int nl(const EyModel&) { return NL; }
  static __device__ __forceinline__ constexpr int dim(const EyModel&, int k) { return k == 0 ? D0 : (k == 1 ? D1 : (k == 2 ? D2 : D3)); }
};

// A target that is no MLP: a Gaussian mixture on theta itself (EY_KIND_MIX, mix_target below).  One wave per chain, no
// row-wave form (on = false).
struct TargetMix {
  static constexpr bool on = false;
};
// ... or a separable exponential tilt on theta itself (EY_KIND_TILT, tilt_target below): the same form
struct TargetTilt {
  static constexpr bool on = false;
};

template <int CTRL, int ROWMASK, typename T>
__device__ __forceinline__ T tiny_dpp(T v) {
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xF, false));
  } else {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROWMASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROWMASK, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
  }
}
// wave total as a uniform value: adds inside each 16-lane row, then row_bcast:15 / :31 carry the row totals to lane 63
template <typename T>
__device__ __forceinline__ T tiny_wsum(T v) {
  v += tiny_dpp<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v += tiny_dpp<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v += tiny_dpp<0x141, 0xF>(v);  // row_half_mirror
  v += tiny_dpp<0x140, 0xF>(v);  // row_mirror
  v += tiny_dpp<0x142, 0xA>(v);  // row_bcast:15 (a masked-off row adds the 0 of update_dpp's old value)
  v += tiny_dpp<0x143, 0xC>(v);  // row_bcast:31
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
  } else {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
  }
}

// activation of up to four values with the (wave-uniform) switch outside the element loop
template <typename T>
__device__ __forceinline__ void tiny_act(int code, T (&h)[TINY_DH], int n) {
  if (code == EY_ACT_NONE) return;
#pragma unroll
  for (int j = 0; j < TINY_DH; ++j)
    if (j < n) h[j] = act_fn<T>(code, h[j]);
}

// The row loop of eval_target for a tiny model: the sum of the rows' log-likelihood terms (per lane: the caller adds
// the lanes) and, when GRAD, the gradient of the log-likelihood in gr (LDS, canonical layout).
template <typename T, bool GRAD, class S>
__device__ __forceinline__ T tiny_rows(const EyModel& m, const T* th, T* gr, bool has_temp, T temp, T* row_out,
                                       const RowWaves& rw, T* fwd_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const T* x = static_cast<const T*>(m.x);
  const T* y = static_cast<const T*>(m.y);
  const int nl = S::nl(m), dK = S::dim(m, nl), d0 = S::dim(m, 0);
  // wave-uniform register copies of the position, padded to [3][4][8 | 4] (+ [3][4] biases)
  T W[3][TINY_DH][TINY_D0], B[3][TINY_DH], G[3][TINY_DH][TINY_D0], GB[3][TINY_DH];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < nl) {
      const int din = S::dim(m, k), dout = S::dim(m, k + 1);
#pragma unroll
      for (int j = 0; j < TINY_DH; ++j) {
#pragma unroll
        for (int i = 0; i < (k == 0 ? TINY_D0 : TINY_DH); ++i) {
          W[k][j][i] = (j < dout && i < din) ? th[m.woff[k] + j * din + i] : T(0);
          G[k][j][i] = T(0);
        }
        B[k][j] = (j < dout && m.boff[k] >= 0) ? th[m.boff[k] + j] : T(0);
        GB[k][j] = T(0);
      }
    }
  }
  T lik = T(0);
  for (int n0 = rw.wave * WAVE; n0 < m.N; n0 += rw.nw * WAVE) {
    const int n = n0 + lane;
    const bool valid = n < m.N;
    T h0[TINY_D0], h[3][TINY_DH];  // h[k] = output of layer k
#pragma unroll
    for (int i = 0; i < TINY_D0; ++i) h0[i] = (i < d0 && valid) ? x[(size_t)n * d0 + i] : T(0);
    // ---- forward (mlp.py:45-50)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k < nl) {
        const int din = S::dim(m, k), dout = S::dim(m, k + 1);
#pragma unroll
        for (int j = 0; j < TINY_DH; ++j) {
          T g = T(0);
          if (j < dout) {
#pragma unroll
            for (int i = 0; i < (k == 0 ? TINY_D0 : TINY_DH); ++i)
              if (i < din) g += (k == 0 ? h0[i] : h[k == 0 ? 0 : k - 1][i]) * W[k][j][i];
            g += B[k][j];  // 0 when the layer has no bias
          }
          h[k][j] = g;
        }
        tiny_act<T>(m.act[k], h[k], dout);
      }
    }
    // ---- likelihood and output delta (constants.py:15-18, loss.py:1-11): the arithmetic of eval_target
    T out[TINY_DH], d[TINY_DH];
#pragma unroll
    for (int j = 0; j < TINY_DH; ++j) {
      out[j] = nl == 1 ? h[0][j] : (nl == 2 ? h[1][j] : h[2][j]);
      d[j] = T(0);
    }
    const int act_out = m.act[nl - 1];
    if (fwd_out && valid) {  // ey_forward: the row's outputs, next to row_out below
#pragma unroll
      for (int j = 0; j < TINY_DH; ++j)
        if (j < dK) fwd_out[(size_t)n * dK + j] = out[j];
    }
    T row_lik = T(0);
    // m.lik is a kernel argument: the branches on it are scalar
    if (m.lik >= EY_LIK_GAUSS_SUM) {
      // regression (include/eeyore_amd.h: enum ey_lik): r = out - y, lw = 1/s^2 or 1/s, lc the log-normaliser of one output
      const T lw = T(m.lik_w), lc = T(m.lik_c);
#pragma unroll
      for (int j = 0; j < TINY_DH; ++j)
        if (j < dK) {
          const T o = out[j];
          const T yy = valid ? y[(size_t)n * dK + j] : T(0);
          EY_REG_TERM(m.lik, o, yy, lw, lc, term, dd);
          lik += valid ? term : T(0);
          row_lik += term;
          if (GRAD) d[j] = valid ? dd * dact_fn<T>(act_out, o) : T(0);
        }
    } else
    if (m.lik == EY_LIK_BCE_SUM) {
#pragma unroll
      for (int j = 0; j < TINY_DH; ++j)
        if (j < dK) {
          const T o = out[j];
          const T yy = valid ? y[(size_t)n * dK + j] : T(0);
          const T term = EY_BCE_TERM(o, yy);
          lik += valid ? term : T(0);
          row_lik += term;
          if (GRAD) {
            const T dd = EY_BCE_DOUT(o, yy) * dact_fn<T>(act_out, o);
            d[j] = valid ? dd : T(0);
          }
        }
    } else {
      const int lab = valid ? m.labels[n] : 0;
      T mx = out[0];
#pragma unroll
      for (int j = 1; j < TINY_DH; ++j)
        if (j < dK) mx = fmax(mx, out[j]);
      T ssum = T(0), olab = out[0];
#pragma unroll
      for (int j = 0; j < TINY_DH; ++j)
        if (j < dK) {
          ssum += Num<T>::exp(out[j] - mx);
          if (j == lab) olab = out[j];
        }
      row_lik = olab - (mx + Num<T>::log(ssum));
      lik += valid ? row_lik : T(0);
      if (GRAD) {
#pragma unroll
        for (int j = 0; j < TINY_DH; ++j)
          if (j < dK) {
            const T dd = ((j == lab ? T(1) : T(0)) - Num<T>::exp(out[j] - mx) / ssum) * dact_fn<T>(act_out, out[j]);
            d[j] = valid ? dd : T(0);
          }
      }
    }
    if (row_out && valid) row_out[n] = has_temp ? row_lik * temp : row_lik;
    if (GRAD) {
      // ---- backward: dW_k += delta_k (x) h_{k-1}, db_k += delta_k, delta_{k-1} = (W_k^T delta_k) * act'(h_{k-1})
#pragma unroll
      for (int k = 2; k >= 0; --k) {
        if (k < nl) {
          const int din = S::dim(m, k), dout = S::dim(m, k + 1);
#pragma unroll
          for (int j = 0; j < TINY_DH; ++j)
            if (j < dout) {
#pragma unroll
              for (int i = 0; i < (k == 0 ? TINY_D0 : TINY_DH); ++i)
                if (i < din) G[k][j][i] += d[j] * (k == 0 ? h0[i] : h[k == 0 ? 0 : k - 1][i]);
              GB[k][j] += d[j];
            }
          if (k > 0) {
            T dn[TINY_DH];
#pragma unroll
            for (int i = 0; i < TINY_DH; ++i) {
              T a = T(0);
              if (i < din) {
#pragma unroll
                for (int j = 0; j < TINY_DH; ++j)
                  if (j < dout) a += d[j] * W[k][j][i];
                a *= dact_fn<T>(m.act[k - 1], h[k - 1][i]);
              }
              dn[i] = a;
            }
#pragma unroll
            for (int i = 0; i < TINY_DH; ++i) d[i] = dn[i];
          }
        }
      }
    }
  }
  if (rw.nw > 1) {
    // ---- ROW WAVES: every wave leaves its per-lane partial sums in the exchange buffer; the parameters (and the
    // log-likelihood, as entry P) are then shared out over the waves, each adding the waves' partials lane by lane in the
    // order wave 0, 1, ... and reducing over the lanes as below; every wave copies the totals into its own gradient.
    T* ex = static_cast<T*>(rw.part);
    T* totals = ex + (size_t)(m.P + 1) * rw.nw * WAVE;
    auto slot = [&](int idx) { return ex + ((size_t)idx * rw.nw + rw.wave) * WAVE + lane; };
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k < nl) {
          const int din = S::dim(m, k), dout = S::dim(m, k + 1);
#pragma unroll
          for (int j = 0; j < TINY_DH; ++j)
            if (j < dout) {
#pragma unroll
              for (int i = 0; i < (k == 0 ? TINY_D0 : TINY_DH); ++i)
                if (i < din) *slot(m.woff[k] + j * din + i) = G[k][j][i];
              if (m.boff[k] >= 0) *slot(m.boff[k] + j) = GB[k][j];
            }
        }
      }
    }
    *slot(m.P) = lik;
    __syncthreads();
    for (int idx = (GRAD ? rw.wave : m.P + rw.wave); idx <= m.P; idx += rw.nw) {
      const T* src = ex + (size_t)idx * rw.nw * WAVE + lane;
      T v = src[0];
      for (int w = 1; w < rw.nw; ++w) v += src[w * WAVE];
      const T tot = tiny_wsum<T>(v);
      totals[idx] = tot;  // (wave-uniform: every lane stores it)
    }
    __syncthreads();
    if (GRAD)
      for (int i = lane; i < m.P; i += WAVE) gr[i] = totals[i];
    return lane == 0 ? totals[m.P] : T(0);  // the caller's wave_sum hands it to every lane
  }
  if (GRAD) {
    // ---- the lanes' partial gradients, summed in a fixed order, into the canonical layout
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k < nl) {
        const int din = S::dim(m, k), dout = S::dim(m, k + 1);
#pragma unroll
        for (int j = 0; j < TINY_DH; ++j)
          if (j < dout) {
#pragma unroll
            for (int i = 0; i < (k == 0 ? TINY_D0 : TINY_DH); ++i)
              if (i < din) {
                // (the total is wave-uniform: every lane stores it -- no store behind a per-lane branch while the
                // partial gradients of all the other elements are live in registers)
                const T tot = tiny_wsum<T>(G[k][j][i]);
                gr[m.woff[k] + j * din + i] = tot;
              }
            if (m.boff[k] >= 0) {
              const T tot = tiny_wsum<T>(GB[k][j]);
              gr[m.boff[k] + j] = tot;
            }
          }
      }
    }
  }
  return lik;
}

// log-target (and gradient when GRAD) of the position in `th`; result broadcast to every lane.
// gr receives the gradient of the (tempered) log-target.  lik/prior are the tempered parts.
// the chain's N(0,1) stream for elements 0..P-1 into an LDS array, one block of four per lane and round
template <typename T>
__device__ inline void fill_normals(T* dst, const EyRng& rn, int P) {
  for (int b = threadIdx.x & (WAVE - 1); 4 * b < P; b += WAVE) {
    T o[4];
    ey_rng_normal4<T>(rn, (uint32_t)b, o);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * b + j < P) dst[4 * b + j] = o[j];
  }
  __syncthreads();
}

// ------------------------------------------------------------------ Gaussian-mixture target (EY_KIND_MIX)
// The densities of the reference's distribution examples (eeyore/models/distribution_model.py:20-28 with a closure that is
// a multivariate normal or a mixture of them), in closed form:
//   d_k = theta - mu_k,  v_k = Lambda_k d_k,  a_k = c_k - q_k / 2 with q_k = d_k . v_k,  A = max_k a_k,  s = sum_k exp(a_k - A)
//   log p = A + log s,   grad log p = -(sum_k exp(a_k - A) v_k) / s
// Tables shared by all chains in global memory: mean [M, P] (m.x), prec [M, P, P] (m.y), c [M] (m.mu); M = m.N.  Lane i
// owns rows i and i + 64 of Lambda_k d_k and reads COLUMN i of the exactly symmetric Lambda_k, so that the 64 lanes read
// consecutive addresses; d_k is broadcast from LDS.  The scratch (the act region, sized by ey_generic_mix_scratch) keeps the
// M vectors v_k for the gradient pass, d_k, a_k and exp(a_k - A).  M = 1 takes no exp / log: value a_0, gradient -v_0.  The
// maximum propagates a NaN (fmax would drop it), and a_k = -inf for every k gives exp(NaN): a NaN target either way.
template <typename T, bool GRAD>
__device__ T mix_target(const EyModel& m, const Lds<T>& l, const T* th, T* gr, bool has_temp, T temp, T* lik_out,
                        T* prior_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int P = m.P, M = m.N;
  const T* mean = static_cast<const T*>(m.x);
  const T* prec = static_cast<const T*>(m.y);
  const T* cc = static_cast<const T*>(m.mu);
  T* v = l.act;       // [M][P]
  T* dd = v + M * P;  // [P]
  T* aa = dd + P;     // [M]
  T* ee = aa + M;     // [M]
  for (int k = 0; k < M; ++k) {
    const T* mu = mean + (size_t)k * P;
    const T* Lk = prec + (size_t)k * P * P;
    __syncthreads();  // the position written by the caller is visible; the previous component's reads of dd are done
    EY_LANE_PASS(P, i, on) {
      (void)on;
      dd[i] = th[i] - mu[i];
    }
    __syncthreads();
    T q = T(0);
    EY_LANE_PASS(P, i, on) {
      const T* col = Lk + i;
      T acc = T(0);
#pragma unroll 4
      for (int j = 0; j < P; ++j) acc += col[(size_t)j * P] * dd[j];
      v[k * P + i] = acc;
      q += (on ? dd[i] : T(0)) * acc;
    }
    q = wave_sum(q);
    aa[k] = cc[k] - T(0.5) * q;  // (wave-uniform: every lane stores it)
  }
  __syncthreads();
  T val;
  if (M == 1) {
    val = aa[0];
    if (GRAD) {
      EY_LANE_PASS(P, i, on) {
        (void)on;
        const T g = -v[i];
        gr[i] = has_temp ? g * temp : g;
      }
    }
  } else {
    T A = aa[0];
    for (int k = 1; k < M; ++k) {
      const T a = aa[k];
      A = (a > A || a != a) ? a : A;
    }
    T s = T(0);
    for (int k = 0; k < M; ++k) {
      const T e = Num<T>::exp(aa[k] - A);
      ee[k] = e;  // (wave-uniform)
      s += e;
    }
    val = A + Num<T>::log(s);
    if (GRAD) {
      __syncthreads();
      EY_LANE_PASS(P, i, on) {
        (void)on;
        T g = T(0);
        for (int k = 0; k < M; ++k) g += ee[k] * v[k * P + i];
        g = -(g / s);
        gr[i] = has_temp ? g * temp : g;
      }
    }
  }
  if (has_temp) val *= temp;
  if (lik_out) *lik_out = val;
  if (prior_out) *prior_out = T(0);
  __syncthreads();
  return val;
}
// the scratch of mix_target in units of the carve: hrows rows of TS elements, no delta ping-pong
#if EY_GEN_PART == 0
void ey_generic_mix_scratch(EyModel& m) {
  m.hrows = (m.N * m.P + m.P + 2 * m.N + TS - 1) / TS;
  m.dmax = 0;
}
#endif

// ------------------------------------------------------------------ exponential-tilt target (EY_KIND_TILT)
// The reference's Gamma examples sample theta = log x with the Jacobian in the closure; that density and its
// relatives (inverse Gamma, Weibull, Gumbel) are one separable family,
//   log p = sum_i [ c_i + a_i theta_i - b_i exp(s_i theta_i) ],   d/dtheta_i = a_i - b_i s_i exp(s_i theta_i)
// Tables shared by all chains in global memory: c (m.x), a (m.y), b (m.mu), s (m.inv_var), [P] each; lane i owns coordinates
// i and i + 64 and reads consecutive addresses.  No scratch.  Nothing is clamped: an overflowing exp gives b e = +inf (b > 0),
// hence a -inf term and value and a gradient component of -sign(s) inf -- never inf - inf, since a theta stays finite; an
// underflowing one gives b e s = 0 and the component a exactly; a NaN coordinate gives a NaN value and component.
template <typename T, bool GRAD>
__device__ T tilt_target(const EyModel& m, const Lds<T>& l, const T* th, T* gr, bool has_temp, T temp, T* lik_out,
                         T* prior_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const T* cc = static_cast<const T*>(m.x);
  const T* aa = static_cast<const T*>(m.y);
  const T* bb = static_cast<const T*>(m.mu);
  const T* ss = static_cast<const T*>(m.inv_var);
  (void)l;
  __syncthreads();  // the position written by the caller is visible
  T val = T(0);
  EY_LANE_PASS(m.P, i, on) {
    const T t = th[i], a = aa[i], s = ss[i];
    const T be = bb[i] * Num<T>::exp(s * t);
    const T term = cc[i] + a * t - be;
    val += on ? term : T(0);
    if (GRAD) {
      const T g = a - be * s;
      gr[i] = has_temp ? g * temp : g;
    }
  }
  val = wave_sum(val);
  if (has_temp) val *= temp;
  if (lik_out) *lik_out = val;
  if (prior_out) *prior_out = T(0);
  __syncthreads();
  return val;
}
// ... which has no scratch: no activation rows, no delta ping-pong
#if EY_GEN_PART == 0
void ey_generic_tilt_scratch(EyModel& m) {
  m.hrows = 0;
  m.dmax = 0;
}
#endif

template <typename T, bool GRAD, class TINY = TinyOff>
__device__ T eval_target(const EyModel& m, const Lds<T>& l, const T* th, T* gr, bool has_temp, T temp, T* lik_out,
                         T* prior_out, T* row_out = nullptr, const RowWaves rw = RowWaves{0, 1, nullptr},
                         T* fwd_out = nullptr) {
  if constexpr (std::is_same<TINY, TargetMix>::value)
    return mix_target<T, GRAD>(m, l, th, gr, has_temp, temp, lik_out, prior_out);
  if constexpr (std::is_same<TINY, TargetTilt>::value)
    return tilt_target<T, GRAD>(m, l, th, gr, has_temp, temp, lik_out, prior_out);
  const int lane = threadIdx.x & (WAVE - 1);
  const T* x = static_cast<const T*>(m.x);
  const T* y = static_cast<const T*>(m.y);
  const int nl = m.nl;
  const int dK = m.dims[nl];
  T lik = T(0);
  if constexpr (TINY::on) {
    __syncthreads();  // the position written by the caller is visible
    lik = tiny_rows<T, GRAD, TINY>(m, th, gr, has_temp, temp, row_out, rw, fwd_out);
  } else {
  if (GRAD) {
    for (int i = lane; i < m.P; i += WAVE) gr[i] = T(0);
  }
  for (int n0 = 0; n0 < m.N; n0 += WAVE) {
    const int rows = min(WAVE, m.N - n0);
    const int n = n0 + lane;
    const bool valid = lane < rows;
    __syncthreads();  // previous tile's parameter-parallel reads are done; th/gr initialisation visible
    for (int i = 0; i < m.dims[0]; ++i) l.act[(m.hoff[0] + i) * TS + lane] = valid ? x[(size_t)n * m.dims[0] + i] : T(0);
    // ---- forward, row-parallel (mlp.py:45-50)
    for (int k = 0; k < nl; ++k) {
      const int din = m.dims[k], dout = m.dims[k + 1];
      const T* W = th + m.woff[k];
      const T* hin = l.act + m.hoff[k] * TS + lane;
      T* hout = l.act + m.hoff[k + 1] * TS + lane;
      // four outputs at a time: one read of the row's input feeds four sums and nothing is stored inside the i loop,
      // so its loads pipeline (one output at a time every load waited behind the previous output's store); each sum
      // still adds its terms in the order i = 0, 1, ..., so the results are those of the plain loop, bit for bit
      for (int j0 = 0; j0 < dout; j0 += 4) {
        const int nj = min(4, dout - j0);
        const T* w0 = W + j0 * din;
        const T* w1 = w0 + (nj > 1 ? din : 0);  // rows beyond dout alias row j0: read, never stored
        const T* w2 = w0 + (nj > 2 ? 2 * din : 0);
        const T* w3 = w0 + (nj > 3 ? 3 * din : 0);
        T g0 = T(0), g1 = T(0), g2 = T(0), g3 = T(0);
#pragma unroll 4
        for (int i = 0; i < din; ++i) {
          const T h = hin[i * TS];
          g0 += h * w0[i];
          g1 += h * w1[i];
          g2 += h * w2[i];
          g3 += h * w3[i];
        }
        auto put = [&](int q, T g) {
          if (q < nj) {
            if (m.boff[k] >= 0) g += th[m.boff[k] + j0 + q];
            hout[(j0 + q) * TS] = act_fn<T>(m.act[k], g);
          }
        };
        put(0, g0); put(1, g1); put(2, g2); put(3, g3);
      }
    }
    // ---- likelihood and output delta
    const T* out = l.act + m.hoff[nl] * TS + lane;
    T* dcur = l.dl;
    T* dnext = l.dl + m.dmax * TS;
    T row_lik = T(0);  // this row's term of the log-likelihood sum (ey_log_lik_rows)
    if (fwd_out && valid) {  // ey_forward: the row's outputs, next to row_out below
      for (int j = 0; j < dK; ++j) fwd_out[(size_t)n * dK + j] = out[j * TS];
    }
    if (m.lik >= EY_LIK_GAUSS_SUM) {
      // regression (include/eeyore_amd.h: enum ey_lik), the arithmetic of tiny_rows: a scalar branch on the kernel argument
      const T lw = T(m.lik_w), lc = T(m.lik_c);
      for (int j = 0; j < dK; ++j) {
        const T o = out[j * TS];
        const T yy = valid ? y[(size_t)n * dK + j] : T(0);
        EY_REG_TERM(m.lik, o, yy, lw, lc, term, d);
        if (valid) lik += term;
        row_lik += term;
        if (GRAD) dcur[j * TS + lane] = valid ? d * dact_fn<T>(m.act[nl - 1], o) : T(0);
      }
    } else
    if (m.lik == EY_LIK_BCE_SUM) {
      for (int j = 0; j < dK; ++j) {
        const T o = out[j * TS];
        const T yy = valid ? y[(size_t)n * dK + j] : T(0);
        // naive logs exactly as eeyore/stats/loss.py:2 (NaN once a sigmoid saturates)
        const T term = EY_BCE_TERM(o, yy);
        if (valid) lik += term;
        row_lik += term;
        if (GRAD) {
          const T d = EY_BCE_DOUT(o, yy) * dact_fn<T>(m.act[nl - 1], o);
          dcur[j * TS + lane] = valid ? d : T(0);
        }
      }
    } else {
      const int lab = valid ? m.labels[n] : 0;
      T mx = out[0];
      for (int j = 1; j < dK; ++j) mx = fmax(mx, out[j * TS]);
      T ssum = T(0);
      for (int j = 0; j < dK; ++j) ssum += Num<T>::exp(out[j * TS] - mx);
      row_lik = out[lab * TS] - (mx + Num<T>::log(ssum));
      if (valid) lik += row_lik;
      if (GRAD) {
        for (int j = 0; j < dK; ++j) {
          const T o = out[j * TS];
          const T d = ((j == lab ? T(1) : T(0)) - Num<T>::exp(o - mx) / ssum) * dact_fn<T>(m.act[nl - 1], o);
          dcur[j * TS + lane] = valid ? d : T(0);
        }
      }
    }
    if (row_out && valid) row_out[n] = has_temp ? row_lik * temp : row_lik;
    if (GRAD) {
      // ---- backward
      for (int k = nl - 1; k >= 0; --k) {
        const int din = m.dims[k], dout = m.dims[k + 1];
        __syncthreads();  // delta_k of every row visible
        // dW_k[j][i] += sum_n delta[j][n] * h_{k}[i][n]   (parameter-parallel)
        const T* hin_t = l.act + m.hoff[k] * TS;
        for (int idx = lane; idx < dout * din; idx += WAVE) {
          const int j = idx / din, i = idx - j * din;
          const T* dj = dcur + j * TS;
          const T* hi = hin_t + i * TS;
          T acc = T(0);
          // few lanes are active when a layer is small: keep several LDS reads in flight per lane
#pragma unroll 8
          for (int r = 0; r < rows; ++r) acc += dj[r] * hi[r];
          gr[m.woff[k] + idx] += acc;
        }
        if (m.boff[k] >= 0) {
          for (int j = lane; j < dout; j += WAVE) {
            const T* dj = dcur + j * TS;
            T acc = T(0);
#pragma unroll 8
            for (int r = 0; r < rows; ++r) acc += dj[r];
            gr[m.boff[k] + j] += acc;
          }
        }
        if (k > 0) {
          // delta_{k-1}[i][n] = (sum_j delta_k[j][n] W_k[j][i]) * act'(h_k[i][n])   (row-parallel)
          const T* W = th + m.woff[k];
          for (int i0 = 0; i0 < din; i0 += 4) {  // four inputs at a time, each sum in the order j = 0, 1, ...
            const int ni = min(4, din - i0);
            const int o1 = ni > 1 ? 1 : 0, o2 = ni > 2 ? 2 : 0, o3 = ni > 3 ? 3 : 0;
            T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
#pragma unroll 4
            for (int j = 0; j < dout; ++j) {
              const T d = dcur[j * TS + lane];
              const T* w = W + j * din + i0;
              a0 += d * w[0];
              a1 += d * w[o1];
              a2 += d * w[o2];
              a3 += d * w[o3];
            }
            auto put = [&](int q, T a) {
              if (q < ni) dnext[(i0 + q) * TS + lane] = a * dact_fn<T>(m.act[k - 1], hin_t[(i0 + q) * TS + lane]);
            };
            put(0, a0); put(1, a1); put(2, a2); put(3, a3);
          }
          T* t = dcur; dcur = dnext; dnext = t;
        }
      }
    }
  }
  }  // !TINY
  __syncthreads();
  lik = wave_sum(lik);
  // ---- prior (bayesian_model.py:46-50), elementwise Normal(mu, sigma), or Laplace / Student-t (ey_plan_set_prior_family)
  const T* mu = static_cast<const T*>(m.mu);
  const T* iv = static_cast<const T*>(m.inv_var);
  T q = T(0);
  // m.prior_kind is a kernel argument: the branch is scalar, one family's loop runs and every lane of the wave runs it
  if (m.prior_kind == EY_PRIOR_LAPLACE) {
    // -|d| / b per parameter (iv holds 1/b); the derivative of |d| is sign(d) with sign(0) = 0, what autograd gives at the kink
    EY_LANE_PASS(m.P, i, on) {
      const T d = th[i] - mu[i];
      const T dz = on ? d : T(0);
      q += Num<T>::abs(dz) * iv[i];
      if (GRAD) {
        const T sg = d > T(0) ? T(1) : (d < T(0) ? T(-1) : T(0));
        T g = gr[i] - sg * iv[i];
        if (has_temp) g *= temp;
        gr[i] = g;
      }
    }
  } else if (m.prior_kind == EY_PRIOR_STUDENT_T) {
    // -h log1p(d^2 w) per parameter (iv holds w = 1/(nu s^2), hh holds h = (nu+1)/2); Cauchy is nu = 1
    const T* hh = static_cast<const T*>(m.prior_h);
    EY_LANE_PASS(m.P, i, on) {
      const T d = th[i] - mu[i];
      const T dz = on ? d : T(0);
      q += hh[i] * Num<T>::log1p(dz * dz * iv[i]);
      if (GRAD) {
        T g = gr[i] - T(2) * hh[i] * d * iv[i] / (T(1) + d * d * iv[i]);
        if (has_temp) g *= temp;
        gr[i] = g;
      }
    }
  } else
  // (EY_LANE_PASS: the same trip count in every lane -- a sum carried across a loop whose last round runs under a partial
  // EXEC mask is what the fast-allocator build of this unit got wrong)
  EY_LANE_PASS(m.P, i, on) {
    const T d = th[i] - mu[i];
    const T dz = on ? d : T(0);
    q += dz * dz * iv[i];
    if (GRAD) {
      T g = gr[i] - d * iv[i];
      if (has_temp) g *= temp;
      gr[i] = g;
    }
  }
  q = wave_sum(q);
  T prior = T(m.prior_const) - T(0.5) * q;
  if (m.prior_kind != EY_PRIOR_NORMAL) prior = T(m.prior_const) - q;
  if (has_temp) { lik *= temp; prior *= temp; }
  if (lik_out) *lik_out = lik;
  if (prior_out) *prior_out = prior;
  __syncthreads();
  return lik + prior;
}

// ----------------------------------------------------------------------------------------------- steps the kernels share
// Each is written once and expanded where a kernel takes it; what a kernel does differently it passes in.
// Beside its arguments a macro reads names that every kernel using it gives its template parameters, arguments and
// locals; each macro's comment lists the names it reads.  Those that are statements are used with a semicolon.

// How a row-wave kernel starts: the wave's place among the chain's waves (rw) and its own LDS image of nvec [P] vectors (l).
// RW false: one wave, all of this folds away.  Wave 0 is the wave that writes to global memory (ROW WAVES).
// DECLARES smem, rw and l for the kernel.  Reads: T, RW, m.
#define EY_WAVE_IMAGE(nvec)                                                                             \
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];                                  \
  const RowWaves rw = RW ? row_waves<T>(m, smem, nvec) : RowWaves{0, 1, nullptr};                       \
  const Lds<T> l = carve<T>(m, smem + (RW ? (size_t)rw.wave * lds_bytes(m, nvec, sizeof(T)) : 0), nvec)

// The leapfrog trajectory (hmc.py:100-124) from the gradient in l.gr: half a momentum step, L position steps with an
// evaluation each (its value left in t), the last momentum step halved; grad_potential = -grad.
// Reads: T, TINY, m, l, rw, lane, P, p (the momentum, in LDS), eps, L, ht, tc.
#define EY_LEAPFROG(t)                                                                         \
  do {                                                                                         \
    for (int i = lane; i < P; i += WAVE) p[i] = p[i] + T(0.5) * eps * l.gr[i];                 \
    for (int k = 1; k <= L; ++k) {                                                             \
      for (int i = lane; i < P; i += WAVE) l.th[i] = l.th[i] + eps * p[i];                     \
      t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr, nullptr, rw); \
      const T w = (k < L) ? eps : T(0.5) * eps;                                                \
      for (int i = lane; i < P; i += WAVE) p[i] = p[i] + w * l.gr[i];                          \
    }                                                                                          \
  } while (0)

// What a draw leaves behind.  By the wave that writes (`on`): the recorded sample `value` of element i, the state the chain
// is left in (what ChainList.update stores, chain_list.py:64-67) ...  Reads: T, run, it, C, c, P, lane.
#define EY_RECORD_SAMPLE(on, i, value)                                  \
  do {                                                                  \
    if (run.samples && (on)) {                                          \
      T* so = static_cast<T*>(run.samples) + ((int64_t)it * C + c) * P; \
      for (int i = lane; i < P; i += WAVE) so[i] = (value);             \
    }                                                                   \
  } while (0)
// ... and by its lane 0 (`on`): the state's target, the accept flag, the log-rate and the run's records.  (A
// function: this one the compiler inlines without a trace.)
template <typename T>
__device__ __forceinline__ void record_draw(bool on, int64_t c, int it, int64_t C, bool acc, T tv, T t_state, T log_rate,
                                            T* target, unsigned char* accepted, T* log_rate_o, const EyRun& run) {
  if (on) {
    if (acc) target[c] = tv;
    accepted[c] = acc ? 1 : 0;
    if (log_rate_o) log_rate_o[c] = log_rate;
    if (run.targets) static_cast<T*>(run.targets)[(int64_t)it * C + c] = t_state;
    if (run.accepted) static_cast<unsigned char*>(run.accepted)[(int64_t)it * C + c] = acc ? 1 : 0;
    if (run.accept_count && acc) run.accept_count[c] += 1;
  }
}

// ----------------------------------------------------------------------------------------------- kernels
template <typename T, bool GRAD, class TINY, bool RW = false>
__global__ void __launch_bounds__(RW ? RW_MAX * WAVE : WAVE) k_log_target(EyModel m, const T* theta, const T* temp, T* lik_o, T* prior_o,
                                                     T* target_o, T* grad_o, T* rows_o) {
  EY_WAVE_IMAGE(2);
  const bool w0 = rw.wave == 0;  // the wave that writes to global memory (ROW WAVES)
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (int i = lane; i < m.P; i += WAVE) l.th[i] = theta[c * m.P + i];
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T lik, prior;
  const T t = eval_target<T, GRAD, TINY>(m, l, l.th, l.gr, ht, tc, &lik, &prior, rows_o ? rows_o + c * m.N : nullptr, rw);
  if (lane == 0 && w0) {
    if (lik_o) lik_o[c] = lik;
    if (prior_o) prior_o[c] = prior;
    if (target_o) target_o[c] = t;
  }
  if (GRAD && w0) {
    for (int i = lane; i < m.P; i += WAVE) grad_o[c * m.P + i] = l.gr[i];
  }
}

// ey_forward: the network outputs of every chain, out [C, N, dK].  A kernel of its own, so that k_log_target stays the code it
// was (its values are held bit-equal to the targets the sampling kernels carry); the value, the prior and the gradient the
// evaluation also works out are dropped.
template <typename T, class TINY, bool RW = false>
__global__ void __launch_bounds__(RW ? RW_MAX * WAVE : WAVE) k_forward(EyModel m, const T* theta, T* out) {
  EY_WAVE_IMAGE(2);
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (int i = lane; i < m.P; i += WAVE) l.th[i] = theta[c * m.P + i];
  eval_target<T, false, TINY>(m, l, l.th, l.gr, false, T(1), nullptr, nullptr, nullptr, rw, out + c * m.N * m.dims[m.nl]);
}

// k_hmc takes an EyRun's fields as five arguments of its own and keeps its own record of a draw (EY_RECORD_SAMPLE and
// record_draw read an EyRun): handing it the struct changes the instructions of every one of its instantiations, and
// k_hmc<double, TinyDyn> sits at 512 registers with scratch.
template <typename T, class TINY, bool RW = false>
__global__ void __launch_bounds__(RW ? RW_MAX * WAVE : WAVE) k_hmc(EyModel m, T* theta, T* target, T* grad, const T* p0, const T* u_in,
                                              T step, const T* step_vec, int L, const T* temp, uint64_t seed,
                                              uint64_t iter0, uint64_t chain_offset, int recompute,
                                              unsigned char* accepted, T* rate_o, T* hcur_o, T* hprop_o, int n_iters,
                                              T* rec_samples, T* rec_targets, unsigned char* rec_accepted,
                                              int* accept_count, int64_t C) {
  EY_WAVE_IMAGE(3);
  const bool w0 = rw.wave == 0;  // the wave that writes to global memory (ROW WAVES)
  const int64_t c = blockIdx.x;
  const int lane = RW ? (threadIdx.x & (WAVE - 1)) : threadIdx.x;
  const int P = m.P;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  const T eps = step_vec ? step_vec[c] : step;
  T* p = l.a;
  T t_state = target[c];
  // ey_hmc_run: n_iters draws in one launch; every lane re-reads only what it wrote itself (theta, grad), the
  // log-target is carried in a register
  for (int it = 0; it < n_iters; ++it) {
  const uint64_t iter = iter0 + (uint64_t)it;
  // momentum ~ N(0, I)  (hmc.py:134)
  const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
  T kin = T(0);
  if (!p0) fill_normals<T>(p, rn, P);
  EY_LANE_PASS(P, i, on) {
    l.th[i] = theta[c * P + i];
    l.gr[i] = grad[c * P + i];
    const T pi = p0 ? p0[c * P + i] : p[i];
    p[i] = pi;
    const T pz = on ? pi : T(0);
    kin += pz * pz;
  }
  kin = wave_sum(kin);
  const T t_cur = t_state;
  const T h_cur = -t_cur + T(0.5) * kin;  // hmc.py:91-98,137
  __syncthreads();
  T t = t_cur;
  if (recompute) t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr, nullptr, rw);  // hmc.py:104
  EY_LEAPFROG(t);
  kin = T(0);
  EY_LANE_PASS(P, i, on) {  // p -> -p leaves it unchanged (hmc.py:122)
    const T pz = on ? p[i] : T(0);
    kin += pz * pz;
  }
  kin = wave_sum(kin);
  const T h_prop = -t + T(0.5) * kin;
  T rate = Num<T>::exp(h_cur - h_prop);  // hmc.py:143-146
  if (rate > T(1)) rate = T(1);
  const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
  const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
  const bool acc = u < rate;  // strict <; NaN rate => reject (hmc.py:148)
  if (acc && w0) {
    for (int i = lane; i < P; i += WAVE) {
      theta[c * P + i] = l.th[i];
      grad[c * P + i] = l.gr[i];
    }
  }
  if (acc) t_state = t;
  if (rec_samples && w0) {  // the state the chain is left in (what ChainList.update stores, chain_list.py:64-67)
    T* so = rec_samples + ((int64_t)it * C + c) * P;
    for (int i = lane; i < P; i += WAVE) so[i] = acc ? l.th[i] : theta[c * P + i];
  }
  if (lane == 0 && w0) {
    if (acc) target[c] = t;
    accepted[c] = acc ? 1 : 0;
    if (rate_o) rate_o[c] = rate;
    if (hcur_o) hcur_o[c] = h_cur;
    if (hprop_o) hprop_o[c] = h_prop;
    if (rec_targets) rec_targets[(int64_t)it * C + c] = t_state;
    if (rec_accepted) rec_accepted[(int64_t)it * C + c] = acc ? 1 : 0;
    if (accept_count && acc) accept_count[c] += 1;
  }
  __syncthreads();
  }
}

// HMC.leapfrog as a standalone operator (hmc.py:100-124): L+1 evaluations, momentum negated.
template <typename T, class TINY, bool RW = false>
__global__ void __launch_bounds__(RW ? RW_MAX * WAVE : WAVE) k_leapfrog(EyModel m, T* theta, T* pio, T step, const T* step_vec, int L,
                                                   const T* temp, T* target, T* grad) {
  EY_WAVE_IMAGE(3);
  const bool w0 = rw.wave == 0;  // the wave that writes to global memory (ROW WAVES)
  const int64_t c = blockIdx.x;
  const int lane = RW ? (threadIdx.x & (WAVE - 1)) : threadIdx.x;
  const int P = m.P;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  const T eps = step_vec ? step_vec[c] : step;
  T* p = l.a;
  for (int i = lane; i < P; i += WAVE) {
    l.th[i] = theta[c * P + i];
    p[i] = pio[c * P + i];
  }
  __syncthreads();
  T t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr, nullptr, rw);
  EY_LEAPFROG(t);
  if (w0) {
    for (int i = lane; i < P; i += WAVE) {
      theta[c * P + i] = l.th[i];
      pio[c * P + i] = -p[i];
      grad[c * P + i] = l.gr[i];
    }
    if (lane == 0) target[c] = t;
  }
}

template <typename T, class TINY, bool RW = false>
__global__ void __launch_bounds__(RW ? RW_MAX * WAVE : WAVE) k_mala(EyModel m, T* theta, T* target, T* grad, const T* z_in, const T* u_in,
                                               T step, T sqrt_step, const T* step_vec, const T* temp, uint64_t seed,
                                               uint64_t iter0, uint64_t chain_offset, unsigned char* accepted,
                                               T* log_rate_o, EyRun run, int64_t C) {
  EY_WAVE_IMAGE(4);
  const bool w0 = rw.wave == 0;  // the wave that writes to global memory (ROW WAVES)
  const int64_t c = blockIdx.x;
  const int lane = RW ? (threadIdx.x & (WAVE - 1)) : threadIdx.x;
  const int P = m.P;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  const T eps = step_vec ? step_vec[c] : step;
  const T sc = step_vec ? Num<T>::sqrt(eps) : sqrt_step;  // scale = sqrt(step) (mala.py:39)
  const T inv2v = T(1) / (T(2) * sc * sc);
  T* prop = l.a;
  T* gp = l.b;
  T t_state = target[c];
  // ey_mala_run: n_iters draws in one launch; every lane re-reads only what it wrote itself (theta, grad), the
  // log-target is carried in a register
  for (int it = 0; it < run.n_iters; ++it) {
  const uint64_t iter = iter0 + (uint64_t)it;
  const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
  T qf = T(0);
  if (!z_in) fill_normals<T>(prop, rn, P);
  EY_LANE_PASS(P, i, on) {
    const T th = theta[c * P + i], g = grad[c * P + i];
    l.th[i] = th;
    l.gr[i] = g;
    const T zi = z_in ? z_in[c * P + i] : prop[i];
    const T loc = th + T(0.5) * eps * g;  // kernel_mean (mala.py:35-36)
    const T pr = loc + sc * zi;           // Normal(loc, scale).sample()
    prop[i] = pr;
    const T d = on ? pr - loc : T(0);
    qf += d * d;
  }
  __syncthreads();
  const T tv = eval_target<T, true, TINY>(m, l, prop, gp, ht, tc, nullptr, nullptr, nullptr, rw);
  T qb = T(0);
  EY_LANE_PASS(P, i, on) {
    const T loc2 = prop[i] + T(0.5) * eps * gp[i];
    const T d = on ? l.th[i] - loc2 : T(0);
    qb += d * d;
  }
  qf = wave_sum(qf);
  qb = wave_sum(qb);
  // log q terms share -P log(scale) - P/2 log(2 pi): they cancel in log_rate (mala.py:58-64)
  const T log_rate = (tv - t_state) + qf * inv2v - qb * inv2v;
  const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
  const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
  const bool acc = Num<T>::log(u) < log_rate;  // mala.py:66
  if (acc) {
    t_state = tv;
    if (w0)
      for (int i = lane; i < P; i += WAVE) {
        theta[c * P + i] = prop[i];
        grad[c * P + i] = gp[i];
      }
  }
  EY_RECORD_SAMPLE(w0, i, acc ? prop[i] : l.th[i]);
  record_draw<T>(lane == 0 && w0, c, it, C, acc, tv, t_state, log_rate, target, accepted, log_rate_o, run);
  __syncthreads();
  }
}

template <typename T, class TINY, bool RW = false>
__global__ void __launch_bounds__(RW ? RW_MAX * WAVE : WAVE) k_mh(EyModel m, T* theta, T* target, const T* z_in, const T* u_in,
                                             const T* scale, const T* temp, uint64_t seed, uint64_t iter0,
                                             uint64_t chain_offset, unsigned char* accepted, T* log_rate_o, EyRun run,
                                             int64_t C) {
  EY_WAVE_IMAGE(2);
  const bool w0 = rw.wave == 0;  // the wave that writes to global memory (ROW WAVES)
  const int64_t c = blockIdx.x;
  const int lane = RW ? (threadIdx.x & (WAVE - 1)) : threadIdx.x;
  const int P = m.P;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {  // ey_mh_run: see k_mala
  const uint64_t iter = iter0 + (uint64_t)it;
  const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
  if (!z_in) fill_normals<T>(l.th, rn, P);
  for (int i = lane; i < P; i += WAVE) {
    const T zi = z_in ? z_in[c * P + i] : l.th[i];
    l.th[i] = theta[c * P + i] + scale[i] * zi;  // NormalKernel(theta, scale).sample()
  }
  __syncthreads();
  const T tv = eval_target<T, false, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr, nullptr, rw);
  const T log_rate = tv - t_state;  // symmetric kernel (metropolis_hastings.py:50)
  const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
  const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
  const bool acc = Num<T>::log(u) < log_rate;  // :56
  if (acc) {
    t_state = tv;
    if (w0)
      for (int i = lane; i < P; i += WAVE) theta[c * P + i] = l.th[i];
  }
  EY_RECORD_SAMPLE(w0, i, acc ? l.th[i] : theta[c * P + i]);
  record_draw<T>(lane == 0 && w0, c, it, C, acc, tv, t_state, log_rate, target, accepted, log_rate_o, run);
  __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------- host launchers

// Where the register-resident evaluation pays (tools/tiny_scan.py, profiles/r02_tiny_scan.txt): it has a fixed cost per
// evaluation (the register copies of the position, one wave reduction per parameter), so it is taken from two 64-row
// tiles up: 1.6-2.8 x the LDS loop at a few hundred chains, where that loop's dependent round trips are exposed, 1.1-1.7 x
// in f32 when the chains fill the chip; in f64 (one wave per SIMD) a chip full of chains is 0.75-1.1 x.  The rule looks
// at the batch only, not at the number of chains: the arithmetic a chain sees must not depend on how many chains (or
// GPUs) run beside it.  ey_debug_set_variant bit 8: never (A/B, tests), bit 9: whenever the model qualifies.
// 0: the LDS tile loop, 1: TinyDyn, 2..: the compile-time shapes (taken for any batch: their fixed cost is a handful of
// loads and reductions)
static int tiny_kind(const ey_plan* pl) {
  const EyModel& m = pl->m;
  if (!ey_generic_tiny_ok(m) || EY_VBIT(8)) return 0;
  auto is = [&](int nl, int a, int b, int c, int d) {
    return m.nl == nl && m.dims[0] == a && m.dims[1] == b && (nl < 2 || m.dims[2] == c) && (nl < 3 || m.dims[3] == d);
  };
  if (is(2, 2, 2, 1, 0)) return 2;
  if (is(3, 2, 3, 2, 1)) return 3;
  if (is(2, 4, 3, 3, 0)) return 4;
  if (is(3, 4, 3, 2, 3)) return 5;
  if (is(2, 1, 2, 1, 0)) return 6;
  if (is(3, 2, 3, 3, 2)) return 7;
  if (is(1, 4, 1, 0, 0)) return 8;
  return (EY_VBIT(9) || m.N >= 128) ? 1 : 0;
}
template <typename F>
static int tiny_dispatch_mlp(const ey_plan* pl, F f) {
  switch (tiny_kind(pl)) {
    case 1: return f(TinyDyn{});
    case 2: return f(TinyFix<2, 2, 2, 1, 0>{});
    case 3: return f(TinyFix<3, 2, 3, 2, 1>{});
    case 4: return f(TinyFix<2, 4, 3, 3, 0>{});
    case 5: return f(TinyFix<3, 4, 3, 2, 3>{});
    case 6: return f(TinyFix<2, 1, 2, 1, 0>{});
    case 7: return f(TinyFix<3, 2, 3, 3, 2>{});
    case 8: return f(TinyFix<1, 4, 1, 0, 0>{});
    default: return f(TinyOff{});
  }
}
// ... and TargetMix for a mixture plan, TargetTilt for an exponential-tilt plan, in every kernel but k_gibbs (the reference's
// Gibbs needs MLP node blocks)
template <typename F>
static int tiny_dispatch(const ey_plan* pl, F f) {
  if (pl->m.kind == EY_KIND_MIX) return f(TargetMix{});
  if (pl->m.kind == EY_KIND_TILT) return f(TargetTilt{});
  return tiny_dispatch_mlp(pl, f);
}
// fn<T, policy>(...) for the plan's dtype and the policy `dispatch` (tiny_dispatch or tiny_dispatch_mlp) picks
#define EY_TINY_DISPATCH(dispatch, fn, ...)                                                            \
  dispatch(pl, [&](auto tiny_tag) {                                                                    \
    typedef decltype(tiny_tag) TinyS;                                                                  \
    return pl->dtype == EY_F32 ? fn<float, TinyS>(__VA_ARGS__) : fn<double, TinyS>(__VA_ARGS__);       \
  })

template <typename K>
static int prep(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) EY_FAIL(EY_ERR_UNSUPPORTED, "generic kernel: model does not fit the 160 KiB LDS of a CU");
  if (bytes > 48 * 1024)
    EY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes));
  return EY_OK;
}

// one draw, nothing recorded: the run of a caller that passes none
static const EyRun kOneDraw = {1, nullptr, nullptr, nullptr, nullptr};
// the arguments every sampler kernel but k_hmc ends with, from the draw d: temp, the Philox key, accepted, log_rate, run, C
#define EY_DRAW_ARGS(T, d)                                                                                      \
  (const T*)(d).temp, (d).seed, (d).iter, (d).chain_offset, (unsigned char*)(d).accepted, (T*)(d).log_rate, \
      (d).run ? *(d).run : kOneDraw, (d).C

// one kernel over C chains of nw waves: the LDS attribute, the launch, its error
template <typename... Ps, typename... As>
static int launch(void (*kernel)(Ps...), int64_t C, int nw, size_t bytes, hipStream_t s, As... args) {
  int rc;
  if ((rc = prep(kernel, bytes))) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)C), dim3(nw * WAVE), bytes, s, args...);
  EY_HIP(hipGetLastError());
  return EY_OK;
}
// ... of a row-wave kernel with an image of nvec vectors: its row-waves instantiation (RW) where the launch uses several
// waves per chain, the lean one otherwise.  kernel_of(std::bool_constant<RW>) names the instantiation (EY_RW_KERNEL).
template <typename T, class TINY, typename KF, typename... As>
static int launch_row_waves(ey_plan* pl, int nvec, int64_t C, hipStream_t s, KF kernel_of, As... args) {
  const int nw = row_waves_for(pl, TINY::on, C);
  const size_t bytes = lds_total(pl->m, nvec, sizeof(T), nw);
  if constexpr (TINY::on) {
    if (nw > 1) return launch(kernel_of(std::true_type{}), C, nw, bytes, s, args...);
  }
  return launch(kernel_of(std::false_type{}), C, nw, bytes, s, args...);
}
#define EY_RW_KERNEL(k, ...) [](auto rw_tag) { return k<__VA_ARGS__, decltype(rw_tag)::value>; }

#if EY_GEN_PART == 0
template <typename T, class TINY>
static int launch_log_target(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* lik, void* prior,
                             void* target, void* grad, hipStream_t s, void* rows = nullptr) {
  if (grad)
    return launch_row_waves<T, TINY>(pl, 2, C, s, EY_RW_KERNEL(k_log_target, T, true, TINY), pl->m, (const T*)theta,
                                     (const T*)temp, (T*)lik, (T*)prior, (T*)target, (T*)grad, (T*)nullptr);
  return launch_row_waves<T, TINY>(pl, 2, C, s, EY_RW_KERNEL(k_log_target, T, false, TINY), pl->m, (const T*)theta,
                                   (const T*)temp, (T*)lik, (T*)prior, (T*)target, (T*)nullptr, (T*)rows);
}

int ey_generic_log_target(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* lik, void* prior,
                          void* target, void* grad, hipStream_t s) {
  return EY_TINY_DISPATCH(tiny_dispatch, launch_log_target, pl, theta, temp, C, lik, prior, target, grad, s);
}

int ey_generic_log_lik_rows(ey_plan* pl, const void* theta, const void* temp, int64_t C, void* rows, hipStream_t s) {
  if (pl->m.kind != EY_KIND_MLP) EY_FAIL(EY_ERR_UNSUPPORTED, "ey_log_lik_rows: this plan has no data rows");
  return EY_TINY_DISPATCH(tiny_dispatch, launch_log_target, pl, theta, temp, C, nullptr, nullptr, nullptr, nullptr, s,
                          rows);
}

template <typename T, class TINY>
static int launch_forward(ey_plan* pl, const void* theta, int64_t C, void* out, hipStream_t s) {
  return launch_row_waves<T, TINY>(pl, 2, C, s, EY_RW_KERNEL(k_forward, T, TINY), pl->m, (const T*)theta, (T*)out);
}
// ey_forward: out [C, N, dK]
int ey_generic_forward(ey_plan* pl, const void* theta, int64_t C, void* out, hipStream_t s) {
  if (pl->m.kind != EY_KIND_MLP) EY_FAIL(EY_ERR_INVALID, "ey_forward: this plan has no network");
  return EY_TINY_DISPATCH(tiny_dispatch_mlp, launch_forward, pl, theta, C, out, s);
}

template <typename T, class TINY>
static int launch_hmc(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                      const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop) {
  const EyRun& run = d.run ? *d.run : kOneDraw;
  return launch_row_waves<T, TINY>(pl, 3, d.C, d.s, EY_RW_KERNEL(k_hmc, T, TINY), pl->m, (T*)theta, (T*)target, (T*)grad,
                                   (const T*)p0, (const T*)u, (T)step, (const T*)step_vec, L, (const T*)d.temp, d.seed,
                                   d.iter, d.chain_offset, (int)((d.flags & EY_RECOMPUTE_INITIAL_GRAD) != 0),
                                   (unsigned char*)d.accepted, (T*)rate, (T*)hcur, (T*)hprop, run.n_iters, (T*)run.samples,
                                   (T*)run.targets, (unsigned char*)run.accepted, run.accept_count, d.C);
}

int ey_generic_hmc(ey_plan* pl, void* theta, void* target, void* grad, const void* p0, const void* u, double step,
                   const void* step_vec, int L, const EyDraw& d, void* rate, void* hcur, void* hprop) {
  return EY_TINY_DISPATCH(tiny_dispatch, launch_hmc, pl, theta, target, grad, p0, u, step, step_vec, L, d, rate, hcur,
                          hprop);
}

template <typename T, class TINY>
static int launch_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                           int64_t C, void* target, void* grad, hipStream_t s) {
  return launch_row_waves<T, TINY>(pl, 3, C, s, EY_RW_KERNEL(k_leapfrog, T, TINY), pl->m, (T*)theta, (T*)p, (T)step,
                                   (const T*)step_vec, L, (const T*)temp, (T*)target, (T*)grad);
}

int ey_generic_leapfrog(ey_plan* pl, void* theta, void* p, double step, const void* step_vec, int L, const void* temp,
                        int64_t C, void* target, void* grad, hipStream_t s) {
  return EY_TINY_DISPATCH(tiny_dispatch, launch_leapfrog, pl, theta, p, step, step_vec, L, temp, C, target, grad, s);
}

template <typename T, class TINY>
static int launch_mala(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                       const void* step_vec, const EyDraw& d) {
  // scale = np.sqrt(step) on the python float, then cast to the model dtype (mala.py:39)
  return launch_row_waves<T, TINY>(pl, 4, d.C, d.s, EY_RW_KERNEL(k_mala, T, TINY), pl->m, (T*)theta, (T*)target, (T*)grad,
                                   (const T*)z, (const T*)u, (T)step, (T)sqrt(step), (const T*)step_vec,
                                   EY_DRAW_ARGS(T, d));
}

int ey_generic_mala(ey_plan* pl, void* theta, void* target, void* grad, const void* z, const void* u, double step,
                    const void* step_vec, const EyDraw& d) {
  return EY_TINY_DISPATCH(tiny_dispatch, launch_mala, pl, theta, target, grad, z, u, step, step_vec, d);
}

template <typename T, class TINY>
static int launch_mh(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
                     const EyDraw& d) {
  return launch_row_waves<T, TINY>(pl, 2, d.C, d.s, EY_RW_KERNEL(k_mh, T, TINY), pl->m, (T*)theta, (T*)target, (const T*)z,
                                   (const T*)u, (const T*)scale, EY_DRAW_ARGS(T, d));
}

int ey_generic_mh(ey_plan* pl, void* theta, void* target, const void* z, const void* u, const void* scale,
                  const EyDraw& d) {
  return EY_TINY_DISPATCH(tiny_dispatch, launch_mh, pl, theta, target, z, u, scale, d);
}
#endif  // EY_GEN_PART == 0

// ----------------------------------------------------------------------------------------------- robust adaptive Metropolis
// RAM.draw (eeyore/samplers/ram.py:38-70; Vihola 2012): propose theta + S z with the chain's lower-triangular factor S,
// accept as MH does, then ALWAYS adapt  S <- chol(S (I + beta w w^T) S^T),  w = z / |z|,  beta = h (alpha - a),
// h = min(1, P n^-g).  The re-factorisation has a closed form S' = S L_w, L_w the Cholesky factor of I + beta w w^T:
//   t_{-1} = 1,  t_k = 1 + beta sum_{j<=k} w_j^2,  d_k = sqrt(t_k / t_{k-1}),  g_k = beta w_k / sqrt(t_{k-1} t_k)
//   S'[i,k] = d_k S[i,k] + g_k sum_{k<j<=i} S[i,j] w_j                                               (i >= k)
// so every row of S' is a backward sweep over its own row of S with one running sum of OLD values; only the per-column
// scalars d_k, g_k are shared.  t_k >= 1 - a > 0 for 0 < a < 1: the update cannot break down.
// One wave per chain, lane <-> row (rows lane and lane + 64: P <= 128).  The factor stays in LDS for the whole launch,
// packed lower triangle, column-major: (i, j) at j P - j (j - 1) / 2 + (i - j) -- both sweeps walk a column at
// consecutive addresses.  Global state: dense [C, P, P] row-major (what torch.linalg.cholesky returns); only j <= i is
// read or written.  No row-wave form: the kernel is one wave per chain whatever plan.row_waves says.
#define RAM_MAX_P 128
__host__ __device__ static inline int ram_col(int j, int P) { return j * P - (j * (j - 1)) / 2; }
__host__ __device__ static size_t ram_extra_bytes(int P, size_t esz) {
  const size_t packed = ((size_t)P * (P + 1) / 2 + 3) & ~(size_t)3, Ppad = (P + 3) & ~3;
  return esz * (packed + 3 * Ppad + WAVE);  // factor, w, d, g, and a slot per lane for the stores of rows above a column
}

// ---- steps the one-wave kernels share (k_ram, k_mh_tril, k_mala_tril, k_am, k_gibbs), macros as the kernels' above
// Lg: chain c's factor in tril [G, P, P], chosen as the comment of k_mh_tril says (G, tril_index, clamped into [0, G)).
// DECLARES g and Lg.  Reads: T, tril, tril_index, G, c, P.  EY_CHAIN_INDEX is its choice alone, for a table of another
// stride (k_hmc_metric's [G, P] scales): DECLARES g.  Reads: G, c.
#define EY_CHAIN_INDEX(g, index)                            \
  int64_t g = G == 1 ? 0 : ((index) ? (int64_t)(index)[c] : c); \
  g = g < 0 ? 0 : (g > G - 1 ? G - 1 : g)
#define EY_CHAIN_FACTOR(Lg)        \
  EY_CHAIN_INDEX(g, tril_index);   \
  const T* Lg = tril + g * (int64_t)P * P

// z of a draw into the LDS vector dst: the chain's own stream, or the caller's values.  Reads: T, z_in, rn, c, P, lane.
#define EY_READ_Z(dst)                                                 \
  do {                                                                 \
    if (!z_in) fill_normals<T>(dst, rn, P);                            \
    else {                                                             \
      for (int i = lane; i < P; i += WAVE) (dst)[i] = z_in[c * P + i]; \
      __syncthreads();                                                 \
    }                                                                  \
  } while (0)

// a dense row-major lower triangle (only j <= i is touched) into the packed ram_col order.  One statement.  Reads: P, lane.
#define EY_TRIL_PACK(S, dense)                                                                        \
  for (int j = 0; j < P; ++j)                                                                         \
    for (int i = j + lane; i < P; i += WAVE) (S)[ram_col(j, P) + i - j] = (dense)[(int64_t)i * P + j]

// acc[r] += sum_j (b S[i, j]) z[j] for the packed factor S and the lane's R rows i = lane + 64 r: a column sweep, one running
// sum per row (clamped index, the term's input selected to zero: DESIGN.md 4.4).  R is wave-uniform (P <= 64 has no second
// row); a caller without a scale passes b = 1, which multiplies nothing.  Reads: T, P, lane.
#define EY_TRIL_SWEEP(S, z, R, b, acc)            \
  do {                                            \
    for (int j = 0; j < P; ++j) {                 \
      const T zj = (z)[j];                        \
      const T* col = (S) + ram_col(j, P) - j;     \
      _Pragma("unroll")                           \
      for (int r = 0; r < 2; ++r) {               \
        if (r >= (R)) break;                      \
        const int i = lane + r * WAVE;            \
        const bool on = i >= j && i < P;          \
        const T s = col[on ? i : j];              \
        (acc)[r] += ((b) * (on ? s : T(0))) * zj; \
      }                                           \
    }                                             \
  } while (0)

// acc[r] += sum_i (b S[i, j]) x[i] for the packed factor S and the lane's R COLUMNS j = lane + 64 r: the transposed product
// L^T x.  The packed order keeps a column contiguous from its diagonal down, so a lane walks its own columns.  Every lane
// sums over i = 0, 1, ..., P - 1 in that order -- the rows above a column's diagonal enter with the factor selected to zero
// behind an index clamped onto the diagonal -- so the trip count is wave-uniform and the order of a sum depends on
// nothing but P.  A lane without a column (j >= P) takes column P - 1 and repeats its owner's work: the same inputs, hence
// the same bits (EY_LANE_PASS's rule).  x is read as a broadcast.  Reads: T, P, lane.
#define EY_TRIL_TSWEEP(S, x, R, b, acc)                                         \
  do {                                                                          \
    const int ey_j0_ = lane < P ? lane : P - 1;                                 \
    const int ey_j1_ = lane + WAVE < P ? lane + WAVE : P - 1;                   \
    const T* ey_c0_ = (S) + ram_col(ey_j0_, P) - ey_j0_;                        \
    const T* ey_c1_ = (S) + ram_col(ey_j1_, P) - ey_j1_;                        \
    for (int i = 0; i < P; ++i) {                                               \
      const T xi = (x)[i];                                                      \
      _Pragma("unroll")                                                         \
      for (int r = 0; r < 2; ++r) {                                             \
        if (r >= (R)) break;                                                    \
        const int j = r ? ey_j1_ : ey_j0_;                                      \
        const bool on = i >= j;                                                 \
        const T s = (r ? ey_c1_ : ey_c0_)[on ? i : j];                          \
        (acc)[r] += ((b) * (on ? s : T(0))) * xi;                               \
      }                                                                         \
    }                                                                           \
  } while (0)

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_ram(EyModel m, T* theta, T* target, T* chol, const T* z_in, const T* u_in,
                                              double a, double g, uint64_t n0, const T* temp, uint64_t seed,
                                              uint64_t iter0, uint64_t chain_offset, unsigned char* accepted,
                                              T* log_rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, 2);
  const int P = m.P;
  T* S = reinterpret_cast<T*>(smem + lds_bytes(m, 2, sizeof(T)));
  const int Ppad = (P + 3) & ~3;
  T* w = S + (((size_t)P * (P + 1) / 2 + 3) & ~(size_t)3);
  T* dk = w + Ppad;
  T* gk = dk + Ppad;
  T* junk = gk + Ppad;
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T* Sg = chol + c * (int64_t)P * P;
  EY_TRIL_PACK(S, Sg);
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {
    const uint64_t iter = iter0 + (uint64_t)it;
    // ---- z ~ N(0, I) (ram.py:44), then the proposal theta + S z (:45): a column sweep, one running sum per row
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    EY_READ_Z(w);
    T acc[2] = {T(0), T(0)};
    EY_TRIL_SWEEP(S, w, 2, T(1), acc);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      if (i < P) l.th[i] = theta[c * P + i] + acc[r];
    }
    __syncthreads();
    const T tv = eval_target<T, false, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);
    const T log_rate = tv - t_state;  // ram.py:48
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
    const bool acc_ = Num<T>::log(u) < log_rate;  // :50
    if (acc_) {
      t_state = tv;
      for (int i = lane; i < P; i += WAVE) theta[c * P + i] = l.th[i];
    }
    EY_RECORD_SAMPLE(true, i, acc_ ? l.th[i] : theta[c * P + i]);
    record_draw<T>(lane == 0, c, it, C, acc_, tv, t_state, log_rate, target, accepted, log_rate_o, run);
    // ---- adaptation (:59-63), accepted or not.  alpha = min(1, exp(log_rate)) as Python's min takes it: NaN -> 1.
    const T e = Num<T>::exp(log_rate);
    const T alpha = e < T(1) ? e : T(1);
    const double h = fmin(1.0, (double)P * pow((double)(n0 + (uint64_t)it), -g));
    const T beta = (T)(h * ((double)alpha - a));
    T zz = T(0);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      const T zi = w[i < P ? i : 0];
      zz += (i < P ? zi : T(0)) * zi;
    }
    const T nrm = Num<T>::sqrt(wave_sum(zz));
    __syncthreads();  // every lane has read z
    for (int i = lane; i < P; i += WAVE) w[i] = w[i] / nrm;
    __syncthreads();
    // d_k, g_k: lane k sums w_j^2 over j < k in the order j = 0, 1, ... (lane k - 1 adds the same terms in the same order)
    T pre[2] = {T(0), T(0)};
    for (int j = 0; j < P; ++j) {
      const T wj = w[j];
      const T q = wj * wj;
#pragma unroll
      for (int r = 0; r < 2; ++r) pre[r] += (j < lane + r * WAVE) ? q : T(0);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int k = lane + r * WAVE;
      const T wk = w[k < P ? k : 0];
      const T t0 = T(1) + beta * pre[r];
      const T t1 = T(1) + beta * (pre[r] + wk * wk);
      if (k < P) {
        dk[k] = Num<T>::sqrt(t1 / t0);
        gk[k] = beta * wk / Num<T>::sqrt(t0 * t1);
      }
    }
    __syncthreads();
    // backward column sweep: row i keeps sum_{j>k} S_old[i,j] w_j; a lane whose row lies above column k stores into its
    // own slot of `junk` (no store behind a per-lane branch while the running sums are live)
    T run_s[2] = {T(0), T(0)};
    for (int k = P - 1; k >= 0; --k) {
      const T d = dk[k], gm = gk[k], wk = w[k];
      T* col = S + ram_col(k, P) - k;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int i = lane + r * WAVE;
        const bool on = i >= k && i < P;
        const T s = col[on ? i : k];
        const T so = on ? s : T(0);
        const T nv = d * so + gm * run_s[r];
        run_s[r] += so * wk;
        *(on ? col + i : junk + lane) = nv;
      }
    }
    __syncthreads();
  }
  for (int j = 0; j < P; ++j)  // the adapted factor back to its dense form
    for (int i = j + lane; i < P; i += WAVE) Sg[(int64_t)i * P + j] = S[ram_col(j, P) + i - j];
}

// The two limits of the kernels that keep [P, P] triangles in LDS beside the evaluation image, under the sampler's name:
// `lives` is what the P limit is for, `held` what the bytes hold.
static int tril_limits(const ey_plan* pl, const std::string& name, const std::string& lives, const std::string& held,
                       size_t bytes) {
  if (pl->m.P > RAM_MAX_P)
    EY_FAIL(EY_ERR_UNSUPPORTED, name + ": P = " + std::to_string(pl->m.P) + " exceeds the limit of " +
                                    std::to_string(RAM_MAX_P) + " parameters (" + lives + " lives in LDS)");
  if (bytes > 160 * 1024)
    EY_FAIL(EY_ERR_UNSUPPORTED, name + ": " + held + " and the model's evaluation image (" + std::to_string(bytes) +
                                    " bytes) do not fit the 160 KiB LDS of a CU");
  return EY_OK;
}

#if EY_GEN_PART == 0
template <typename T, class TINY>
static int launch_ram(ey_plan* pl, void* theta, void* target, void* chol, const void* z, const void* u, double a,
                      double g, uint64_t n, const EyDraw& d) {
  return launch(k_ram<T, TINY>, d.C, 1, ey_generic_ram_lds(pl), d.s, pl->m, (T*)theta, (T*)target, (T*)chol, (const T*)z,
                (const T*)u, a, g, n, EY_DRAW_ARGS(T, d));
}

size_t ey_generic_ram_lds(const ey_plan* pl) {
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  return lds_bytes(pl->m, 2, esz) + ram_extra_bytes(pl->m.P, esz);
}

int ey_generic_ram(ey_plan* pl, void* theta, void* target, void* chol, const void* z, const void* u, double a, double g,
                   uint64_t n, const EyDraw& d) {
  if (int rc = tril_limits(pl, "RAM", "the factor", "the factor", ey_generic_ram_lds(pl))) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_ram, pl, theta, target, chol, z, u, a, g, n, d);
}
#endif  // EY_GEN_PART == 0

// ----------------------------------------------------------------------------------------------- MH with a fixed factor
// MetropolisHastings.draw (eeyore/samplers/metropolis_hastings.py:41-73) whose kernel is a MultivariateNormalKernel: the
// proposal MultivariateNormal(theta, scale_tril = L).sample() = theta + L z, the loop body of k_mh otherwise (the same
// Philox streams and fill_normals, so L = I proposes what k_mh does with scale = 1).  k_ram without its adaptation: one
// wave per chain, lane <-> rows lane and lane + 64 (P <= 128), the chain's factor staged ONCE per launch into LDS behind
// the MH image in ram_col order, the proposal k_ram's column sweep with one running sum per row.
// tril [G, P, P] row-major: G == 1 one factor for all chains, tril_index == NULL (G == C) chain c's own, otherwise factor
// tril_index[c], clamped into [0, G) so that a bad index cannot become an out-of-bounds read (the range is the caller's
// to check).  Only j <= i of a factor is read.
// z waits in the image's gradient slot, which a gradient-free evaluation leaves free until the proposal is made.
__host__ __device__ static size_t mh_tril_extra_bytes(int P, size_t esz) {
  return esz * (((size_t)P * (P + 1) / 2 + 3) & ~(size_t)3);  // the packed factor
}

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_mh_tril(EyModel m, T* theta, T* target, const T* tril, int64_t G,
                                                  const int* tril_index, const T* z_in, const T* u_in, const T* temp,
                                                  uint64_t seed, uint64_t iter0, uint64_t chain_offset,
                                                  unsigned char* accepted, T* log_rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, 2);
  const int P = m.P;
  T* S = reinterpret_cast<T*>(smem + lds_bytes(m, 2, sizeof(T)));
  T* w = l.gr;
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  EY_CHAIN_FACTOR(Lg);
  EY_TRIL_PACK(S, Lg);
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {  // ey_mh_tril_run: see k_mala
    const uint64_t iter = iter0 + (uint64_t)it;
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    EY_READ_Z(w);
    // theta + L z: k_ram's column sweep
    T acc[2] = {T(0), T(0)};
    EY_TRIL_SWEEP(S, w, 2, T(1), acc);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      if (i < P) l.th[i] = theta[c * P + i] + acc[r];
    }
    __syncthreads();
    const T tv = eval_target<T, false, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);
    const T log_rate = tv - t_state;  // symmetric kernel (metropolis_hastings.py:50)
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
    const bool acc_ = Num<T>::log(u) < log_rate;  // :56
    if (acc_) {
      t_state = tv;
      for (int i = lane; i < P; i += WAVE) theta[c * P + i] = l.th[i];
    }
    EY_RECORD_SAMPLE(true, i, acc_ ? l.th[i] : theta[c * P + i]);
    record_draw<T>(lane == 0, c, it, C, acc_, tv, t_state, log_rate, target, accepted, log_rate_o, run);
    __syncthreads();
  }
}

#if EY_GEN_PART == 0
template <typename T, class TINY>
static int launch_mh_tril(ey_plan* pl, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                          const void* z, const void* u, const EyDraw& d) {
  return launch(k_mh_tril<T, TINY>, d.C, 1, ey_generic_mh_tril_lds(pl), d.s, pl->m, (T*)theta, (T*)target, (const T*)tril,
                G, (const int*)tril_index, (const T*)z, (const T*)u, EY_DRAW_ARGS(T, d));
}

size_t ey_generic_mh_tril_lds(const ey_plan* pl) {
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  return lds_bytes(pl->m, 2, esz) + mh_tril_extra_bytes(pl->m.P, esz);
}

int ey_generic_mh_tril(ey_plan* pl, void* theta, void* target, const void* tril, int64_t G, const void* tril_index,
                       const void* z, const void* u, const EyDraw& d) {
  if (int rc = tril_limits(pl, "MH with a factor", "the factor", "the factor", ey_generic_mh_tril_lds(pl))) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_mh_tril, pl, theta, target, tril, G, tril_index, z, u, d);
}
#endif  // EY_GEN_PART == 0

// ----------------------------------------------------------------------------------------------- MALA with a fixed factor
// MALA.draw (eeyore/samplers/mala.py:46-82) whose kernel is a MultivariateNormalKernel: the proposal
// MultivariateNormal(loc, scale_tril = L).sample() = loc + L z around loc = theta + step/2 grad, the loop body of k_mala
// otherwise (the same Philox streams and fill_normals).  step enters the mean only: the covariance is L L^T as given.
// k_mh_tril's layout: one wave per chain, lane <-> rows lane and lane + 64 (P <= 128), the chain's factor staged ONCE per
// launch into LDS behind the MALA image in ram_col order, chosen as there (G, tril_index, clamped); only j <= i is read.
// z waits in the image's slot of the proposal's gradient, which is free until the evaluation at the proposal.
// The proposal is no longer symmetric:  log_rate = (t' - t) + |L^-1 (prop - loc)|^2 / 2 - |L^-1 (theta - loc')|^2 / 2 with
// loc' = prop + step/2 grad', the -sum log L_ii - P/2 log 2 pi of both densities cancelling.

// |L^-1 r|^2 for the packed factor S by column-oriented forward substitution: a lane holds the residuals of its two rows
// (r0: row lane, r1: row lane + 64; rows >= P hold 0 and are never touched), y_j = r_j / L_jj comes from the lane that owns
// row j (j is wave-uniform) and every lane sums the y_j^2 in the order of j, so the result is wave-uniform.  Clamped
// index, the term's input selected to zero, no memory operation behind a per-lane branch.
template <typename T>
__device__ inline T tril_solve_sq(const T* S, int P, T r0, T r1, int lane) {
  T q = T(0);
  for (int j = 0; j < P; ++j) {
    const T* col = S + ram_col(j, P) - j;
    const T y = __shfl(j < WAVE ? r0 : r1, j & (WAVE - 1), WAVE) / col[j];
    q += y * y;
    {
      const int i = lane;
      const bool on = i > j && i < P;
      const T s = col[on ? i : j];
      r0 -= (on ? s : T(0)) * y;
    }
    {
      const int i = lane + WAVE;
      const bool on = i > j && i < P;
      const T s = col[on ? i : j];
      r1 -= (on ? s : T(0)) * y;
    }
  }
  return q;
}

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_mala_tril(EyModel m, T* theta, T* target, T* grad, const T* tril, int64_t G,
                                                    const int* tril_index, const T* z_in, const T* u_in, T step,
                                                    const T* step_vec, const T* temp, uint64_t seed, uint64_t iter0,
                                                    uint64_t chain_offset, unsigned char* accepted, T* log_rate_o,
                                                    EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, 4);
  const int P = m.P;
  T* S = reinterpret_cast<T*>(smem + lds_bytes(m, 4, sizeof(T)));
  T* prop = l.a;
  T* gp = l.b;
  T* w = l.b;
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  const T eps = step_vec ? step_vec[c] : step;
  EY_CHAIN_FACTOR(Lg);
  EY_TRIL_PACK(S, Lg);
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {  // ey_mala_tril_run: see k_mala
    const uint64_t iter = iter0 + (uint64_t)it;
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    EY_READ_Z(w);
    // loc = kernel_mean (mala.py:35-36); a lane without a row repeats row P - 1's loads and stores
    T loc[2], acc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      const int ii = i < P ? i : P - 1;
      const T th = theta[c * P + ii], gi = grad[c * P + ii];
      l.th[ii] = th;
      l.gr[ii] = gi;
      loc[r] = th + T(0.5) * eps * gi;
      acc[r] = loc[r];
    }
    // loc + L z, MultivariateNormal(loc, scale_tril=L).sample(): k_ram's column sweep with the running sum of a row
    // started at its loc, so that L = sqrt(step) I makes the one multiply-add per row that k_mala makes
    EY_TRIL_SWEEP(S, w, 2, T(1), acc);
    T d[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      const bool on = i < P;
      *(on ? prop + i : w + (P - 1)) = acc[r];  // a lane without a row stores into z's slot, which is spent
      d[r] = on ? acc[r] - loc[r] : T(0);
    }
    const T qf = tril_solve_sq<T>(S, P, d[0], d[1], lane);  // the reference solves for it too (log_prob(proposed), :60)
    __syncthreads();
    // inlined here whatever the other kernels of this file do with it: out of line (TinyDyn in f64), the call makes this
    // kernel save its live registers to scratch around it
    T tv;
    [[clang::always_inline]] tv = eval_target<T, true, TINY>(m, l, prop, gp, ht, tc, nullptr, nullptr);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      const bool on = i < P;
      const int ii = on ? i : P - 1;
      const T loc2 = prop[ii] + T(0.5) * eps * gp[ii];
      d[r] = on ? l.th[ii] - loc2 : T(0);
    }
    const T qb = tril_solve_sq<T>(S, P, d[0], d[1], lane);
    const T log_rate = ((tv - t_state) + T(0.5) * qf) - T(0.5) * qb;  // mala.py:58-64, the constants cancelled
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
    const bool acc_ = Num<T>::log(u) < log_rate;  // mala.py:66
    if (acc_) {
      t_state = tv;
      for (int i = lane; i < P; i += WAVE) {
        theta[c * P + i] = prop[i];
        grad[c * P + i] = gp[i];
      }
    }
    EY_RECORD_SAMPLE(true, i, acc_ ? prop[i] : l.th[i]);
    record_draw<T>(lane == 0, c, it, C, acc_, tv, t_state, log_rate, target, accepted, log_rate_o, run);
    __syncthreads();
  }
}

#if EY_GEN_PART == 0
template <typename T, class TINY>
static int launch_mala_tril(ey_plan* pl, void* theta, void* target, void* grad, const void* tril, int64_t G,
                            const void* tril_index, const void* z, const void* u, double step, const void* step_vec,
                            const EyDraw& d) {
  return launch(k_mala_tril<T, TINY>, d.C, 1, ey_generic_mala_tril_lds(pl), d.s, pl->m, (T*)theta, (T*)target, (T*)grad,
                (const T*)tril, G, (const int*)tril_index, (const T*)z, (const T*)u, (T)step, (const T*)step_vec,
                EY_DRAW_ARGS(T, d));
}

size_t ey_generic_mala_tril_lds(const ey_plan* pl) {
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  return lds_bytes(pl->m, 4, esz) + mh_tril_extra_bytes(pl->m.P, esz);
}

int ey_generic_mala_tril(ey_plan* pl, void* theta, void* target, void* grad, const void* tril, int64_t G,
                         const void* tril_index, const void* z, const void* u, double step, const void* step_vec,
                         const EyDraw& d) {
  if (int rc = tril_limits(pl, "MALA with a factor", "the factor", "the factor", ey_generic_mala_tril_lds(pl))) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_mala_tril, pl, theta, target, grad, tril, G, tril_index, z, u, step,
                          step_vec, d);
}
#endif  // EY_GEN_PART == 0

// ----------------------------------------------------------------------------------------------- HMC with a fixed metric
// Euclidean-metric HMC with a fixed inverse metric Sigma = L L^T (Stan's diag_e / dense_e): p ~ N(0, Sigma^-1),
// K(p) = p^T Sigma p / 2, written in the whitened velocity v = L^T p so that nothing is solved for:
//   v ~ N(0, I);  h_cur = -t + |v|^2 / 2;  v += eps/2 L^T g;  L times { theta += eps L v;  (t, g) at theta;  v += w L^T g };
//   h_prop = -t + |v|^2 / 2;  the accept step of k_hmc.
// The loop body of k_hmc otherwise -- the same Philox streams and fill_normals, so L = I makes k_hmc's draw, and each
// multiply-add of it: the products run with the step folded into the factor, (eps L_ij) x_j, on a running sum started at
// the vector they update.  One wave per chain, no row-wave form, n_iters draws per launch on the records of the one-wave
// kernels.  FORM EY_METRIC_TRIL: k_mala_tril's layout -- the chain's factor staged ONCE per launch behind the three-vector
// image in ram_col order, chosen as there (G, metric_index, clamped), P <= 128, rows lane and lane + 64; L v is k_ram's
// column sweep (a lane owns rows), L^T g the transposed sweep (a lane owns columns).  FORM EY_METRIC_DIAG: L = diag(s), s
// [P] of metric [G, P] staged as the image's fourth vector; any P the image holds.
__host__ __device__ static size_t hmc_metric_lds(const EyModel& m, int form, size_t esz) {
  return form == EY_METRIC_TRIL ? lds_bytes(m, 3, esz) + mh_tril_extra_bytes(m.P, esz) : lds_bytes(m, 4, esz);
}

// The two halves of a leapfrog step under the metric, written once for both forms.  Each ends with the barrier that lets
// every lane read what the others wrote (a sweep reads the whole of the other vector).  The diagonal form's element loops
// run, in this unit, a trip count that is stated to be wave-uniform (readfirstlane), over the index clamped as in
// EY_LANE_PASS: as `for (i = lane; i < P; i += WAVE)`, and as EY_LANE_PASS on a P the compiler keeps in a vector register,
// the loop is left with EXEC empty, and k_hmc_metric<float, TinyDyn, EY_METRIC_DIAG> was built with the copies that carry
// the image's offsets around the leapfrog loop inside that region, where they copy nothing -- an accepted draw then stored
// its gradient from the wrong LDS address.  k_nuts (EY_GEN_PART 1) keeps the plain loop: with a lane pass
// the compiler stops on that unit ("Illegal instruction detected: Operand has incorrect register class"), and
// tests/test_cross_metric_gpu.py holds its build as it is.
#if EY_GEN_PART == 0
#define EY_METRIC_EACH(i)                                                                                         \
  for (int ey_r_ = 0, ey_nr_ = __builtin_amdgcn_readfirstlane((P + WAVE - 1) / WAVE), i = lane < P ? lane : P - 1; \
       ey_r_ < ey_nr_; ++ey_r_, i = lane + ey_r_ * WAVE < P ? lane + ey_r_ * WAVE : P - 1)
#else
#define EY_METRIC_EACH(i) for (int i = lane, ey_r_ = 0; i < P; i += WAVE)
#endif
// v += w L^T g.  Reads: T, FORM, P, R, lane, S, sd, v, l.
#define EY_METRIC_KICK(w)                                                                   \
  do {                                                                                      \
    const T ey_w_ = (w);                                                                    \
    if constexpr (FORM == EY_METRIC_TRIL) {                                                 \
      T acc[2];                                                                             \
      _Pragma("unroll")                                                                     \
      for (int r = 0; r < 2; ++r) acc[r] = v[lane + r * WAVE < P ? lane + r * WAVE : P - 1]; \
      EY_TRIL_TSWEEP(S, l.gr, R, ey_w_, acc);                                               \
      _Pragma("unroll")                                                                     \
      for (int r = 0; r < 2; ++r) {                                                         \
        if (r >= R) break;                                                                  \
        v[lane + r * WAVE < P ? lane + r * WAVE : P - 1] = acc[r];                          \
      }                                                                                     \
    } else {                                                                                \
      EY_METRIC_EACH(i) {                                                                   \
        (void)ey_r_;                                                                        \
        v[i] = v[i] + (ey_w_ * sd[i]) * l.gr[i];                                            \
      }                                                                                     \
    }                                                                                       \
    __syncthreads();                                                                        \
  } while (0)
// theta += eps L v.  Reads: T, FORM, P, R, lane, S, sd, v, l, eps.
#define EY_METRIC_DRIFT()                                                                   \
  do {                                                                                      \
    if constexpr (FORM == EY_METRIC_TRIL) {                                                 \
      T acc[2];                                                                             \
      _Pragma("unroll")                                                                     \
      for (int r = 0; r < 2; ++r) acc[r] = l.th[lane + r * WAVE < P ? lane + r * WAVE : P - 1]; \
      EY_TRIL_SWEEP(S, v, R, eps, acc);                                                     \
      _Pragma("unroll")                                                                     \
      for (int r = 0; r < 2; ++r) {                                                         \
        const int i = lane + r * WAVE;                                                      \
        if (i < P) l.th[i] = acc[r];                                                        \
      }                                                                                     \
    } else {                                                                                \
      EY_METRIC_EACH(i) {                                                                   \
        (void)ey_r_;                                                                        \
        l.th[i] = l.th[i] + (eps * sd[i]) * v[i];                                           \
      }                                                                                     \
    }                                                                                       \
    __syncthreads();                                                                        \
  } while (0)
// EY_LEAPFROG under the metric: half a kick, L drifts with an evaluation each (its value left in t), the last kick halved.
// Reads: what the two halves read, and TINY, m, ht, tc, L.
#define EY_LEAPFROG_METRIC(t)                                                           \
  do {                                                                                  \
    EY_METRIC_KICK(T(0.5) * eps);                                                       \
    for (int k = 1; k <= L; ++k) {                                                      \
      EY_METRIC_DRIFT();                                                                \
      t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);       \
      const T w = (k < L) ? eps : T(0.5) * eps;                                         \
      EY_METRIC_KICK(w);                                                                \
    }                                                                                   \
  } while (0)

// ---- steps the metric kernels share (k_hmc_metric, k_hmc_metric_warmup; k_nuts and k_nuts_ws through ey_nuts_draw.h)
// The chain's metric into LDS, once per launch: the row of `metric` chosen as EY_CHAIN_INDEX says, a dense factor packed
// into S, a diagonal's scales copied into sd.  The caller's barrier follows.  DECLARES g.  Reads: T, FORM, metric,
// metric_index, G, c, P, lane, S, sd.
#define EY_METRIC_STAGE()                                \
  EY_CHAIN_INDEX(g, metric_index);                       \
  if constexpr (FORM == EY_METRIC_TRIL) {                \
    const T* Lg = metric + g * (int64_t)P * P;           \
    EY_TRIL_PACK(S, Lg);                                 \
  } else {                                               \
    const T* sg = metric + g * (int64_t)P;               \
    for (int i = lane; i < P; i += WAVE) sd[i] = sg[i];  \
  }
// kin = |v|^2 over the wave: a lane pass, the idle lanes' inputs selected to zero.  Reads: T, P, lane, v.
#define EY_KINETIC(kin)                \
  do {                                 \
    kin = T(0);                        \
    EY_LANE_PASS(P, i, on) {           \
      const T vz = on ? v[i] : T(0);   \
      kin += vz * vz;                  \
    }                                  \
    kin = wave_sum(kin);               \
  } while (0)
// The two warm-up epilogues of a draw, as the comment of k_hmc_metric_warmup describes them: the dual-averaging step on
// `rate` into the step variable `eps` (and step_vec[c]), then the Welford moments of x_i, an expression in i for element i
// of the state the chain is left in.  Both conditions are wave-uniform.  Reads: T, FORM, P, lane, c, it, w, da, rate,
// step_vec, mean_c, M2_c, dlt.
#define EY_WARM_EPILOGUES(x_i, eps)                                                                                  \
  do {                                                                                                               \
    if (w.da_state && it < w.da_n) {                                                                                 \
      eps = (T)ey_da_update(da, w.da_table + 3 * it, (double)rate, w.d, w.has_eub != 0, w.logeub, it == w.final_it); \
      if (lane == 0) step_vec[c] = eps;                                                                              \
    }                                                                                                                \
    if (mean_c) {                                                                                                    \
      const double ey_cnt_ = (double)(w.count + it + 1);                                                             \
      const double ey_f_ = (ey_cnt_ - 1.0) / ey_cnt_;                                                                \
      /* l.gr has been read for the last time: dlt takes its place */                                                \
      if constexpr (FORM == EY_METRIC_TRIL) __syncthreads();                                                         \
      EY_LANE_PASS(P, i, on) {                                                                                       \
        (void)on;                                                                                                    \
        const double x = (double)(x_i);                                                                              \
        const double mu = mean_c[i];                                                                                 \
        const double dx = x - mu;                                                                                    \
        mean_c[i] = mu + dx / ey_cnt_;                                                                               \
        if constexpr (FORM == EY_METRIC_TRIL) {                                                                      \
          dlt[i] = dx;                                                                                               \
        } else {                                                                                                     \
          M2_c[i] = M2_c[i] + ey_f_ * (dx * dx);                                                                     \
        }                                                                                                            \
      }                                                                                                              \
      if constexpr (FORM == EY_METRIC_TRIL) {                                                                        \
        __syncthreads();                                                                                             \
        for (int i = 0; i < P; ++i) {                                                                                \
          const double fi = ey_f_ * dlt[i];                                                                          \
          double* row = M2_c + (int64_t)i * P;                                                                       \
          _Pragma("unroll")                                                                                          \
          for (int r = 0; r < 2; ++r) {                                                                              \
            if (r * WAVE > i) break; /* a round wholly beyond the diagonal: wave-uniform */                          \
            const int j = lane + r * WAVE;                                                                           \
            const int jj = j <= i ? j : i;                                                                           \
            row[jj] = row[jj] + fi * dlt[jj];                                                                        \
          }                                                                                                          \
        }                                                                                                            \
      }                                                                                                              \
    }                                                                                                                \
  } while (0)

// The LDS limit of the diagonal form, which holds no triangle: the refusal under the sampler's name.
static int diag_limit(const std::string& name, size_t bytes) {
  if (bytes > 160 * 1024)
    EY_FAIL(EY_ERR_UNSUPPORTED, name + " with a diagonal metric: the model's evaluation image and the scales (" +
                                    std::to_string(bytes) + " bytes) do not fit the 160 KiB LDS of a CU");
  return EY_OK;
}

#if EY_GEN_PART == 0  // (to the end of the file)
template <typename T, class TINY, int FORM>
__global__ void __launch_bounds__(WAVE) k_hmc_metric(EyModel m, T* theta, T* target, T* grad, const T* metric, int64_t G,
                                                     const int* metric_index, const T* v0, const T* u_in, T step,
                                                     const T* step_vec, int L, int recompute, T* hcur_o, T* hprop_o,
                                                     const T* temp, uint64_t seed, uint64_t iter0, uint64_t chain_offset,
                                                     unsigned char* accepted, T* rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, FORM == EY_METRIC_TRIL ? 3 : 4);
  const int P = m.P;
  T* S = reinterpret_cast<T*>(smem + lds_bytes(m, 3, sizeof(T)));  // EY_METRIC_TRIL: the packed factor
  T* sd = l.b;                                                     // EY_METRIC_DIAG: the scales
  T* v = l.a;
  const int R = P > WAVE ? 2 : 1;  // the rows (and columns) of a lane: wave-uniform
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  const T eps = step_vec ? step_vec[c] : step;
  EY_METRIC_STAGE();
  (void)S; (void)sd; (void)R;
  __syncthreads();
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {  // ey_hmc_metric_run: see k_mala
    const uint64_t iter = iter0 + (uint64_t)it;
    // v ~ N(0, I): k_hmc's momentum draw
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    T kin = T(0);
    if (!v0) fill_normals<T>(v, rn, P);
    EY_LANE_PASS(P, i, on) {
      l.th[i] = theta[c * P + i];
      l.gr[i] = grad[c * P + i];
      const T vi = v0 ? v0[c * P + i] : v[i];
      v[i] = vi;
      const T vz = on ? vi : T(0);
      kin += vz * vz;
    }
    kin = wave_sum(kin);
    const T h_cur = -t_state + T(0.5) * kin;
    __syncthreads();
    T t = t_state;
    if (recompute) t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);
    EY_LEAPFROG_METRIC(t);
    EY_KINETIC(kin);
    const T h_prop = -t + T(0.5) * kin;
    T rate = Num<T>::exp(h_cur - h_prop);
    if (rate > T(1)) rate = T(1);
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
    const bool acc_ = u < rate;  // strict <; a NaN rate rejects (k_hmc)
    if (acc_) {
      t_state = t;
      for (int i = lane; i < P; i += WAVE) {
        theta[c * P + i] = l.th[i];
        grad[c * P + i] = l.gr[i];
      }
    }
    EY_RECORD_SAMPLE(true, i, acc_ ? l.th[i] : theta[c * P + i]);
    record_draw<T>(lane == 0, c, it, C, acc_, t, t_state, rate, target, accepted, rate_o, run);
    if (lane == 0) {
      if (hcur_o) hcur_o[c] = h_cur;
      if (hprop_o) hprop_o[c] = h_prop;
    }
    __syncthreads();
  }
}

template <typename T, class TINY>
static int launch_hmc_metric(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                             const void* metric_index, const void* v0, const void* u, double step, const void* step_vec,
                             int L, const EyDraw& d, void* hcur, void* hprop) {
  const size_t bytes = ey_generic_hmc_metric_lds(pl, form);
  const int recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) != 0;
  if (form == EY_METRIC_TRIL)
    return launch(k_hmc_metric<T, TINY, EY_METRIC_TRIL>, d.C, 1, bytes, d.s, pl->m, (T*)theta, (T*)target, (T*)grad,
                  (const T*)metric, G, (const int*)metric_index, (const T*)v0, (const T*)u, (T)step, (const T*)step_vec, L,
                  recompute, (T*)hcur, (T*)hprop, EY_DRAW_ARGS(T, d));
  return launch(k_hmc_metric<T, TINY, EY_METRIC_DIAG>, d.C, 1, bytes, d.s, pl->m, (T*)theta, (T*)target, (T*)grad,
                (const T*)metric, G, (const int*)metric_index, (const T*)v0, (const T*)u, (T)step, (const T*)step_vec, L,
                recompute, (T*)hcur, (T*)hprop, EY_DRAW_ARGS(T, d));
}

size_t ey_generic_hmc_metric_lds(const ey_plan* pl, int form) {
  return hmc_metric_lds(pl->m, form, pl->dtype == EY_F32 ? 4 : 8);
}

// `rate` takes the place of a draw's log_rate: record_draw writes it with the accept flag
int ey_generic_hmc_metric(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                          const void* metric_index, const void* v0, const void* u, double step, const void* step_vec, int L,
                          const EyDraw& d, void* rate, void* hcur, void* hprop) {
  const size_t bytes = ey_generic_hmc_metric_lds(pl, form);
  if (int rc = form == EY_METRIC_TRIL ? tril_limits(pl, "HMC with a dense metric", "the factor", "the factor", bytes)
                                      : diag_limit("HMC", bytes))
    return rc;
  EyDraw dr = d;
  dr.log_rate = rate;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_hmc_metric, pl, theta, target, grad, metric, form, G, metric_index, v0, u,
                          step, step_vec, L, dr, hcur, hprop);
}

// ----------------------------------------------------------------------------------- HMC under a metric: the warm-up form
// k_hmc_metric's draw loop on its own Philox streams (no v0, no u: ey_hmc_metric_run's draws, expression for expression, so
// that a launch with nothing attached leaves its bits), with two optional epilogues after each draw's accept step
// (DESIGN.md 4.23).  A sibling kernel, not a parameter of k_hmc_metric: that kernel and its instantiations stay as they are.
//  Dual averaging: every lane runs ey_da_update on the draw's rate from the chain's state in registers (the same inputs in
//    every lane, hence the same step in every lane: nothing is broadcast), lane 0 writes the step of the next draw to
//    step_vec[c]; the state goes back to memory once, after the last draw.
//  Welford moments of the state the chain is left in, in double, in global memory.  EY_METRIC_DIAG: one pass, a lane owns
//    elements lane, lane + 64, ... of mean and M2 (EY_LANE_PASS: contiguous across the wave).  EY_METRIC_TRIL: the same pass
//    leaves dlt = x - mean_old as doubles in LDS, over l.gr and l.a, which hold nothing between the accept step and the next
//    draw's loads (8 P bytes <= the two vectors in either dtype); then row i of M2 is updated for j <= i with the lanes
//    along j, 64 columns a round: a round beyond the diagonal is skipped (wave-uniform), a lane beyond it inside a round
//    takes the diagonal element and repeats its owner's work on the same inputs.  The strict upper triangle is never
//    touched.  No atomics; every sum's order depends on P alone.
template <typename T, class TINY, int FORM>
__global__ void __launch_bounds__(WAVE) k_hmc_metric_warmup(EyModel m, T* theta, T* target, T* grad, const T* metric,
                                                            int64_t G, const int* metric_index, T step, T* step_vec, int L,
                                                            int recompute, EyWarm w, const T* temp, uint64_t seed,
                                                            uint64_t iter0, uint64_t chain_offset, unsigned char* accepted,
                                                            T* rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, FORM == EY_METRIC_TRIL ? 3 : 4);
  const int P = m.P;
  T* S = reinterpret_cast<T*>(smem + lds_bytes(m, 3, sizeof(T)));  // EY_METRIC_TRIL: the packed factor
  T* sd = l.b;                                                     // EY_METRIC_DIAG: the scales
  T* v = l.a;
  double* dlt = reinterpret_cast<double*>(l.gr);                   // EY_METRIC_TRIL moments: x - mean_old, between draws
  const int R = P > WAVE ? 2 : 1;  // the rows (and columns) of a lane: wave-uniform
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T eps = step_vec ? step_vec[c] : step;
  EY_METRIC_STAGE();
  (void)S; (void)sd; (void)R; (void)dlt;
  double da[3] = {0.0, 0.0, 0.0};
  if (w.da_state) {
    for (int k = 0; k < 3; ++k) da[k] = w.da_state[3 * c + k];
  }
  double* mean_c = w.mean ? w.mean + c * (int64_t)P : nullptr;
  double* M2_c = w.M2 ? w.M2 + c * (FORM == EY_METRIC_TRIL ? (int64_t)P * P : (int64_t)P) : nullptr;
  __syncthreads();
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {
    const uint64_t iter = iter0 + (uint64_t)it;
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    T kin = T(0);
    fill_normals<T>(v, rn, P);
    EY_LANE_PASS(P, i, on) {
      l.th[i] = theta[c * P + i];
      l.gr[i] = grad[c * P + i];
      const T vi = v[i];
      v[i] = vi;
      const T vz = on ? vi : T(0);
      kin += vz * vz;
    }
    kin = wave_sum(kin);
    const T h_cur = -t_state + T(0.5) * kin;
    __syncthreads();
    T t = t_state;
    if (recompute) t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);
    EY_LEAPFROG_METRIC(t);
    EY_KINETIC(kin);
    const T h_prop = -t + T(0.5) * kin;
    T rate = Num<T>::exp(h_cur - h_prop);
    if (rate > T(1)) rate = T(1);
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    const T u = ey_rng_uniform<T>(ru);
    const bool acc_ = u < rate;  // strict <; a NaN rate rejects (k_hmc)
    if (acc_) {
      t_state = t;
      for (int i = lane; i < P; i += WAVE) {
        theta[c * P + i] = l.th[i];
        grad[c * P + i] = l.gr[i];
      }
    }
    EY_RECORD_SAMPLE(true, i, acc_ ? l.th[i] : theta[c * P + i]);
    record_draw<T>(lane == 0, c, it, C, acc_, t, t_state, rate, target, accepted, rate_o, run);
    if (lane == 0) {
      if (w.steps_rec) static_cast<T*>(w.steps_rec)[(int64_t)it * C + c] = eps;
      if (w.rate_rec) static_cast<T*>(w.rate_rec)[(int64_t)it * C + c] = rate;
    }
    EY_WARM_EPILOGUES(acc_ ? l.th[i] : theta[c * P + i], eps);
    __syncthreads();
  }
  if (w.da_state && lane == 0) {
    w.da_state[3 * c] = da[0];
    w.da_state[3 * c + 1] = da[1];
  }
}

template <typename T, class TINY>
static int launch_hmc_metric_warmup(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form,
                                    int64_t G, const void* metric_index, double step, void* step_vec, int L,
                                    const EyDraw& d, const EyWarm& w) {
  const size_t bytes = ey_generic_hmc_metric_lds(pl, form);
  const int recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) != 0;
  if (form == EY_METRIC_TRIL)
    return launch(k_hmc_metric_warmup<T, TINY, EY_METRIC_TRIL>, d.C, 1, bytes, d.s, pl->m, (T*)theta, (T*)target, (T*)grad,
                  (const T*)metric, G, (const int*)metric_index, (T)step, (T*)step_vec, L, recompute, w,
                  EY_DRAW_ARGS(T, d));
  return launch(k_hmc_metric_warmup<T, TINY, EY_METRIC_DIAG>, d.C, 1, bytes, d.s, pl->m, (T*)theta, (T*)target, (T*)grad,
                (const T*)metric, G, (const int*)metric_index, (T)step, (T*)step_vec, L, recompute, w, EY_DRAW_ARGS(T, d));
}

// the limits and the LDS image are ey_generic_hmc_metric's: the moments live in global memory
int ey_generic_hmc_metric_warmup(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form,
                                 int64_t G, const void* metric_index, double step, void* step_vec, int L, const EyDraw& d,
                                 const EyWarm& w) {
  const size_t bytes = ey_generic_hmc_metric_lds(pl, form);
  if (int rc = form == EY_METRIC_TRIL ? tril_limits(pl, "HMC with a dense metric", "the factor", "the factor", bytes)
                                      : diag_limit("HMC", bytes))
    return rc;
  EyDraw dr = d;
  dr.log_rate = nullptr;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_hmc_metric_warmup, pl, theta, target, grad, metric, form, G, metric_index,
                          step, step_vec, L, dr, w);
}

// ----------------------------------------------------------------------------------------------- Metropolis within Gibbs
// Gibbs.draw (eeyore/samplers/gibbs.py:67-102): per draw, S accept/reject sub-steps, each a Normal random-walk proposal
// for one block of parameters and one evaluation of the whole log-target.  The kernel knows nothing of nodes: it walks a
// table of disjoint index sets (ey_gibbs_table), so that parameter i consumes normal i of the iteration's stream whichever
// block holds it.  One wave per chain, no row-wave form.  LDS: the proposal vector in l.th, the CURRENT state in l.gr
// (eval_target<GRAD = false> never touches it), the iteration's normals in l.a, then the table.  Global theta is read once
// per launch and written once per iteration.  carry = false: a rejected block of the proposal vector is restored from the
// state (a valid Metropolis-within-Gibbs); carry = true: it stays for the rest of the draw, as the reference leaves it
// (DESIGN.md 4.11, 8), and the proposal vector restarts from the state at the next draw (`proposed = current.clone()`).
static size_t gibbs_table_bytes(int S, int n_idx, size_t esz) {
  return (((size_t)4 * (S + 1 + n_idx) + 7) & ~(size_t)7) + esz * (size_t)S;
}

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_gibbs(EyModel m, T* theta, T* target, const T* z_in, const T* u_in,
                                                const int* blk_off, const int* blk_idx, const T* blk_scale, int S,
                                                int n_idx, int carry, const T* temp, uint64_t seed, uint64_t iter0,
                                                uint64_t chain_offset, unsigned char* accepted, T* log_rate_o,
                                                double* mom_acc, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, 3);
  const int P = m.P;
  T* cur = l.gr;
  T* zs = l.a;
  unsigned char* tb = smem + lds_bytes(m, 3, sizeof(T));
  int* off = reinterpret_cast<int*>(tb);
  int* idx = off + S + 1;
  T* scl = reinterpret_cast<T*>(tb + (((size_t)4 * (S + 1 + n_idx) + 7) & ~(size_t)7));
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  for (int s = lane; s <= S; s += WAVE) off[s] = blk_off[s];
  for (int j = lane; j < n_idx; j += WAVE) idx[j] = blk_idx[j];
  for (int s = lane; s < S; s += WAVE) scl[s] = blk_scale[s];
  for (int i = lane; i < P; i += WAVE) {
    const T v = theta[c * P + i];
    cur[i] = v;
    l.th[i] = v;
  }
  T t_state = target[c];
  __syncthreads();
  for (int it = 0; it < run.n_iters; ++it) {
    const uint64_t iter = iter0 + (uint64_t)it;
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    EY_READ_Z(zs);
    int n_acc = 0;
    for (int s = 0; s < S; ++s) {
      const int o0 = off[s], o1 = off[s + 1];
      const T sc = scl[s];
      for (int j = o0 + lane; j < o1; j += WAVE) {
        const int i = idx[j];
        l.th[i] = l.th[i] + sc * zs[i];  // NormalKernel(proposed[idx], scale).sample() (gibbs.py:84-86)
      }
      __syncthreads();
      const T tv = eval_target<T, false, TINY>(m, l, l.th, cur, ht, tc, nullptr, nullptr);
      const T log_rate = tv - t_state;  // :89
      const T u = u_in ? u_in[c * S + s] : ey_rng_uniform_at<T>(ru, (uint32_t)s);
      const bool acc = Num<T>::log(u) < log_rate;  // :90; a NaN log-rate rejects
      if (acc) {
        t_state = tv;
        for (int j = o0 + lane; j < o1; j += WAVE) {
          const int i = idx[j];
          cur[i] = l.th[i];
        }
      } else if (!carry) {
        for (int j = o0 + lane; j < o1; j += WAVE) {
          const int i = idx[j];
          l.th[i] = cur[i];
        }
      }
      n_acc += acc ? 1 : 0;
      if (lane == 0) {
        accepted[c * S + s] = acc ? 1 : 0;
        if (log_rate_o) log_rate_o[c * S + s] = log_rate;
        if (run.accepted) static_cast<unsigned char*>(run.accepted)[((int64_t)it * C + c) * S + s] = acc ? 1 : 0;
        if (run.accept_count && acc) run.accept_count[c * S + s] += 1;
      }
      __syncthreads();
    }
    T* so = run.samples ? static_cast<T*>(run.samples) + ((int64_t)it * C + c) * P : nullptr;
    for (int i = lane; i < P; i += WAVE) {
      const T v = cur[i];
      theta[c * P + i] = v;
      if (so) so[i] = v;
      if (carry) l.th[i] = v;  // the next draw's proposal vector starts from the state (:78)
    }
    if (lane == 0) {
      target[c] = t_state;
      if (run.targets) static_cast<T*>(run.targets)[(int64_t)it * C + c] = t_state;
      if (mom_acc) mom_acc[c] += (double)n_acc / (double)S;
    }
    __syncthreads();
  }
}

template <typename T, class TINY>
static int launch_gibbs(ey_plan* pl, const ey_gibbs_table* tb, void* theta, void* target, const void* z, const void* u,
                        const EyDraw& d, double* mom_acc) {
  return launch(k_gibbs<T, TINY>, d.C, 1, ey_generic_gibbs_lds(pl, tb), d.s, pl->m, (T*)theta, (T*)target, (const T*)z,
                (const T*)u, (const int*)tb->d_off, (const int*)tb->d_idx, (const T*)tb->d_scale, tb->S, tb->n_idx,
                (d.flags & EY_GIBBS_CARRY) ? 1 : 0, (const T*)d.temp, d.seed, d.iter, d.chain_offset,
                (unsigned char*)d.accepted, (T*)d.log_rate, mom_acc, d.run ? *d.run : kOneDraw, d.C);
}

size_t ey_generic_gibbs_lds(const ey_plan* pl, const ey_gibbs_table* tb) {
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  return lds_bytes(pl->m, 3, esz) + gibbs_table_bytes(tb->S, tb->n_idx, esz);
}

int ey_generic_gibbs(ey_plan* pl, const ey_gibbs_table* tb, void* theta, void* target, const void* z, const void* u,
                     const EyDraw& d, double* mom_acc) {
  if (ey_generic_gibbs_lds(pl, tb) > 160 * 1024)
    EY_FAIL(EY_ERR_UNSUPPORTED, "Gibbs: the model's evaluation image and the block table (" +
                                    std::to_string(ey_generic_gibbs_lds(pl, tb)) +
                                    " bytes) do not fit the 160 KiB LDS of a CU");
  if (pl->m.kind != EY_KIND_MLP) EY_FAIL(EY_ERR_UNSUPPORTED, "Gibbs: the blocks are the nodes of an MLP; this plan has none");
  return EY_TINY_DISPATCH(tiny_dispatch_mlp, launch_gibbs, pl, tb, theta, target, z, u, d, mom_acc);
}

// ----------------------------------------------------------------------------------------------- softabs, one wave
// softabs(A, a) = Q diag(f(lambda)) Q^T, f(x) = x / tanh(a x), f(0) = 1 / a (eeyore/stats/metrics.py:3-5) of a symmetric
// [P, P] matrix, P <= 128, by one wave in LDS, in f64 whatever the matrix's dtype.  f is even, so no
// eigenvector is accumulated: one-sided (Hestenes) Jacobi rotates the COLUMNS of a dense copy G = A until every pair is
// orthogonal to (P + 6) 2^-53 of its norms (what rounding leaves of an inner product of two freshly rotated columns: three
// roundings per entry of either column and P additions; a tighter test can rotate for ever); then |lambda_k| = sigma_k =
// |g_k| and
//   softabs(A) = I / a + sum_{sigma_k > tau} ((f(sigma_k) - 1/a) / sigma_k^2) g_k g_k^T,   tau = P 2^-52 max sigma.
// A round of the round-robin (circle) schedule holds ceil(P / 2) <= 64 disjoint column pairs: lane <-> pair, every lane
// walks its two columns (leading dimension P | 1, odd, so the lanes' columns start in different LDS banks).  The loops
// run for the whole wave -- rounds, rows, and the rotation pass is taken when ANY lane rotates --; a lane without a pair,
// or whose pair is orthogonal already, stores into its own slot of `junk`.  A sweep without a rotation ends the
// iteration, SOFTABS_MAX_SWEEPS caps it (the result is then what the columns give).  Nothing is contracted into fused
// multiply-adds: the kernels that inline these functions (k_am, k_softabs) compute the same bits.
#define SOFTABS_MAX_SWEEPS 80
struct SoftabsWork {
  double* G;     // [P] columns of ld
  double* coef;  // [P]
  double* junk;  // [WAVE]
  int ld;
};
__host__ __device__ static inline int softabs_ld(int P) { return P | 1; }
__host__ __device__ static size_t softabs_work_bytes(int P) {
  return 8 * ((size_t)softabs_ld(P) * P + ((P + 3) & ~3) + WAVE);
}
__device__ inline SoftabsWork softabs_carve(unsigned char* p, int P) {
  SoftabsWork w;
  w.ld = softabs_ld(P);
  w.G = reinterpret_cast<double*>(p);
  w.coef = w.G + (size_t)w.ld * P;
  w.junk = w.coef + ((P + 3) & ~3);
  return w;
}

// G <- the symmetric matrix whose lower triangle load(i, j), j <= i, hands out.  False when an entry is not finite.
template <typename LD>
__device__ inline bool softabs_fill(const SoftabsWork w, int P, int lane, LD load) {
  bool bad = false;
  for (int j = 0; j < P; ++j)
    for (int i = j + lane; i < P; i += WAVE) {
      const double v = (double)load(i, j);
      bad = bad || !(fabs(v) <= 1.7976931348623157e308);
      w.G[j * w.ld + i] = v;
      w.G[i * w.ld + j] = v;
    }
  __syncthreads();
  return !__any(bad ? 1 : 0);
}

// the Jacobi sweeps on G, then coef_k; returns the number of sweeps (the last one rotated nothing unless the cap ended it)
__device__ inline int softabs_jacobi(const SoftabsWork w, int P, int lane, double a) {
#pragma clang fp contract(off)
  double* G = w.G;
  const int ld = w.ld;
  const int half = (P + 1) >> 1, m1 = 2 * half - 1;  // players 0 .. m1; player m1 = P is the bye of an odd P
  const double tol = (double)(P + 6) * 0x1p-53;
  int sweeps = 0;
  bool more = P > 1;
  while (more && sweeps < SOFTABS_MAX_SWEEPS) {
    ++sweeps;
    more = false;
    for (int r = 0; r < m1; ++r) {
      const int k = lane < half ? lane : 0;
      int p = k == 0 ? r : (r + k) % m1;
      int q = k == 0 ? m1 : (r + m1 - k) % m1;
      if (p > q) {
        const int t = p;
        p = q;
        q = t;
      }
      const bool on = lane < half && q < P;
      const double* gp = G + (on ? p : 0) * ld;
      const double* gq = G + (on ? q : 0) * ld;
      double al = 0.0, be = 0.0, ga = 0.0;
      for (int i = 0; i < P; ++i) {
        const double x = gp[i], y = gq[i];
        al += x * x;
        be += y * y;
        ga += x * y;
      }
      const bool rot = on && fabs(ga) > tol * (sqrt(al) * sqrt(be));
      if (__any(rot ? 1 : 0)) {  // wave-uniform
        more = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cr = 1.0 / sqrt(1.0 + t * t);
        const double c = rot ? cr : 1.0, s = rot ? cr * t : 0.0;
        double* dp = G + (rot ? p : 0) * ld;
        double* dq = G + (rot ? q : 0) * ld;
        for (int i = 0; i < P; ++i) {
          const double x = dp[i], y = dq[i];
          *(rot ? dp + i : w.junk + lane) = c * x - s * y;
          *(rot ? dq + i : w.junk + lane) = s * x + c * y;
        }
      }
      __syncthreads();
    }
  }
  // sigma_k = |g_k| (lane <-> columns lane, lane + 64), the threshold, the coefficient of g_k g_k^T
  double sig[2], smax = 0.0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int k = lane + r * WAVE;
    const double* g = G + (k < P ? k : 0) * ld;
    double ss = 0.0;
    for (int i = 0; i < P; ++i) ss += g[i] * g[i];
    sig[r] = k < P ? sqrt(ss) : 0.0;
    smax = fmax(smax, sig[r]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) smax = fmax(smax, __shfl_xor(smax, o, WAVE));
  const double tau = ((double)P * 0x1p-52) * smax, ia = 1.0 / a;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int k = lane + r * WAVE;
    const double sg = sig[r] > tau ? sig[r] : 1.0;
    const double f = sg / tanh(a * sg);
    const double cf = sig[r] > tau ? ((f - ia) / sg) / sg : 0.0;
    *(k < P ? w.coef + k : w.junk + lane) = cf;
  }
  __syncthreads();
  return sweeps;
}

// store(i, j, v, on) takes entry (i, j), j <= i, of I / a + sum_k coef_k g_k g_k^T (k ascending, the diagonal's 1 / a added
// last); a lane past the column's end calls it with on = false and a valid (i, j)
template <typename ST>
__device__ inline void softabs_emit(const SoftabsWork w, int P, int lane, double a, ST store) {
#pragma clang fp contract(off)
  const double ia = 1.0 / a;
  for (int j = 0; j < P; ++j)
    for (int i0 = j; i0 < P; i0 += WAVE) {
      const bool on = i0 + lane < P;
      const int i = on ? i0 + lane : j;
      double acc = 0.0;
      for (int k = 0; k < P; ++k) {
        const double* g = w.G + k * w.ld;
        acc += (w.coef[k] * g[i]) * g[j];
      }
      acc += i == j ? ia : 0.0;
      store(i, j, acc, on);
    }
}

// ey_softabs: B dense [P, P] matrices, one wave each; the lower triangle is read, the whole symmetric matrix written.  A
// matrix with an entry that is not finite comes back as it was (its lower triangle mirrored), sweeps = -1.
template <typename T>
__global__ void __launch_bounds__(WAVE) k_softabs(const T* A, T* out, int* sweeps, int P, double a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SoftabsWork w = softabs_carve(smem, P);
  const int lane = threadIdx.x;
  const T* Ab = A + (int64_t)blockIdx.x * P * P;
  T* Ob = out + (int64_t)blockIdx.x * P * P;
  int sw = -1;
  if (softabs_fill(w, P, lane, [&](int i, int j) { return Ab[(int64_t)i * P + j]; })) {
    sw = softabs_jacobi(w, P, lane, a);
    softabs_emit(w, P, lane, a, [&](int i, int j, double v, bool on) {
      if (on) {
        Ob[(int64_t)i * P + j] = (T)v;
        Ob[(int64_t)j * P + i] = (T)v;
      }
    });
  } else {
    for (int j = 0; j < P; ++j)
      for (int i = j + lane; i < P; i += WAVE) {
        const T v = Ab[(int64_t)i * P + j];
        Ob[(int64_t)i * P + j] = v;
        Ob[(int64_t)j * P + i] = v;
      }
  }
  if (sweeps && lane == 0) sweeps[blockIdx.x] = sw;
}

int ey_generic_softabs(const void* A, int64_t B, int P, int dtype, double a, void* out, void* sweeps, hipStream_t s) {
  const size_t bytes = softabs_work_bytes(P);
  if (dtype == EY_F32)
    return launch(k_softabs<float>, B, 1, bytes, s, (const float*)A, (float*)out, (int*)sweeps, P, a);
  return launch(k_softabs<double>, B, 1, bytes, s, (const double*)A, (double*)out, (int*)sweeps, P, a);
}

// ----------------------------------------------------------------------------------------------- adaptive Metropolis
// AM.draw (eeyore/samplers/am.py:61-107; Haario et al. 2001) with the transform cov -> cov + eps I fused,
// or, in the TR = EY_AM_SOFTABS instantiation, the transform softabs(cov, a): the adaptation then writes the raw covariance
// into the work triangle and the wave transforms it there.  That instantiation lays its LDS out as position and state,
// the AM block, then the evaluation's scratch; the dense f64 work matrix of the section above shares the scratch's place
// (nothing of an evaluation lives between two of them), so the launch needs the larger of the two.
// n = idx + 1 - offset.  Proposal: theta + c z while n <= t0; afterwards one more uniform u_mix picks theta + c z
// (u_mix < l) or theta + (b L) z with L = chol(cov).  Accept as MH does; num_accepted counts accepts of idx > 0.  Then,
// accepted or not:  mean <- ((n - 1) mean + theta) / n,  cov_sum <- cov_sum + theta theta^T,  and from n >= t0 on
// cov <- cov0' while num_accepted == 0, else (cov_sum - n mean mean^T) / (n - 1) + eps I -- the reference's order of
// operations in the working dtype.
// One wave per chain, lane <-> row (rows lane and lane + 64: P <= 128), as k_ram.  LDS after the MH image: two packed
// lower triangles in ram_col order -- cov_sum, and a work triangle that holds cov and is factorised IN PLACE only in a draw
// that takes the L z branch (such a draw has n > t0, so its adaptation rebuilds the triangle: between draws it is
// always cov) -- then running_mean, z and a slot per lane for the stores of rows above a column.  l.gr keeps the current
// state (eval_target<GRAD = false> never touches it).  cov_sum, running_mean and cov are read once per launch from dense
// row-major global state and written back once at its end; only j <= i is touched.
// Factorisation: left-looking column Cholesky.  For column j lane i >= j forms A[i,j] - sum_{k<j} L[i,k] L[j,k] (L[j,k]
// one address for the wave, L[i,k] consecutive along a column), the pivot is broadcast from its lane, tested, and the
// column scaled by the reciprocal of its root.  A pivot that is not > 0 (NaN included) is a breakdown: the draw proposes
// theta + c z, the chain's breakdown counter grows by one, and the adaptation repairs the triangle.
__host__ __device__ static size_t am_extra_bytes(int P, size_t esz) {
  const size_t packed = ((size_t)P * (P + 1) / 2 + 3) & ~(size_t)3, Ppad = (P + 3) & ~3;
  return esz * (2 * packed + 2 * Ppad + WAVE);
}

// The LDS of k_am: the MH image, then the AM block (the Ridge instantiation); or position and state, the AM block, then the
// evaluation's scratch -- activations and deltas, dead between two evaluations -- whose place the f64 work matrix of softabs
// shares (the softabs instantiation: the launch needs the larger of the two).
template <typename T, int TR>
__device__ inline Lds<T> am_carve(const EyModel& m, unsigned char* smem) {
  Lds<T> l = carve<T>(m, smem, 2);
  if constexpr (TR == EY_AM_SOFTABS) {
    l.act = reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(l.act) + am_extra_bytes(m.P, sizeof(T)));
    l.dl = l.act + m.hrows * TS;
  }
  return l;
}

template <typename T, class TINY, int TR = EY_AM_RIDGE>
__global__ void __launch_bounds__(WAVE) k_am(EyModel m, T* theta, T* target, EyAm am, const T* temp, uint64_t seed,
                                             uint64_t iter0, uint64_t chain_offset, unsigned char* accepted,
                                             T* log_rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = am_carve<T, TR>(m, smem);
  const int P = m.P;
  const size_t packed = ((size_t)P * (P + 1) / 2 + 3) & ~(size_t)3;
  const int Ppad = (P + 3) & ~3;
  T* CS = reinterpret_cast<T*>(smem + (TR == EY_AM_SOFTABS ? sizeof(T) * 2 * Ppad : lds_bytes(m, 2, sizeof(T))));
  T* W = CS + packed;
  T* mean = W + packed;
  T* zs = mean + Ppad;
  T* junk = zs + Ppad;
  T* cur = l.gr;
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const int R = P > WAVE ? 2 : 1;  // rows per lane
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T* CSg = static_cast<T*>(am.cov_sum) + c * (int64_t)P * P;
  T* Wg = static_cast<T*>(am.cov) + c * (int64_t)P * P;
  T* mg = static_cast<T*>(am.mean) + c * (int64_t)P;
  const T* c0g = static_cast<const T*>(am.cov0) + (am.cov0_per_chain ? c * (int64_t)P * P : 0);
  const T* z_in = static_cast<const T*>(am.z);
  const T* umix_in = static_cast<const T*>(am.u_mix);
  const T* u_in = static_cast<const T*>(am.u);
  const T lT = (T)am.l, bT = (T)am.b, cT = (T)am.c, epsT = (T)am.eps;
  for (int j = 0; j < P; ++j)
    for (int i = j + lane; i < P; i += WAVE) {
      CS[ram_col(j, P) + i - j] = CSg[(int64_t)i * P + j];
      W[ram_col(j, P) + i - j] = Wg[(int64_t)i * P + j];
    }
  for (int i = lane; i < P; i += WAVE) {
    mean[i] = mg[i];
    cur[i] = theta[c * P + i];
  }
  T t_state = target[c];
  int nacc = am.num_accepted[c];
  int nbreak = am.breakdowns[c];
  int branch = 0;
  __syncthreads();
  for (int it = 0; it < run.n_iters; ++it) {
    const uint64_t iter = iter0 + (uint64_t)it;
    const int64_t idx = am.idx + it;
    const int64_t n = idx + 1 - am.offset;
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    EY_READ_Z(zs);  // am.py:67
    branch = 0;
    if (n > am.t0) {  // :68-73: the mixture uniform is drawn only here
      const T um = umix_in ? umix_in[c] : ey_rng_uniform_at<T>(ru, 1u);
      branch = um < lT ? 0 : 1;
    }
    if (branch == 1) {
      // ---- W <- chol(W), column by column; every quantity that steers the loop is wave-uniform
      const T* ck0 = W;
      bool ok = true;
      for (int j = 0; j < P; ++j) {
        T* colj = W + ram_col(j, P) - j;
        T sum[2] = {T(0), T(0)};
        const T* colk = ck0;
        for (int k = 0; k < j; ++k) {
          const T ljk = colk[j];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            if (r >= R) break;  // wave-uniform: P <= 64 has no second row
            const int i = lane + r * WAVE;
            const bool on = i >= j && i < P;
            const T lik = colk[on ? i : j];
            sum[r] += lik * ljk;
          }
          colk += P - k - 1;
        }
        T s[2] = {T(0), T(0)};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (r >= R) break;  // wave-uniform: P <= 64 has no second row
          const int i = lane + r * WAVE;
          const bool on = i >= j && i < P;
          s[r] = colj[on ? i : j] - sum[r];
        }
        const T d = __shfl(j >= WAVE ? s[1] : s[0], j & (WAVE - 1), WAVE);
        if (!(d > T(0))) {
          ok = false;
          break;
        }
        const T piv = Num<T>::sqrt(d);
        const T rp = T(1) / piv;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (r >= R) break;  // wave-uniform: P <= 64 has no second row
          const int i = lane + r * WAVE;
          const bool on = i >= j && i < P;
          const T v = i == j ? piv : s[r] * rp;
          *(on ? colj + i : junk + lane) = v;
        }
        __syncthreads();
      }
      if (!ok) {
        branch = 2;
        nbreak += 1;
      }
    }
    if (branch == 1) {  // theta + (b L) z (:73): a column sweep, one running sum per row
      T acc[2] = {T(0), T(0)};
      EY_TRIL_SWEEP(W, zs, R, bT, acc);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r >= R) break;  // wave-uniform: P <= 64 has no second row
        const int i = lane + r * WAVE;
        if (i < P) l.th[i] = cur[i] + acc[r];
      }
    } else {
      for (int i = lane; i < P; i += WAVE) l.th[i] = cur[i] + cT * zs[i];  // :70, :75 -- k_mh's proposal with scale c
    }
    __syncthreads();
    const T tv = eval_target<T, false, TINY>(m, l, l.th, cur, ht, tc, nullptr, nullptr);
    const T log_rate = tv - t_state;  // :78
    const T u = u_in ? u_in[c] : ey_rng_uniform<T>(ru);
    const bool acc_ = Num<T>::log(u) < log_rate;  // :80; a NaN log-rate rejects
    if (acc_) {
      t_state = tv;
      if (idx > 0) nacc += 1;  // :85 looks at the absolute index
      for (int i = lane; i < P; i += WAVE) {
        const T v = l.th[i];
        cur[i] = v;
        theta[c * P + i] = v;
      }
    }
    // ---- adaptation (:91-101), accepted or not
    const T nT = (T)n, n1T = (T)(n - 1);
    for (int i = lane; i < P; i += WAVE) mean[i] = (n1T * mean[i] + cur[i]) / nT;
    __syncthreads();  // the state and the mean of every row are visible
    EY_RECORD_SAMPLE(true, i, cur[i]);
    record_draw<T>(lane == 0, c, it, C, acc_, tv, t_state, log_rate, target, accepted, log_rate_o, run);
    const int rebuild = n >= am.t0 ? (nacc == 0 ? 1 : 2) : 0;
    T ti[2], mi[2];
    for (int r = 0; r < 2; ++r) {
      const int i = lane + r * WAVE;
      ti[r] = cur[i < P ? i : 0];
      mi[r] = mean[i < P ? i : 0];
    }
    for (int j = 0; j < P; ++j) {
      const T tj = cur[j], mj = mean[j];
      T* cs = CS + ram_col(j, P) - j;
      T* w = W + ram_col(j, P) - j;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r >= R) break;  // wave-uniform: P <= 64 has no second row
        const int i = lane + r * WAVE;
        const bool on = i >= j && i < P;
        const int ii = on ? i : j;
        const T sv = cs[ii] + ti[r] * tj;  // :94
        T* dst = on ? cs + i : junk + lane;
        *dst = sv;
        if (rebuild) {
          T wv;
          if (rebuild == 1) wv = c0g[(int64_t)ii * P + j];                         // :97
          else if constexpr (TR == EY_AM_RIDGE) wv = (sv - nT * (mi[r] * mj)) / n1T + (ii == j ? epsT : T(0));  // :59, then the ridge
          else wv = (sv - nT * (mi[r] * mj)) / n1T;  // :59 as it is: the wave transforms the triangle below
          T* dw = on ? w + i : junk + lane;
          *dw = wv;
        }
      }
    }
    __syncthreads();
    if constexpr (TR == EY_AM_SOFTABS) {
      // W <- softabs(W, a), a = am.eps; a covariance with an entry that is not finite stays as it is (the next
      // factorisation reports it)
      const SoftabsWork sw = softabs_carve(reinterpret_cast<unsigned char*>(l.act), P);
      if (rebuild == 2 && softabs_fill(sw, P, lane, [&](int i, int j) { return W[ram_col(j, P) + i - j]; })) {
        softabs_jacobi(sw, P, lane, am.eps);
        softabs_emit(sw, P, lane, am.eps, [&](int i, int j, double v, bool on) {
          *(on ? W + ram_col(j, P) + i - j : junk + lane) = (T)v;
        });
        __syncthreads();
      }
    }
  }
  for (int j = 0; j < P; ++j)
    for (int i = j + lane; i < P; i += WAVE) {
      CSg[(int64_t)i * P + j] = CS[ram_col(j, P) + i - j];
      Wg[(int64_t)i * P + j] = W[ram_col(j, P) + i - j];
    }
  for (int i = lane; i < P; i += WAVE) mg[i] = mean[i];
  if (lane == 0) {
    am.num_accepted[c] = nacc;
    am.breakdowns[c] = nbreak;
    if (am.branch) am.branch[c] = (unsigned char)branch;
  }
}

template <typename T, class TINY>
static int launch_am(ey_plan* pl, void* theta, void* target, const EyAm& am, const EyDraw& d) {
  return launch(k_am<T, TINY>, d.C, 1, ey_generic_am_lds(pl), d.s, pl->m, (T*)theta, (T*)target, am, EY_DRAW_ARGS(T, d));
}

template <typename T, class TINY>
static int launch_am_softabs(ey_plan* pl, void* theta, void* target, const EyAm& am, const EyDraw& d) {
  return launch(k_am<T, TINY, EY_AM_SOFTABS>, d.C, 1, ey_generic_am_lds(pl, EY_AM_SOFTABS), d.s, pl->m, (T*)theta,
                (T*)target, am, EY_DRAW_ARGS(T, d));
}

size_t ey_generic_am_lds(const ey_plan* pl, int transform) {
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  const size_t bytes = lds_bytes(pl->m, 2, esz) + am_extra_bytes(pl->m.P, esz);
  if (transform != EY_AM_SOFTABS) return bytes;
  // the f64 work matrix of softabs shares the place of the evaluation's scratch (see k_am)
  const size_t vectors = esz * 2 * (size_t)((pl->m.P + 3) & ~3);
  const size_t eval_scratch = lds_bytes(pl->m, 2, esz) - vectors;
  return vectors + am_extra_bytes(pl->m.P, esz) + std::max(eval_scratch, softabs_work_bytes(pl->m.P));
}

int ey_generic_am(ey_plan* pl, void* theta, void* target, const EyAm& am, const EyDraw& d, int transform) {
  if (transform == EY_AM_SOFTABS) {
    if (int rc = tril_limits(pl, "AM with softabs", "the covariance",
                             "the two covariance triangles, the f64 work matrix of softabs",
                             ey_generic_am_lds(pl, EY_AM_SOFTABS)))
      return rc;
    return EY_TINY_DISPATCH(tiny_dispatch, launch_am_softabs, pl, theta, target, am, d);
  }
  if (int rc = tril_limits(pl, "AM", "the covariance", "the two covariance triangles", ey_generic_am_lds(pl))) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_am, pl, theta, target, am, d);
}

bool ey_generic_am_softabs_fits(const ey_plan* pl) {
  return pl->m.P <= RAM_MAX_P && ey_generic_am_lds(pl, EY_AM_SOFTABS) <= 160 * 1024;
}
#endif  // EY_GEN_PART == 0
