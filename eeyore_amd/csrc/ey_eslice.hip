// k_eslice: elliptical slice sampling (include/eeyore_amd_eslice.h).  A sibling of k_mh in a translation
// unit of its own, so that it builds beside ey_generic.hip: that file is included for what the kernels share (EY_GEN_PART 1
// there: the evaluation, the LDS image, the records of a draw, the launch helpers) with every entry point and kernel
// instantiation of its own left out.
#define EY_GEN_PART 1
#include "ey_generic.hip"

#include "ey_eslice.h"

// One wave per chain on the generic evaluation, whatever plan.kernel says.  The image is carve(m, smem, 4) (less the delta
// ping-pong, see ey_eslice_lds): th is the point evaluated, and the other three vectors hold x = theta - m (gr: a value-only
// evaluation leaves it alone), nu (a) and the base's location m (b), so a point of the ellipse is one pass over LDS.  The base's scale is read from global memory in lane
// order where it is needed: once per draw for nu, and once per evaluation for the base's quadratic form when the caller
// gave the base.  Every decision is wave-uniform (the sums are butterfly all-reduces, the uniforms are read by every lane)
// and is moved to a scalar register before it is branched on, so the shrink loop runs under a full EXEC mask.

// a wave-uniform decision as a scalar
#define ES_UNIFORM(cond) (__builtin_amdgcn_readfirstlane((cond) ? 1 : 0) != 0)
// the uniform at block word `word` of the draw: the caller's table, or the chain's stream.  Reads: T, u_in, S_u, c, ru.
#define ES_U(word) (u_in ? u_in[c * S_u + (int64_t)(word)] : ey_rng_uniform_at<T>(ru, (uint32_t)(word)))

// angles are kept in turns: cospi / sinpi do the range reduction exactly, as the Box-Muller code of ey_common.h does
__device__ __forceinline__ float es_cospi(float v) { return cospif(v); }
__device__ __forceinline__ double es_cospi(double v) { return cospi(v); }
__device__ __forceinline__ float es_sinpi(float v) { return sinpif(v); }
__device__ __forceinline__ double es_sinpi(double v) { return sinpi(v); }

// ell and the (tempered) log-target at the point in l.th, which the caller has written (and made visible).  Without a base
// ell is the (tempered) log-likelihood; with one it is the log-target minus the base's exponent, sum_i -d_i^2 / 2 with
// d_i = (th_i - m_i) / s_i.  Both are broadcast to every lane.
template <typename T, class TINY>
__device__ __forceinline__ T eslice_ell_at(const EyModel& m, const Lds<T>& l, bool ht, T tc, const T* base_loc,
                                           const T* base_scale, int lane, T* target_out) {
  T lik, prior;
  const T t = eval_target<T, false, TINY>(m, l, l.th, l.gr, ht, tc, &lik, &prior);
  *target_out = t;
  if (!base_loc) return lik;  // (a kernel argument: the branch is scalar)
  T q = T(0);
  EY_LANE_PASS(m.P, i, on) {
    const T d = (l.th[i] - base_loc[i]) / base_scale[i];
    const T dz = on ? d : T(0);
    q += dz * dz;
  }
  q = wave_sum(q);
  return t + T(0.5) * q;
}

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_eslice_ell(EyModel m, const T* theta, const T* base_loc, const T* base_scale,
                                                     const T* temp, T* ell_o, T* target_o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, 4);
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  for (int i = lane; i < m.P; i += WAVE) l.th[i] = theta[c * m.P + i];
  __syncthreads();
  T t;
  const T e = eslice_ell_at<T, TINY>(m, l, ht, tc, base_loc, base_scale, lane, &t);
  if (lane == 0) {
    if (ell_o) ell_o[c] = e;
    if (target_o) target_o[c] = t;
  }
}

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_eslice(EyModel m, T* theta, T* target, T* ell, const T* base_loc,
                                                 const T* base_scale, const T* z_in, const T* u_in, int64_t S_u,
                                                 int max_shrinks, int* n_evals, int* n_evals_rec, const T* temp,
                                                 uint64_t seed, uint64_t iter0, uint64_t chain_offset,
                                                 unsigned char* accepted, T* log_rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds<T> l = carve<T>(m, smem, 4);
  const int P = m.P;
  T* x = l.gr;
  T* nu = l.a;
  T* loc = l.b;
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  const T* gm = base_loc ? base_loc : static_cast<const T*>(m.mu);
  const T* iv = static_cast<const T*>(m.inv_var);
  (void)log_rate_o;
  T t_state = target[c], e_state = ell[c];
  for (int it = 0; it < run.n_iters; ++it) {  // ey_eslice_run: see k_mala
    const uint64_t iter = iter0 + (uint64_t)it;
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
    // 1. nu = s z, x = theta - m.  Without a base s is the prior's sigma / sqrt(t): 1 / sqrt(t / sigma^2)
    //    z goes through th, which is free until the first point is written (k_mh draws its normals there too)
    if (!z_in) {
      fill_normals<T>(l.th, rn, P);
    } else {
      for (int i = lane; i < P; i += WAVE) l.th[i] = z_in[c * P + i];
      __syncthreads();
    }
    EY_LANE_PASS(P, i, on) {
      (void)on;
      const T mi = gm[i];
      const T si = base_scale ? base_scale[i] : T(1) / Num<T>::sqrt(ht ? iv[i] * tc : iv[i]);
      loc[i] = mi;
      x[i] = theta[c * P + i] - mi;
      nu[i] = si * l.th[i];
    }
    __syncthreads();
    int n = 0;
    bool moved = false;
    T t_new = t_state, e_new = e_state;
    // 5. a chain whose carried ell is not finite stays put without evaluating
    if (ES_UNIFORM(e_state - e_state == T(0))) {
      // 2. the slice height; 3. the first angle and its bracket
      const T logy = e_state + Num<T>::log(ES_U(0));
      T a = ES_U(1);
      T lo = a - T(1), hi = a;
      for (int k = 0;; ++k) {
        const T ca = es_cospi(T(2) * a), sa = es_sinpi(T(2) * a);
        EY_LANE_PASS(P, i, on) {
          (void)on;
          l.th[i] = loc[i] + x[i] * ca + nu[i] * sa;
        }
        __syncthreads();
        T t;
        const T e = eslice_ell_at<T, TINY>(m, l, ht, tc, base_loc, base_scale, lane, &t);
        n += 1;
        if (ES_UNIFORM(e > logy)) {  // (a NaN compares false)
          moved = true;
          t_new = t;
          e_new = e;
          break;
        }
        if (k == max_shrinks) break;  // the bracket is exhausted: the chain stays
        if (a < T(0)) lo = a; else hi = a;
        a = lo + (hi - lo) * ES_U(2 + k);
      }
    }
    // (two loops, not one select: `moved` is uniform, and a select between an LDS and a global address becomes a flat one)
    if (moved) {
      t_state = t_new;
      e_state = e_new;
      for (int i = lane; i < P; i += WAVE) theta[c * P + i] = l.th[i];
      EY_RECORD_SAMPLE(true, i, l.th[i]);
    } else {
      EY_RECORD_SAMPLE(true, i, theta[c * P + i]);
    }
    record_draw<T>(lane == 0, c, it, C, moved, t_new, t_state, T(0), target, accepted, (T*)nullptr, run);
    if (lane == 0) {
      if (moved) ell[c] = e_state;
      if (n_evals) n_evals[c] = n;
      if (n_evals_rec) n_evals_rec[(int64_t)it * C + c] = n;
    }
    __syncthreads();
  }
}

// The image of carve(m, smem, 4) without its last region, the delta ping-pong (l.dl): only the backward pass of an
// evaluation touches it, and this kernel makes value-only evaluations alone.  The pointer carve() computes for it lies
// beyond the allocation and is never dereferenced.
size_t ey_eslice_lds(const ey_plan* pl) {
  const size_t esz = pl->dtype == EY_F32 ? 4 : 8;
  return lds_bytes(pl->m, 4, esz) - esz * 2 * (size_t)pl->m.dmax * TS;
}

static int eslice_limits(const ey_plan* pl) {
  const size_t bytes = ey_eslice_lds(pl);
  if (bytes > 160 * 1024)
    EY_FAIL(EY_ERR_UNSUPPORTED, "elliptical slice sampling: the model's evaluation image and three vectors (" +
                                    std::to_string(bytes) + " bytes) do not fit the 160 KiB LDS of a CU");
  return EY_OK;
}

template <typename T, class TINY>
static int launch_eslice(ey_plan* pl, void* theta, void* target, const EyEslice& es, const EyDraw& d) {
  return launch(k_eslice<T, TINY>, d.C, 1, ey_eslice_lds(pl), d.s, pl->m, (T*)theta, (T*)target, (T*)es.ell,
                (const T*)es.base_loc, (const T*)es.base_scale, (const T*)es.z, (const T*)es.u, es.S, es.max_shrinks,
                es.n_evals, es.n_evals_rec, EY_DRAW_ARGS(T, d));
}

int ey_eslice_launch(ey_plan* pl, void* theta, void* target, const EyEslice& es, const EyDraw& d) {
  if (int rc = eslice_limits(pl)) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_eslice, pl, theta, target, es, d);
}

template <typename T, class TINY>
static int launch_eslice_ell(ey_plan* pl, const void* theta, const void* base_loc, const void* base_scale,
                             const void* temp, int64_t C, void* ell, void* target, hipStream_t s) {
  return launch(k_eslice_ell<T, TINY>, C, 1, ey_eslice_lds(pl), s, pl->m, (const T*)theta, (const T*)base_loc,
                (const T*)base_scale, (const T*)temp, (T*)ell, (T*)target);
}

int ey_eslice_ell_launch(ey_plan* pl, const void* theta, const void* base_loc, const void* base_scale, const void* temp,
                         int64_t C, void* ell, void* target, hipStream_t s) {
  if (int rc = eslice_limits(pl)) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_eslice_ell, pl, theta, base_loc, base_scale, temp, C, ell, target, s);
}
