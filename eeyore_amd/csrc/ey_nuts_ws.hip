// k_nuts_ws: k_nuts (ey_nuts.hip) under a DIAGONAL metric with the tree's vectors in a caller-provided device workspace
// instead of LDS, so that P is bounded by the evaluation image alone (include/eeyore_amd_nuts_tree.h).  A
// translation unit of its own beside ey_nuts.hip, on the same share of ey_generic.hip (EY_GEN_PART 1).  The text of the draw
// is k_nuts's, copied statement for statement (sharing it would have meant rewriting that kernel's text): the same Philox
// words, the same per-lane partial sums through wave_sum, the same epilogues.
#define EY_GEN_PART 1
#include "ey_generic.hip"

#include <limits>

#include "ey_nuts.h"

// LDS holds k_hmc_metric's diagonal image only: theta, the gradient, v, the scales and the model's image.  The workspace of
// chain c is nvec = 12 + 2 max_depth vectors of Ppad = P rounded up to 64 elements at ws + c nvec Ppad, in k_nuts's order:
//   the two edges (theta, v, g each), the tree's proposal and the new subtree's candidate (theta, g each), rho, rho',
//   and max_depth checkpoints (v, rho').
// THE LANE-OWNERSHIP RULE: element i of a workspace vector is read and written by lane i mod 64 alone -- every access is an
// elementwise `for (i = lane; ...; i += WAVE)` loop -- so a lane only ever reads back its own stores: no fence, no
// cross-lane visibility is needed of global memory.  Hence no EY_LANE_PASS over a workspace vector (its idle lanes read
// element P - 1, another lane's).  The criterion's sums instead run Ppad / 64 full rounds over the padded vectors, whose
// elements [P, Ppad) this kernel zeroes at the start of every draw, each by its owner: a padded term is x * 0, as an idle
// lane's is in k_nuts.  The proposal is copied into the image before the epilogues read it.  Nothing depends on what the
// workspace holds at entry.
__host__ __device__ static int nuts_ws_ppad(int P) { return (P + WAVE - 1) & ~(WAVE - 1); }
__host__ __device__ static int nuts_ws_nvec(int max_depth) { return 12 + 2 * max_depth; }

// log(exp(a) + exp(b)), branch for branch as numpy's logaddexp (a = b covers two infinities of one sign)
template <typename T>
__device__ __forceinline__ T nuts_logaddexp(T a, T b) {
  if (a == b) return a + T(0.693147180559945309417232121458176568);
  const T d = a - b;
  if (d > T(0)) return a + Num<T>::log1p(Num<T>::exp(-d));
  if (d <= T(0)) return b + Num<T>::log1p(Num<T>::exp(d));
  return d;  // NaN
}

// a wave-uniform decision as a scalar
#define NUTS_UNIFORM(cond) (__builtin_amdgcn_readfirstlane((cond) ? 1 : 0) != 0)
// the uniform at block word `word` of the draw: the caller's table, or the chain's stream.  Reads: T, u_in, S_u, c, ru.
#define NUTS_U(word) (u_in ? u_in[c * S_u + (int64_t)(word)] : ey_rng_uniform_at<T>(ru, (uint32_t)(word)))
// a . rho > 0 and b . rho > 0 with `a_i`, `b_i`, `rho_i` expressions in i (a workspace index, below Ppad) and il (i clamped
// to P - 1, for a vector in LDS): k_nuts's partial sums in Ppad / 64 full rounds.  rho_i is made of padded workspace vectors,
// so a lane without an element in the last round adds x * 0 as it does in k_nuts.  DECLARES `ok`.  Reads: T, P, Ppad, lane.
#define NUTS_WS_CRITERION(ok, a_i, b_i, rho_i)                                          \
  bool ok;                                                                              \
  do {                                                                                  \
    T ey_sa_ = T(0), ey_sb_ = T(0);                                                     \
    for (int ey_k_ = 0, i = lane; ey_k_ < Ppad / WAVE; ++ey_k_, i += WAVE) {            \
      const int il = i < P ? i : P - 1;                                                 \
      (void)il;                                                                         \
      const T ey_rz_ = (rho_i);                                                         \
      ey_sa_ += (a_i) * ey_rz_;                                                         \
      ey_sb_ += (b_i) * ey_rz_;                                                         \
    }                                                                                   \
    ey_sa_ = wave_sum(ey_sa_);                                                          \
    ey_sb_ = wave_sum(ey_sb_);                                                          \
    ok = NUTS_UNIFORM(ey_sa_ > T(0) && ey_sb_ > T(0));                                  \
  } while (0)

template <typename T, class TINY>
__global__ void __launch_bounds__(WAVE) k_nuts_ws(EyModel m, T* theta, T* target, T* grad, const T* metric, int64_t G,
                                                  const int* metric_index, const T* v0, const T* u_in, int64_t S_u, T step,
                                                  T* step_vec, int max_depth, int recompute, EyNuts nu, EyWarm w, T* ws,
                                                  const T* temp, uint64_t seed, uint64_t iter0, uint64_t chain_offset,
                                                  unsigned char* accepted, T* rate_o, EyRun run, int64_t C) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int FORM = EY_METRIC_DIAG;  // (what EY_METRIC_KICK / EY_METRIC_DRIFT read)
  const Lds<T> l = carve<T>(m, smem, 4);
  const int P = m.P;
  const int Ppad = nuts_ws_ppad(P);
  T* S = nullptr;  // (named by the dense branch of the two macros, which is discarded)
  T* sd = l.b;     // the scales
  T* v = l.a;
  const int R = 1;
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  T* nv = ws + c * ((int64_t)nuts_ws_nvec(max_depth) * Ppad);
  T* e_left = nv;               // an edge: theta, then v at + Ppad, g at + 2 Ppad
  T* e_right = nv + 3 * Ppad;
  T* p_th = nv + 6 * Ppad;   // the tree's proposal
  T* p_g = nv + 7 * Ppad;
  T* c_th = nv + 8 * Ppad;   // the new subtree's candidate
  T* c_g = nv + 9 * Ppad;
  T* rho = nv + 10 * Ppad;
  T* rhop = nv + 11 * Ppad;
  T* ck = nv + 12 * Ppad;    // checkpoint s: v at ck + 2 s Ppad, rho' at ck + (2 s + 1) Ppad
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T eps0 = step_vec ? step_vec[c] : step;
  EY_CHAIN_INDEX(g, metric_index);
  {
    const T* sg = metric + g * (int64_t)P;
    for (int i = lane; i < P; i += WAVE) sd[i] = sg[i];
  }
  (void)S; (void)sd; (void)R;
  double da[3] = {0.0, 0.0, 0.0};
  if (w.da_state) {
    for (int k = 0; k < 3; ++k) da[k] = w.da_state[3 * c + k];
  }
  double* mean_c = w.mean ? w.mean + c * (int64_t)P : nullptr;
  double* M2_c = w.M2 ? w.M2 + c * (int64_t)P : nullptr;
  const T ninf = -std::numeric_limits<T>::infinity();
  __syncthreads();
  T t_state = target[c];
  for (int it = 0; it < run.n_iters; ++it) {
    const uint64_t iter = iter0 + (uint64_t)it;
    // v ~ N(0, I): k_hmc_metric's draw
    const EyRng rn = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_NORMAL);
    const EyRng ru = ey_rng_make(seed, chain_offset + (uint64_t)c, iter, EY_STREAM_UNIFORM);
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
    const T H0 = -t_state + T(0.5) * kin;
    __syncthreads();
    if (recompute) (void)eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);
    // the padding of every vector a criterion sums over (the edges' v, rho, rho', the checkpoints), by its owner; no
    // other statement stores beyond P
    {
      const int i = Ppad - WAVE + lane;  // this lane's element of the last round
      if (i >= P) {
        e_left[Ppad + i] = T(0); e_right[Ppad + i] = T(0); rho[i] = T(0); rhop[i] = T(0);
        for (int s = 0; s < 2 * max_depth; ++s) ck[(int64_t)s * Ppad + i] = T(0);
      }
    }
    // the tree is the single leaf (theta, v, g): both edges, the proposal, rho
    for (int i = lane; i < P; i += WAVE) {
      const T thi = l.th[i], vi = v[i], gi = l.gr[i];
      e_left[i] = thi; e_right[i] = thi; p_th[i] = thi;
      e_left[Ppad + i] = vi; e_right[Ppad + i] = vi; rho[i] = vi;
      e_left[2 * Ppad + i] = gi; e_right[2 * Ppad + i] = gi; p_g[i] = gi;
    }
    T t_prop = t_state, H_prop = H0, W = T(0), acc_sum = T(0);
    int depth = 0, n = 0;
    bool divergent = false, moved = false;
    while (depth < max_depth) {
      // 1. the direction; the edge it extends becomes the integrator's state.  Backward integrates with -eps: velocities
      //    keep their forward-time sign, nothing is negated
      const bool fwd = NUTS_UNIFORM(!(NUTS_U(1 + 2 * depth) < T(0.5)));
      const T eps = fwd ? eps0 : -eps0;
      T* edge = fwd ? e_right : e_left;
      __syncthreads();
      for (int i = lane; i < P; i += WAVE) {
        l.th[i] = edge[i];
        v[i] = edge[Ppad + i];
        l.gr[i] = edge[2 * Ppad + i];
        rhop[i] = T(0);
      }
      __syncthreads();
      // 2. the new subtree: 2^depth leaves, one leapfrog step each
      T Wp = ninf, t_cand = T(0), H_cand = T(0);
      bool valid = true;
      const int n_leaf = 1 << depth;
      for (int k = 0; k < n_leaf; ++k) {
        EY_METRIC_KICK(T(0.5) * eps);
        EY_METRIC_DRIFT();
        const T t = eval_target<T, true, TINY>(m, l, l.th, l.gr, ht, tc, nullptr, nullptr);
        EY_METRIC_KICK(T(0.5) * eps);
        kin = T(0);
        EY_LANE_PASS(P, i, on) {
          const T vz = on ? v[i] : T(0);
          kin += vz * vz;
        }
        kin = wave_sum(kin);
        const T H = -t + T(0.5) * kin;
        T delta = H0 - H;
        if (!(delta == delta)) delta = ninf;
        if (NUTS_UNIFORM(-delta > T(1000))) {  // a divergent draw
          divergent = true;
          valid = false;
          break;
        }
        Wp = nuts_logaddexp(Wp, delta);
        // reservoir sampling of the subtree's candidate: the first leaf is always taken
        if (NUTS_UNIFORM(NUTS_U(1 + 2 * EY_NUTS_MAX_DEPTH + n) < Num<T>::exp(delta - Wp))) {
          for (int i = lane; i < P; i += WAVE) {
            c_th[i] = l.th[i];
            c_g[i] = l.gr[i];
          }
          t_cand = t;
          H_cand = H;
        }
        for (int i = lane; i < P; i += WAVE) rhop[i] = rhop[i] + v[i];
        const T a1 = Num<T>::exp(delta);
        acc_sum += a1 < T(1) ? a1 : T(1);
        n += 1;
        // the aligned blocks of 2^j leaves that end at k, from the checkpoints
        if ((k & 1) == 0) {
          T* cv = ck + 2 * __popc((unsigned)(k >> 1)) * Ppad;
          for (int i = lane; i < P; i += WAVE) {
            cv[i] = v[i];
            cv[Ppad + i] = rhop[i];
          }
          __syncthreads();
        } else {
          __syncthreads();
          int slot = __popc((unsigned)(k >> 1));
          for (int kk = k; kk & 1; kk >>= 1, --slot) {
            const T* cv = ck + 2 * slot * Ppad;
            NUTS_WS_CRITERION(ok, cv[i], v[il], rhop[i] - cv[Ppad + i] + cv[i]);
            if (!ok) {
              valid = false;
              break;
            }
          }
          if (!valid) break;
        }
      }
      // 3. an invalid subtree is discarded and the draw stops
      if (!valid) break;
      // 4. biased progressive sampling of the tree's proposal; the edge moves; the criterion between the tree's edges
      if (NUTS_UNIFORM(NUTS_U(2 + 2 * depth) < Num<T>::exp(Wp - W))) {
        for (int i = lane; i < P; i += WAVE) {
          p_th[i] = c_th[i];
          p_g[i] = c_g[i];
        }
        t_prop = t_cand;
        H_prop = H_cand;
        moved = true;
      }
      W = nuts_logaddexp(W, Wp);
      for (int i = lane; i < P; i += WAVE) {
        rho[i] = rho[i] + rhop[i];
        edge[i] = l.th[i];
        edge[Ppad + i] = v[i];
        edge[2 * Ppad + i] = l.gr[i];
      }
      depth += 1;
      __syncthreads();
      NUTS_WS_CRITERION(go, e_left[Ppad + i], e_right[Ppad + i], rho[i]);
      if (!go) break;
    }
    // the proposal into the image, each element by its owner: what follows reads it from LDS, where a lane pass may look at
    // another lane's element (the image's theta is reloaded at the top of the next draw)
    __syncthreads();
    for (int i = lane; i < P; i += WAVE) l.th[i] = p_th[i];
    __syncthreads();
    // the state becomes the proposal
    if (moved) {
      t_state = t_prop;
      for (int i = lane; i < P; i += WAVE) {
        theta[c * P + i] = l.th[i];
        grad[c * P + i] = p_g[i];
      }
    }
    const T rate = n > 0 ? acc_sum / (T)n : T(0);
    EY_RECORD_SAMPLE(true, i, l.th[i]);
    record_draw<T>(lane == 0, c, it, C, moved, t_prop, t_state, rate, target, accepted, rate_o, run);
    if (lane == 0) {
      if (nu.depth) nu.depth[c] = depth;
      if (nu.n_leapfrog) nu.n_leapfrog[c] = n;
      if (nu.divergent) nu.divergent[c] = divergent ? 1 : 0;
      if (nu.energy) static_cast<T*>(nu.energy)[c] = H_prop;
      if (nu.depth_rec) nu.depth_rec[(int64_t)it * C + c] = depth;
      if (nu.div_rec) nu.div_rec[(int64_t)it * C + c] = divergent ? 1 : 0;
      if (w.steps_rec) static_cast<T*>(w.steps_rec)[(int64_t)it * C + c] = eps0;
      if (w.rate_rec) static_cast<T*>(w.rate_rec)[(int64_t)it * C + c] = rate;
    }
    // the two epilogues of k_nuts in their diagonal form, copied, on rate := the draw's mean accept statistic and x := the
    // state the chain is left in, which is the proposal (now in l.th)
    if (w.da_state && it < w.da_n) {  // wave-uniform
      eps0 = (T)ey_da_update(da, w.da_table + 3 * it, (double)rate, w.d, w.has_eub != 0, w.logeub, it == w.final_it);
      if (lane == 0) step_vec[c] = eps0;
    }
    if (mean_c) {  // wave-uniform
      const double cnt = (double)(w.count + it + 1);
      const double f = (cnt - 1.0) / cnt;
      EY_LANE_PASS(P, i, on) {
        (void)on;
        const double x = (double)l.th[i];
        const double mu = mean_c[i];
        const double dx = x - mu;
        mean_c[i] = mu + dx / cnt;
        M2_c[i] = M2_c[i] + f * (dx * dx);
      }
    }
    __syncthreads();
  }
  if (w.da_state && lane == 0) {
    w.da_state[3 * c] = da[0];
    w.da_state[3 * c + 1] = da[1];
  }
}

// the LDS limit of an instantiation is raised once per plan, as launch_nuts_kernel (ey_nuts.hip) does it
template <typename... Ps, typename... As>
static int launch_nuts_ws_kernel(ey_plan* pl, void (*kernel)(Ps...), int64_t C, size_t bytes, hipStream_t s, As... args) {
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (bytes > 48 * 1024 && pl->nuts_ws_attr != fn) {
    EY_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    pl->nuts_ws_attr = fn;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)C), dim3(WAVE), bytes, s, args...);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

template <typename T, class TINY>
static int launch_nuts_ws(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                          const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                          const EyWarm& w) {
  const size_t bytes = hmc_metric_lds(pl->m, EY_METRIC_DIAG, sizeof(T));
  const int recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) != 0;
  return launch_nuts_ws_kernel(pl, k_nuts_ws<T, TINY>, d.C, bytes, d.s, pl->m, (T*)theta, (T*)target, (T*)grad,
                               (const T*)metric, G, (const int*)metric_index, (const T*)nu.v0, (const T*)nu.u, nu.S, (T)step,
                               (T*)step_vec, nu.max_depth, recompute, nu, w, (T*)pl->nuts_tree, EY_DRAW_ARGS(T, d));
}

int64_t ey_nuts_ws_bytes(const ey_plan* pl, int64_t C, int max_depth) {
  return C * (int64_t)nuts_ws_nvec(max_depth) * nuts_ws_ppad(pl->m.P) * (pl->dtype == EY_F32 ? 4 : 8);
}

// The caller (nuts_impl, ey_api.hip) has checked the form, the attached workspace and its size for this (C, max_depth).
int ey_nuts_ws_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                      const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                      const EyWarm& w) {
  const size_t bytes = hmc_metric_lds(pl->m, EY_METRIC_DIAG, pl->dtype == EY_F32 ? 4 : 8);
  if (bytes > 160 * 1024)
    EY_FAIL(EY_ERR_UNSUPPORTED, "NUTS with a diagonal metric: the model's evaluation image and the scales (" +
                                    std::to_string(bytes) + " bytes) do not fit the 160 KiB LDS of a CU");
  if (!pl->nuts_tree || pl->nuts_tree_bytes < ey_nuts_ws_bytes(pl, d.C, nu.max_depth))  // (never: see above)
    EY_FAIL(EY_ERR_INVALID, "NUTS with the tree in device memory: no workspace of this call's size is attached");
  return EY_TINY_DISPATCH(tiny_dispatch, launch_nuts_ws, pl, theta, target, grad, metric, G, metric_index, step, step_vec,
                          d, nu, w);
}
