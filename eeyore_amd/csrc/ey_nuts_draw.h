// The No-U-Turn draw, written once for k_nuts (ey_nuts.hip: the tree in LDS, both metric forms) and k_nuts_ws
// (ey_nuts_ws.hip: the tree in a device workspace, the diagonal form) -- DESIGN.md 4.24 and 4.27.  Not a header in the
// usual sense: a unit includes it ONCE, after ey_generic.hip (EY_GEN_PART 1), ey_nuts.h and its own size functions, with
//   NUTS_TREE_IN_WS   0: the tree behind the image in LDS.  1: at ws + c nvec Ppad in device memory
//   NUTS_KERNEL_HEAD  the kernel's template head, attributes, name and argument list (k_nuts_ws: T* ws after w)
// defined, and this file writes that kernel's body.  The text is included, not called: this compiler allocates a kernel
// differently around an inlined function, and included text leaves each unit's code as it was.  Every place
// where the two kernels differ is an `#if NUTS_TREE_IN_WS` below and says why; the rest is one text.
//
// Multinomial NUTS, iterative: a subtree of 2^d leaves is one loop over its leaves; the aligned blocks that end at leaf k are
// checked from checkpoints, one per trailing 1-bit of k (an even k stores slot popcount(k >> 1), an odd k reads slots from
// popcount(k >> 1) downward).  Every decision is wave-uniform (the sums are butterfly all-reduces, the uniforms are read by
// every lane) and is moved to a scalar register before it is branched on, so the loops below run under a full EXEC mask.
//
// THE LANE-OWNERSHIP RULE of a tree in device memory: element i of a workspace vector is read and written by lane i mod 64
// alone -- every access is an elementwise `for (i = lane; ...; i += WAVE)` loop -- so a lane only ever reads back its own
// stores: no fence, no cross-lane visibility is needed of global memory.  Hence no EY_LANE_PASS over a workspace vector (its
// idle lanes read element P - 1, another lane's).  Nothing depends on what the workspace holds at entry.
#include <limits>

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

// a . rho > 0 and b . rho > 0, the U-turn criterion between two ends in the whitened velocity: `a_i`, `b_i`, `rho_i` are
// expressions in i (an index into a tree vector) and il (into a vector of the LDS image).  DECLARES `ok`.  Reads: T, P,
// Ppad, lane.
#if NUTS_TREE_IN_WS
// In device memory (the lane-ownership rule): Ppad / 64 full rounds over the padded vectors, i unclamped, il clamped to
// P - 1.  rho_i is made of padded workspace vectors, so a lane without an element in the last round adds x * 0, as an idle
// lane does in the pass below.
#define NUTS_CRITERION_EACH for (int ey_k_ = 0, i = lane; ey_k_ < Ppad / WAVE; ++ey_k_, i += WAVE)
#define NUTS_CRITERION_IL (i < P ? i : P - 1)
#define NUTS_CRITERION_RHO(on, r) (r)
// the v of an edge, element i: THE SPELLINGS DIFFER on purpose.  Each is the association its kernel was written with, and
// this compiler's register allocation follows it through the whole kernel: either spelling in the other kernel changes
// most of that kernel's assembly.
#define NUTS_EDGE_V(e, i) (e)[Ppad + i]
#else
// In LDS: a lane pass, i = il clamped, the idle lanes' rho selected to zero.
#define NUTS_CRITERION_EACH EY_LANE_PASS(P, i, on)
#define NUTS_CRITERION_IL i
#define NUTS_CRITERION_RHO(on, r) ((on) ? (r) : T(0))
#define NUTS_EDGE_V(e, i) ((e) + Ppad)[i]
#endif
#define NUTS_CRITERION(ok, a_i, b_i, rho_i)                 \
  bool ok;                                                  \
  do {                                                      \
    T ey_sa_ = T(0), ey_sb_ = T(0);                         \
    NUTS_CRITERION_EACH {                                   \
      const int il = NUTS_CRITERION_IL;                     \
      (void)il;                                             \
      const T ey_r_ = (rho_i);                              \
      const T ey_rz_ = NUTS_CRITERION_RHO(on, ey_r_);       \
      ey_sa_ += (a_i) * ey_rz_;                             \
      ey_sb_ += (b_i) * ey_rz_;                             \
    }                                                       \
    ey_sa_ = wave_sum(ey_sa_);                              \
    ey_sb_ = wave_sum(ey_sb_);                              \
    ok = NUTS_UNIFORM(ey_sa_ > T(0) && ey_sb_ > T(0));      \
  } while (0)

// One wave per chain, as k_hmc_metric: the evaluation image (th, gr, a = v [, the diagonal scales]) and the packed factor
// where there is one; then the tree, nvec vectors of Ppad elements:
//   the two edges of the tree (theta, v, g each), the tree's proposal and the new subtree's candidate (theta, g each: the
//   gradient is kept with a candidate, nothing is re-evaluated when the draw ends), rho of the tree and of the new subtree,
//   and max_depth checkpoints (v, rho' up to and including the checkpoint's leaf) for the sub-block checks.
NUTS_KERNEL_HEAD {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#if NUTS_TREE_IN_WS
  constexpr int FORM = EY_METRIC_DIAG;  // the only form with the tree in device memory: the dense branches are discarded
#endif
  const Lds<T> l = carve<T>(m, smem, FORM == EY_METRIC_TRIL ? 3 : 4);
  const int P = m.P;
  T* S = reinterpret_cast<T*>(smem + lds_bytes(m, 3, sizeof(T)));  // EY_METRIC_TRIL: the packed factor
  T* sd = l.b;                                                     // EY_METRIC_DIAG: the scales
  T* v = l.a;
  double* dlt = reinterpret_cast<double*>(l.gr);                   // EY_METRIC_TRIL moments: x - mean_old, between draws
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  // (the tree's vectors are declared before R: with R first, k_nuts is allocated differently throughout -- DESIGN.md 4.27)
#if NUTS_TREE_IN_WS
  const int Ppad = nuts_ws_ppad(P);  // whole rounds of the wave: every element, padding included, has one owner
  T* nv = ws + c * ((int64_t)nuts_ws_nvec(max_depth) * Ppad);
#else
  const int Ppad = (P + 3) & ~3;
  T* nv = reinterpret_cast<T*>(smem + hmc_metric_lds(m, FORM, sizeof(T)));
#endif
  T* e_left = nv;               // an edge: theta, then v at + Ppad, g at + 2 Ppad
  T* e_right = nv + 3 * Ppad;
  T* p_th = nv + 6 * Ppad;   // the tree's proposal
  T* p_g = nv + 7 * Ppad;
  T* c_th = nv + 8 * Ppad;   // the new subtree's candidate
  T* c_g = nv + 9 * Ppad;
  T* rho = nv + 10 * Ppad;
  T* rhop = nv + 11 * Ppad;
  T* ck = nv + 12 * Ppad;    // checkpoint s: v at ck + 2 s Ppad, rho' at ck + (2 s + 1) Ppad
  const int R = P > WAVE ? 2 : 1;  // the rows (and columns) of a lane: wave-uniform
  const bool ht = temp != nullptr;
  const T tc = ht ? temp[c] : T(1);
  T eps0 = step_vec ? step_vec[c] : step;
  EY_METRIC_STAGE();
  (void)S; (void)sd; (void)R; (void)dlt;
  double da[3] = {0.0, 0.0, 0.0};
  if (w.da_state) {
    for (int k = 0; k < 3; ++k) da[k] = w.da_state[3 * c + k];
  }
  double* mean_c = w.mean ? w.mean + c * (int64_t)P : nullptr;
  double* M2_c = w.M2 ? w.M2 + c * (FORM == EY_METRIC_TRIL ? (int64_t)P * P : (int64_t)P) : nullptr;
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
#if NUTS_TREE_IN_WS
    // the padding [P, Ppad) of every vector a criterion sums over (the edges' v, rho, rho', the checkpoints) is zeroed, each
    // element by its owner: a padded term of the criterion's full rounds is then x * 0, as an idle lane's is in LDS.  No
    // other statement stores beyond P
    {
      const int i = Ppad - WAVE + lane;  // this lane's element of the last round
      if (i >= P) {
        e_left[Ppad + i] = T(0); e_right[Ppad + i] = T(0); rho[i] = T(0); rhop[i] = T(0);
        for (int s = 0; s < 2 * max_depth; ++s) ck[(int64_t)s * Ppad + i] = T(0);
      }
    }
#endif
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
        EY_KINETIC(kin);
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
            NUTS_CRITERION(ok, cv[i], v[il], rhop[i] - cv[Ppad + i] + cv[i]);
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
      NUTS_CRITERION(go, NUTS_EDGE_V(e_left, i), NUTS_EDGE_V(e_right, i), rho[i]);
      if (!go) break;
    }
#if NUTS_TREE_IN_WS
    // the proposal into the image, each element by its owner: what follows reads it from LDS, where a lane pass may look at
    // another lane's element (the image's theta is reloaded at the top of the next draw)
    __syncthreads();
    for (int i = lane; i < P; i += WAVE) l.th[i] = p_th[i];
    __syncthreads();
    T* x_th = l.th;
#else
    T* x_th = p_th;
#endif
    // the state becomes the proposal
    if (moved) {
      t_state = t_prop;
      for (int i = lane; i < P; i += WAVE) {
        theta[c * P + i] = x_th[i];
        grad[c * P + i] = p_g[i];
      }
    }
    const T rate = n > 0 ? acc_sum / (T)n : T(0);
    EY_RECORD_SAMPLE(true, i, x_th[i]);
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
    // rate := the draw's mean accept statistic; the state the chain is left in is the proposal
    EY_WARM_EPILOGUES(x_th[i], eps0);
    __syncthreads();
  }
  if (w.da_state && lane == 0) {
    w.da_state[3 * c] = da[0];
    w.da_state[3 * c + 1] = da[1];
  }
}
