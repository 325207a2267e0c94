// k_nuts_mfma: multinomial NUTS under a DIAGONAL metric (include/eeyore_amd_nuts_fused.h) on the matrix cores
// for the MLP(4-32-32-dK) plans that ey_mfma32.hip serves.  The draw of ey_nuts_draw.h, decision for
// decision, in the frame of k_mfma32: one wave per chain, eight chains per persistent workgroup, chain-major; the data image
// shared in LDS, a region of LDS per wave; theta, v and g in the lane's Vec register layout, exactly the set run_chain holds
// for HMC; every leaf evaluated by the fused evaluation with its gradient.  ey_mfma32.hip is included for all of that
// (EY_MF_PART 2 there: every entry point and kernel instantiation of its own left out).  The tree lives in the workspace of
// k_nuts_ws (ey_nuts_ws.hip), in its layout: nvec = 12 + 2 max_depth vectors of Ppad elements at ws + chain nvec Ppad, indexed
// by canonical parameter index.
//
// THE LANE-OWNERSHIP RULE here: a lane loads from the workspace only addresses it has itself stored in this draw.  Every
// access is a for_each pass, which gives a lane the same canonical indices every time.  Replicas (the two halves of the wave
// for W0, W2, b0, b1; every lane for b2) store the same bits to the same address, as the state write-back of k_mfma32 does.
// No memory operation sits behind a per-lane branch; the padding [P, Ppad) is never touched.  There is no
// workgroup barrier below the chain loop: the waves of a workgroup leave their trees at different leaves.
#define EY_MF_PART 2
#include "ey_mfma32.hip"

#include <limits>

#include "ey_nuts.h"

// a wave-uniform decision as a scalar
#define NM_UNIFORM(cond) (__builtin_amdgcn_readfirstlane((cond) ? 1 : 0) != 0)
// Lane coordinates the compiler cannot identify with those of kernel entry (run_chain's remedy): the element offsets of the
// passes over global memory depend on the lane alone, and left to the compiler all of them are computed once, kept across
// every evaluation and spilled.  Made opaque where a pass begins they are recomputed there and die with it.
#define NM_LANE(le, ce, he)    \
  int le = lane;               \
  asm volatile("" : "+v"(le)); \
  const int ce = le & 31, he = le >> 5

// What the kernel takes beside MfArgs (which carries the state, the step, the temperatures, the Philox key, the records of a
// run and the accept statistic's output as `rate`).
struct NmArgs {
  const float* metric;      // [G, P] scales
  int64_t G;
  const int* metric_index;  // [C] or null
  const float* v0;          // [C, P] or null
  const float* u;           // [C, S] or null
  int64_t S;
  float* step_vec;          // [C] or null; in/out under a dual averaging
  int max_depth;
  float* ws;                // the tree: [C, nvec, Ppad]
  int* depth;
  int* n_leapfrog;
  unsigned char* divergent;
  float* energy;
  int* depth_rec;
  unsigned char* div_rec;
  EyWarm w;
};
struct NmKernArgs {
  MfArgs A;
  NmArgs N;
};
typedef const __attribute__((address_space(4))) NmKernArgs NmKArgs;
typedef const __attribute__((address_space(4))) NmArgs NmNArgs;

// The arguments re-read from the kernarg segment (k_mfma32's remedy): taken once per draw they all stay live in scalar
// registers across the tree, and the allocator spills scalars into vector registers.
__device__ __forceinline__ NmKArgs& nm_args() {
  NmKArgs* Kp = (NmKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(Kp));
  return *Kp;
}
// the uniform at block word `word` of the draw: the caller's table, or the chain's stream (NUTS_U of ey_nuts_draw.h)
__device__ __forceinline__ float nm_uniform(NmKArgs& K, int64_t chain, int it, int word) {
  if (K.N.u) return K.N.u[chain * K.N.S + word];
  const EyRng ru = ey_rng_make(K.A.seed, K.A.chain_offset + (uint64_t)chain, K.A.iter + (uint64_t)it, EY_STREAM_UNIFORM);
  return ey_rng_uniform_at<float>(ru, (uint32_t)word);
}
// the chain's row of the metric table (EY_CHAIN_INDEX): the scales are read from it where a kick or a drift needs them (the
// table is L2-resident; held in registers beside theta, v and g it would send the tile loop to scratch)
__device__ __forceinline__ const float* nm_scales(NmNArgs& N, int64_t chain, int npar) {
  int64_t g = N.G == 1 ? 0 : (N.metric_index ? (int64_t)N.metric_index[chain] : chain);
  g = g < 0 ? 0 : (g > N.G - 1 ? N.G - 1 : g);
  return N.metric + g * npar;
}
// log(exp(a) + exp(b)), branch for branch as nuts_logaddexp (ey_nuts_draw.h)
__device__ __forceinline__ float nm_logaddexp(float a, float b) {
  if (a == b) return a + 0.693147180559945309417232121458176568f;
  const float d = a - b;
  if (d > 0.0f) return a + log1pf(expf(-d));
  if (d <= 0.0f) return b + log1pf(expf(d));
  return d;  // NaN
}

// All draws of one chain of one launch.
template <int BF3, typename SH>
__device__ __forceinline__ void nm_chain(const float* xs, float* lw, const int64_t chain, const int c, const int h,
                                         const int lane, Pace& pc) {
  constexpr int DKV = SH::DK;
  typedef Vec<DKV> Vec;
  constexpr int Ppad = (NPAR + 63) & ~63;  // nuts_ws_ppad
  const float ninf = -std::numeric_limits<float>::infinity();
  float t_state, eps0;
  double da[3] = {0.0, 0.0, 0.0};
  int n_iters;
  {
    NmKArgs& K = nm_args();
    t_state = K.A.target[chain];
    eps0 = K.N.step_vec ? K.N.step_vec[chain] : K.A.step;
    if (K.N.w.da_state) {
      for (int k = 0; k < 3; ++k) da[k] = K.N.w.da_state[3 * chain + k];
    }
    n_iters = K.A.n_iters;
  }
#pragma unroll 1
  for (int it = 0; it < n_iters; ++it) {
    // (run_chain's fences: later iterations read what this wave's lanes wrote at the end of the one before)
    if (it > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    Vec th, v, g;
    W1Lo wl;
    float H0;
    bool has_temp;
    float temp;
    int max_depth;
    {
      NmKArgs& K = nm_args();
      KArgs& A = K.A;
      NmNArgs& N = K.N;
      has_temp = A.temp != nullptr;
      temp = has_temp ? A.temp[chain] : 1.0f;
      max_depth = N.max_depth;
      // v ~ N(0, I): the table, or the chain's stream as k_mfma32 stages it
      const EyRng rn = ey_rng_make(A.seed, A.chain_offset + (uint64_t)chain, A.iter + (uint64_t)it, EY_STREAM_NORMAL);
      const float* vin = N.v0 ? N.v0 + chain * NPAR : nullptr;
      const float* vst = vin ? nullptr : stage_normals<BF3, DKV>(lw, rn, lane);
      const float* thg = A.theta + chain * NPAR;
      const float* grg = A.grad + chain * NPAR;
      float kin = 0.0f;
      for_each3(th, v, g, c, h, lane, [&](float& tv, float& vv, float& gv, int idx, bool counts) {
        tv = thg[idx];
        gv = grg[idx];
        vv = vin ? vin[idx] : vst[idx];
        if (counts) kin += vv * vv;
      });
      wave_lds_fence();  // the staged normals have been read; the evaluations reuse that LDS
      kin = wsum(kin);
      H0 = -t_state + 0.5f * kin;
      if (A.recompute) {
        write_images<BF3, SH>(lw, th, c, h, lane, wl);
        (void)eval_any<0, false, BF3, SH, true>(A, xs, lw, th, g, has_temp, temp, c, h, lane, true, pc, wl);
      }
    }
    // the tree is the single leaf (theta, v, g): both edges, the proposal, rho
    {
      float* nv = nm_args().N.ws + chain * (int64_t)((12 + 2 * max_depth) * Ppad);
      NM_LANE(le, ce, he);
      for_each3(th, v, g, ce, he, le, [&](float& tv, float& vv, float& gv, int idx, bool) {
        nv[idx] = tv; nv[3 * Ppad + idx] = tv; nv[6 * Ppad + idx] = tv;
        nv[Ppad + idx] = vv; nv[4 * Ppad + idx] = vv; nv[10 * Ppad + idx] = vv;
        nv[2 * Ppad + idx] = gv; nv[5 * Ppad + idx] = gv; nv[7 * Ppad + idx] = gv;
      });
    }
    float t_prop = t_state, H_prop = H0, W = 0.0f, acc_sum = 0.0f;
    int depth = 0, n = 0;
    bool divergent = false, moved = false;
#pragma unroll 1
    while (depth < max_depth) {
      // 1. the direction; the edge it extends becomes the integrator's state.  Backward integrates with -eps: velocities
      //    keep their forward-time sign, nothing is negated
      const bool fwd = NM_UNIFORM(!(nm_uniform(nm_args(), chain, it, 1 + 2 * depth) < 0.5f));
      const float eps = fwd ? eps0 : -eps0;
      const int edge_at = fwd ? 3 * Ppad : 0, other_at = fwd ? 0 : 3 * Ppad;
      {
        const float* edge = nm_args().N.ws + chain * (int64_t)((12 + 2 * max_depth) * Ppad) + edge_at;
        NM_LANE(le, ce, he);
        for_each3(th, v, g, ce, he, le, [&](float& tv, float& vv, float& gv, int idx, bool) {
          tv = edge[idx];
          vv = edge[Ppad + idx];
          gv = edge[2 * Ppad + idx];
        });
      }
      // 2. the new subtree: 2^depth leaves, one leapfrog step each.  (rho' needs no zeroing: the first leaf stores 0 + v)
      float Wp = ninf, t_cand = 0.0f, H_cand = 0.0f;
      bool valid = true;
      const int n_leaf = 1 << depth;
#pragma unroll 1
      for (int k = 0; k < n_leaf; ++k) {
        NmKArgs& K = nm_args();
        const float wk = 0.5f * eps;
        {  // half a kick, a drift
          const float* sg = nm_scales(K.N, chain, NPAR);
          NM_LANE(le, ce, he);
          for_each3(th, v, g, ce, he, le, [&](float& tv, float& vv, float& gv, int idx, bool) {
            const float s = sg[idx];
            vv = vv + (wk * s) * gv;
            tv = tv + (eps * s) * vv;
          });
        }
        write_images<BF3, SH>(lw, th, c, h, lane, wl);
        const float t = eval_any<0, false, BF3, SH, true>(K.A, xs, lw, th, g, has_temp, temp, c, h, lane, true, pc, wl);
        float kin = 0.0f;
        {  // half a kick, the kinetic energy
          const float* sg = nm_scales(nm_args().N, chain, NPAR);
          NM_LANE(le, ce, he);
          for_each_pair(v, g, ce, he, le, [&](float& vv, float& gv, int idx, bool counts) {
            vv = vv + (wk * sg[idx]) * gv;
            if (counts) kin += vv * vv;
          });
        }
        kin = wsum(kin);
        const float H = -t + 0.5f * kin;
        float delta = H0 - H;
        if (!(delta == delta)) delta = ninf;
        if (NM_UNIFORM(-delta > 1000.0f)) {  // a divergent draw
          divergent = true;
          valid = false;
          break;
        }
        Wp = nm_logaddexp(Wp, delta);
        float* nv = nm_args().N.ws + chain * (int64_t)((12 + 2 * max_depth) * Ppad);
        // reservoir sampling of the subtree's candidate: the first leaf is always taken
        if (NM_UNIFORM(nm_uniform(nm_args(), chain, it, 1 + 2 * EY_NUTS_MAX_DEPTH + n) < expf(delta - Wp))) {
          NM_LANE(le, ce, he);
          for_each_pair(th, g, ce, he, le, [&](float& tv, float& gv, int idx, bool) {
            nv[8 * Ppad + idx] = tv;
            nv[9 * Ppad + idx] = gv;
          });
          t_cand = t;
          H_cand = H;
        }
        const float a1 = expf(delta);
        acc_sum += a1 < 1.0f ? a1 : 1.0f;
        n += 1;
        // rho' += v, and the aligned blocks of 2^j leaves that end at k, from the checkpoints
        float* rp = nv + 11 * Ppad;
        const bool first = k == 0;
        if ((k & 1) == 0) {
          float* cv = nv + (12 + 2 * __popc((unsigned)(k >> 1))) * Ppad;
          NM_LANE(le, ce, he);
          for_each(v, ce, he, le, [&](float& vv, int idx, bool) {
            const float r = (first ? 0.0f : rp[idx]) + vv;
            rp[idx] = r;
            cv[idx] = vv;
            cv[Ppad + idx] = r;
          });
        } else {
          {
            NM_LANE(le, ce, he);
            for_each(v, ce, he, le, [&](float& vv, int idx, bool) { rp[idx] = rp[idx] + vv; });
          }
          int slot = __popc((unsigned)(k >> 1));
#pragma unroll 1
          for (int kk = k; kk & 1; kk >>= 1, --slot) {
            const float* cv = nv + (12 + 2 * slot) * Ppad;
            float sa = 0.0f, sb = 0.0f;
            NM_LANE(le, ce, he);
            for_each(v, ce, he, le, [&](float& vv, int idx, bool counts) {
              const float cvi = cv[idx];
              const float r = rp[idx] - cv[Ppad + idx] + cvi;
              if (counts) {
                sa += cvi * r;
                sb += vv * r;
              }
            });
            sa = wsum(sa);
            sb = wsum(sb);
            if (!NM_UNIFORM(sa > 0.0f && sb > 0.0f)) {
              valid = false;
              break;
            }
          }
          if (!valid) break;
        }
      }
      // 3. an invalid subtree is discarded and the draw stops
      if (!valid) break;
      // 4. the edge moves, rho += rho', and the criterion between the tree's edges (the extended edge's v is in registers) ...
      float* nv = nm_args().N.ws + chain * (int64_t)((12 + 2 * max_depth) * Ppad);
      float sa = 0.0f, sb = 0.0f;
      {
        float* edge = nv + edge_at;
        const float* other = nv + other_at;
        NM_LANE(le, ce, he);
        for_each3(th, v, g, ce, he, le, [&](float& tv, float& vv, float& gv, int idx, bool counts) {
          edge[idx] = tv;
          edge[Ppad + idx] = vv;
          edge[2 * Ppad + idx] = gv;
          const float r = nv[10 * Ppad + idx] + nv[11 * Ppad + idx];
          nv[10 * Ppad + idx] = r;
          const float ov = other[Ppad + idx];
          if (counts) {
            sa += ov * r;
            sb += vv * r;
          }
        });
      }
      // ... biased progressive sampling of the tree's proposal (theta and g are dead here: they carry the copy)
      if (NM_UNIFORM(nm_uniform(nm_args(), chain, it, 2 + 2 * depth) < expf(Wp - W))) {
        NM_LANE(le, ce, he);
        for_each_pair(th, g, ce, he, le, [&](float& tv, float& gv, int idx, bool) {
          tv = nv[8 * Ppad + idx];
          gv = nv[9 * Ppad + idx];
          nv[6 * Ppad + idx] = tv;
          nv[7 * Ppad + idx] = gv;
        });
        t_prop = t_cand;
        H_prop = H_cand;
        moved = true;
      }
      W = nm_logaddexp(W, Wp);
      depth += 1;
      sa = wsum(sa);
      sb = wsum(sb);
      if (!NM_UNIFORM(sa > 0.0f && sb > 0.0f)) break;
    }
    // the state becomes the proposal.  (`moved` is a scalar: the stores below are behind scalar branches, and every lane
    // stores the same value where one would do -- no store behind a per-lane branch)
    NmKArgs& K = nm_args();
    KArgs& A = K.A;
    NmNArgs& N = K.N;
    const float rate = n > 0 ? acc_sum / (float)n : 0.0f;
    {
      const float* nv = N.ws + chain * (int64_t)((12 + 2 * max_depth) * Ppad);
      float* thg = A.theta + chain * NPAR;
      float* grg = A.grad + chain * NPAR;
      NM_LANE(le, ce, he);
      for_each_pair(th, g, ce, he, le, [&](float& tv, float& gv, int idx, bool) {
        tv = nv[6 * Ppad + idx];
        gv = nv[7 * Ppad + idx];
      });
      if (moved) {
        t_state = t_prop;
        for_each_pair(th, g, ce, he, le, [&](float& tv, float& gv, int idx, bool) {
          thg[idx] = tv;
          grg[idx] = gv;
        });
        A.target[chain] = t_prop;
        if (A.accept_count) A.accept_count[chain] += 1;
      }
      if (A.rec_samples) {  // the state this chain is left in: the proposal
        float* so = A.rec_samples + ((int64_t)it * A.C + chain) * NPAR;
        for_each(th, ce, he, le, [&](float& tv, int idx, bool) { so[idx] = tv; });
      }
    }
    const int64_t at = (int64_t)it * A.C + chain;
    A.accepted[chain] = moved ? 1 : 0;
    if (A.rate) A.rate[chain] = rate;
    if (A.rec_targets) A.rec_targets[at] = t_state;
    if (A.rec_accepted) A.rec_accepted[at] = moved ? 1 : 0;
    if (N.depth) N.depth[chain] = depth;
    if (N.n_leapfrog) N.n_leapfrog[chain] = n;
    if (N.divergent) N.divergent[chain] = divergent ? 1 : 0;
    if (N.energy) N.energy[chain] = H_prop;
    if (N.depth_rec) N.depth_rec[at] = depth;
    if (N.div_rec) N.div_rec[at] = divergent ? 1 : 0;
    if (N.w.steps_rec) static_cast<float*>(N.w.steps_rec)[at] = eps0;
    if (N.w.rate_rec) static_cast<float*>(N.w.rate_rec)[at] = rate;
    // The two warm-up epilogues, with the arithmetic of EY_WARM_EPILOGUES (ey_generic.hip): the dual-averaging step on the
    // draw's accept statistic, then the f64 Welford moments of the state the chain is left in (theta of this scope), in the
    // diagonal form.  Replicas read the same accumulator and store the same bits: the loads of an element are one
    // instruction, ahead of its store.
    if (N.w.da_state && it < N.w.da_n) {
      eps0 = (float)ey_da_update(da, N.w.da_table + 3 * it, (double)rate, N.w.d, N.w.has_eub != 0, N.w.logeub,
                                 it == N.w.final_it);
      N.step_vec[chain] = eps0;
    }
    if (N.w.mean) {
      double* mean_c = N.w.mean + chain * (int64_t)NPAR;
      double* M2_c = N.w.M2 + chain * (int64_t)NPAR;
      const double cnt = (double)(N.w.count + it + 1);
      const double f = (cnt - 1.0) / cnt;
      NM_LANE(le, ce, he);
      for_each(th, ce, he, le, [&](float& tv, int idx, bool) {
        const double x = (double)tv;
        const double mu = mean_c[idx];
        const double dx = x - mu;
        mean_c[idx] = mu + dx / cnt;
        M2_c[idx] = M2_c[idx] + f * (dx * dx);
      });
    }
    if (n_iters > 1) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  }
  NmNArgs& N = nm_args().N;
  if (N.w.da_state) {
    N.w.da_state[3 * chain] = da[0];
    N.w.da_state[3 * chain + 1] = da[1];
  }
}

// k_mfma32's frame, as k_eslice_mfma takes it: the data image staged behind the only workgroup barrier, this wave's region, a
// Pace that is off (the number of leaves of a draw is not known in advance, so there is nothing to pace by: pace_post /
// pace_apply return at once, and no wave ever waits for its SIMD partner).
template <int WAVES, int BF3, typename SH>
__global__ void __launch_bounds__(WAVES * 64, 2) k_nuts_mfma(NmKernArgs K) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  const int xfloats = K.A.ntiles * XTILE_FLOATS;
  for (int i = tid; i < xfloats; i += WAVES * 64) smem[i] = K.A.xpack[i];
  const float* xs = smem;
  float* lw = smem + xfloats + wave * WAVE_FLOATS;
  __syncthreads();
  Pace pc;
  pc.prog = nullptr; pc.junk = nullptr; pc.wave = wave; pc.partner = wave; pc.left = 0; pc.bias = 0;
  pc.on = false; pc.hi = false;
  const int64_t first = (int64_t)blockIdx.x + (int64_t)gridDim.x * wave, stride = (int64_t)gridDim.x * WAVES;
  const int64_t C = K.A.C;
  for (int64_t chain = first; chain < C; chain += stride)  // whole waves; no workgroup synchronisation below
    nm_chain<BF3, SH>(xs, lw, chain, c, h, lane, pc);
}

// ----------------------------------------------------------------------------------------------- host side
template <int BF3, typename SH>
static int nm_launch_v(NmKernArgs& k, int n_cu, hipStream_t s) {
  const size_t bytes = mf_lds_bytes(k.A.ntiles, 8, 0, BF3);
  const void* fn = reinterpret_cast<const void*>(k_nuts_mfma<8, BF3, SH>);
  // per launch, as mf_launch_v: function attributes are per device
  EY_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)mf_lds_bytes(BF3 == 2 ? MF_TRD_TILES : (BF3 ? MF_BF3_TILES : MF_MAX_TILES), 8, 0, BF3)));
  const unsigned grid = (unsigned)std::min<int64_t>(k.A.C, n_cu > 0 ? n_cu : 256);
  hipLaunchKernelGGL((k_nuts_mfma<8, BF3, SH>), dim3(grid), dim3(512), bytes, s, k);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

#define NM_COMMA ,
// mf_launch's choice of form and shape for an evaluation with its gradient: the headline model in both product forms, the
// other 4-32-32 models in bf16x3; the piece images (BF3 = 2) where the data image leaves room for them
#define NM_SHAPE_LAUNCH(SHAPE)                                                          \
  do {                                                                                  \
    if (trd) return nm_launch_v<2, SHAPE>(k, pl->n_cu, s);                              \
    return nm_launch_v<1, SHAPE>(k, pl->n_cu, s);                                       \
  } while (0)

// The caller (nuts_impl, ey_api.hip) has checked that the plan is served by the mfma32 family with the batch it holds, the
// diagonal form, the attached workspace and its size for this (C, max_depth).
int ey_nuts_mfma_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                        const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                        const EyWarm& w) {
  if (!pl->nuts_tree || pl->nuts_tree_bytes < ey_nuts_ws_bytes(pl, d.C, nu.max_depth))  // (never: see above)
    EY_FAIL(EY_ERR_INVALID, "NUTS with the tree in device memory: no workspace of this call's size is attached");
  const EyModel& m = pl->m;
  hipStream_t s = d.s;
  NmKernArgs k = {};
  MfArgs& a = k.A;
  NmArgs& n = k.N;
  a.theta = (float*)theta; a.target = (float*)target; a.grad = (float*)grad;
  a.step = (float)step;
  a.C = d.C; a.temp = (const float*)d.temp; a.seed = d.seed; a.iter = d.iter; a.chain_offset = d.chain_offset;
  a.recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) ? 1 : 0;
  a.accepted = (unsigned char*)d.accepted;
  a.rate = (float*)d.log_rate;
  a.n_iters = 1;
  if (const EyRun* run = d.run) {
    a.n_iters = run->n_iters;
    a.rec_samples = (float*)run->samples;
    a.rec_targets = (float*)run->targets;
    a.rec_accepted = (unsigned char*)run->accepted;
    a.accept_count = run->accept_count;
  }
  a.xpack = (const float*)pl->d_xpack;
  a.mu = (const float*)m.mu;
  a.inv_var = (const float*)m.inv_var;
  a.prior_uniform = pl->prior_uniform ? 1 : 0;
  a.mu0 = (float)pl->prior_mu0;
  a.iv0 = (float)pl->prior_iv0;
  a.prior_const = (float)m.prior_const;
  a.ntiles = (m.N + 31) / 32;
  a.short_last = (m.N - 32 * (a.ntiles - 1)) <= 24 ? 1 : 0;
  a.balance = 0;
  a.stagger = 0;
  n.metric = (const float*)metric; n.G = G; n.metric_index = (const int*)metric_index;
  n.v0 = (const float*)nu.v0; n.u = (const float*)nu.u; n.S = nu.S;
  n.step_vec = (float*)step_vec;
  n.max_depth = nu.max_depth;
  n.ws = (float*)pl->nuts_tree;
  n.depth = nu.depth; n.n_leapfrog = nu.n_leapfrog; n.divergent = nu.divergent; n.energy = (float*)nu.energy;
  n.depth_rec = nu.depth_rec; n.div_rec = nu.div_rec;
  n.w = w;
  const bool bf3 = pl->products == EY_PRODUCTS_BF16X3 && a.ntiles <= MF_BF3_TILES && !(t_ey_variant & 1);
  const bool trd = bf3 && a.ntiles <= MF_TRD_TILES && !(t_ey_variant & 4);
  if (pl->mfma32_kind == 2) {
    if (!bf3) EY_FAIL(EY_ERR_UNSUPPORTED, "mfma32: this model is served in the bf16x3 form only");
    const int act = m.act[0];
    if (m.lik == EY_LIK_CE_SUM) {
      if (act == EY_ACT_TANH) NM_SHAPE_LAUNCH(MfShape<3 NM_COMMA EY_ACT_TANH NM_COMMA EY_LIK_CE_SUM>);
      NM_SHAPE_LAUNCH(MfShape<3 NM_COMMA EY_ACT_RELU NM_COMMA EY_LIK_CE_SUM>);
    }
    if (act == EY_ACT_SIGMOID) NM_SHAPE_LAUNCH(MfShape<1 NM_COMMA EY_ACT_SIGMOID NM_COMMA EY_LIK_BCE_SUM>);
    if (act == EY_ACT_TANH) NM_SHAPE_LAUNCH(MfShape<1 NM_COMMA EY_ACT_TANH NM_COMMA EY_LIK_BCE_SUM>);
    NM_SHAPE_LAUNCH(MfShape<1 NM_COMMA EY_ACT_RELU NM_COMMA EY_LIK_BCE_SUM>);
  }
  if (bf3) NM_SHAPE_LAUNCH(MfHeadline);
  return nm_launch_v<0, MfHeadline>(k, pl->n_cu, s);
}
