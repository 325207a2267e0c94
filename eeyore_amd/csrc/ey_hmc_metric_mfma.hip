// k_hmc_metric_mfma: HMC under a DIAGONAL metric and its warm-up (include/eeyore_amd_hmc_metric_fused.h) on
// the matrix cores for the MLP(4-32-32-dK) plans that ey_mfma32.hip serves.  The draw of k_hmc_metric<T, TINY, EY_METRIC_DIAG>
// and the epilogues of k_hmc_metric_warmup (ey_generic.hip), in the frame of k_nuts_mfma: one wave per
// chain, eight chains per persistent workgroup, chain-major; the data image shared in LDS, a region of LDS per wave; theta, v
// and g in the lane's Vec register layout; every evaluation by the fused evaluation with its gradient.  ey_mfma32.hip is
// included for all of that (EY_MF_PART 2 there: every entry point and kernel instantiation of its own left out).
//
// The velocity is whitened: v ~ N(0, I), v += (w s) g, theta += (eps s) v, with the scales s read from the chain's row of the
// [G, P] table at for_each's canonical index where a kick or a drift needs them.  Replicas (the two halves of the wave for W0,
// W2, b0, b1; every lane for b2) store the same bits to the same address, as the state write-back of k_mfma32 does.  No
// memory operation sits behind a per-lane branch: every decision is read as a scalar before it is branched
// on.  There is no workgroup barrier below the chain loop.
#define EY_MF_PART 2
#include "ey_mfma32.hip"

#include "ey_hmc_metric_mfma.h"

// a wave-uniform decision as a scalar
#define HM_UNIFORM(cond) (__builtin_amdgcn_readfirstlane((cond) ? 1 : 0) != 0)
// Lane coordinates the compiler cannot identify with those of kernel entry (run_chain's remedy): the element offsets of the
// passes over global memory depend on the lane alone, and left to the compiler all of them are computed once, kept across
// every evaluation and spilled.  Made opaque where a pass begins they are recomputed there and die with it.
#define HM_LANE(le, ce, he)    \
  int le = lane;               \
  asm volatile("" : "+v"(le)); \
  const int ce = le & 31, he = le >> 5

// What the kernel takes beside MfArgs (which carries the state, the step, num_steps, the temperatures, the Philox key, v0 as
// `p0`, u, the outputs of a step and the records of a run).
struct HmArgs {
  const float* metric;      // [G, P] scales
  int64_t G;
  const int* metric_index;  // [C] or null
  float* step_vec;          // [C] or null; in/out under a dual averaging
  EyWarm w;
};
struct HmKernArgs {
  MfArgs A;
  HmArgs H;
};
typedef const __attribute__((address_space(4))) HmKernArgs HmKArgs;
typedef const __attribute__((address_space(4))) HmArgs HmHArgs;

// The arguments re-read from the kernarg segment (k_mfma32's remedy): taken once per draw they all stay live in scalar
// registers across the trajectory, and the allocator spills scalars into vector registers.
__device__ __forceinline__ HmKArgs& hm_args() {
  HmKArgs* Kp = (HmKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(Kp));
  return *Kp;
}
// the chain's row of the metric table (EY_CHAIN_INDEX): nm_scales of ey_nuts_mfma.hip
__device__ __forceinline__ const float* hm_scales(HmHArgs& H, int64_t chain, int npar) {
  int64_t g = H.G == 1 ? 0 : (H.metric_index ? (int64_t)H.metric_index[chain] : chain);
  g = g < 0 ? 0 : (g > H.G - 1 ? H.G - 1 : g);
  return H.metric + g * npar;
}

// All draws of one chain of one launch.
template <int BF3, typename SH>
__device__ __forceinline__ void hm_chain(const float* xs, float* lw, const int64_t chain, const int c, const int h,
                                         const int lane, Pace& pc) {
  constexpr int DKV = SH::DK;
  typedef Vec<DKV> Vec;
  float t_state, eps;
  double da[3] = {0.0, 0.0, 0.0};
  int n_iters;
  {
    HmKArgs& K = hm_args();
    t_state = K.A.target[chain];
    eps = K.H.step_vec ? K.H.step_vec[chain] : K.A.step;
    if (K.H.w.da_state) {
      for (int k = 0; k < 3; ++k) da[k] = K.H.w.da_state[3 * chain + k];
    }
    n_iters = K.A.n_iters;
  }
#pragma unroll 1
  for (int it = 0; it < n_iters; ++it) {
    // (run_chain's fences: later iterations read what this wave's lanes wrote at the end of the one before)
    if (it > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    Vec th, v, g;
    W1Lo wl;
    float h_cur;
    bool has_temp;
    float temp;
    int L;
    {
      HmKArgs& K = hm_args();
      KArgs& A = K.A;
      has_temp = A.temp != nullptr;
      temp = has_temp ? A.temp[chain] : 1.0f;
      L = A.L;
      // v ~ N(0, I): the table, or the chain's stream as k_mfma32 stages it
      const EyRng rn = ey_rng_make(A.seed, A.chain_offset + (uint64_t)chain, A.iter + (uint64_t)it, EY_STREAM_NORMAL);
      const float* vin = A.p0 ? A.p0 + chain * NPAR : nullptr;
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
      h_cur = -t_state + 0.5f * kin;
      if (A.recompute) {
        write_images<BF3, SH>(lw, th, c, h, lane, wl);
        (void)eval_any<0, false, BF3, SH, true>(A, xs, lw, th, g, has_temp, temp, c, h, lane, false, pc, wl);
      }
    }
    {  // half a kick
      const float wk = 0.5f * eps;
      const float* sg = hm_scales(hm_args().H, chain, NPAR);
      HM_LANE(le, ce, he);
      for_each_pair(v, g, ce, he, le, [&](float& vv, float& gv, int idx, bool) { vv = vv + (wk * sg[idx]) * gv; });
    }
    float t = t_state, kin = 0.0f;
#pragma unroll 1
    for (int k = 1; k <= L; ++k) {
      HmKArgs& K = hm_args();
      {  // a drift
        const float* sg = hm_scales(K.H, chain, NPAR);
        HM_LANE(le, ce, he);
        for_each_pair(th, v, ce, he, le, [&](float& tv, float& vv, int idx, bool) { tv = tv + (eps * sg[idx]) * vv; });
      }
      write_images<BF3, SH>(lw, th, c, h, lane, wl);
      t = eval_any<0, false, BF3, SH, true>(K.A, xs, lw, th, g, has_temp, temp, c, h, lane, k == L, pc, wl);
      {  // a kick, halved on the last step; the kinetic energy (read after the last step only)
        const float w = (k < L) ? eps : 0.5f * eps;
        const float* sg = hm_scales(hm_args().H, chain, NPAR);
        kin = 0.0f;
        HM_LANE(le, ce, he);
        for_each_pair(v, g, ce, he, le, [&](float& vv, float& gv, int idx, bool counts) {
          vv = vv + (w * sg[idx]) * gv;
          if (counts) kin += vv * vv;
        });
      }
    }
    kin = wsum(kin);
    const float h_prop = -t + 0.5f * kin;
    float rate = expf(h_cur - h_prop);
    if (rate > 1.0f) rate = 1.0f;
    HmKArgs& K = hm_args();
    KArgs& A = K.A;
    HmHArgs& H = K.H;
    const EyRng ru = ey_rng_make(A.seed, A.chain_offset + (uint64_t)chain, A.iter + (uint64_t)it, EY_STREAM_UNIFORM);
    const float u = A.u ? A.u[chain] : ey_rng_uniform<float>(ru);
    // strict <, a NaN rate rejects (k_hmc_metric); the same in every lane, and read as a scalar so that the stores behind it
    // are behind a scalar branch
    const bool acc = HM_UNIFORM(u < rate);
    {
      float* thg = A.theta + chain * NPAR;
      float* grg = A.grad + chain * NPAR;
      HM_LANE(le, ce, he);
      if (acc) {  // a rejected chain's theta, target and gradient are not written: they keep their bits
        t_state = t;
        for_each_pair(th, g, ce, he, le, [&](float& tv, float& gv, int idx, bool) {
          thg[idx] = tv;
          grg[idx] = gv;
        });
        A.target[chain] = t;
        if (A.accept_count) A.accept_count[chain] += 1;
      } else if (A.rec_samples || H.w.mean) {  // the state this chain is left in, for the record and the moments
        for_each(th, ce, he, le, [&](float& tv, int idx, bool) { tv = thg[idx]; });
      }
      if (A.rec_samples) {
        float* so = A.rec_samples + ((int64_t)it * A.C + chain) * NPAR;
        for_each(th, ce, he, le, [&](float& tv, int idx, bool) { so[idx] = tv; });
      }
    }
    // (every lane stores the same value: no store behind a per-lane branch)
    const int64_t at = (int64_t)it * A.C + chain;
    A.accepted[chain] = acc ? 1 : 0;
    if (A.rate) A.rate[chain] = rate;
    if (A.hcur) A.hcur[chain] = h_cur;
    if (A.hprop) A.hprop[chain] = h_prop;
    if (A.rec_targets) A.rec_targets[at] = t_state;
    if (A.rec_accepted) A.rec_accepted[at] = acc ? 1 : 0;
    if (H.w.steps_rec) static_cast<float*>(H.w.steps_rec)[at] = eps;
    if (H.w.rate_rec) static_cast<float*>(H.w.rate_rec)[at] = rate;
    // The two warm-up epilogues, with the arithmetic of EY_WARM_EPILOGUES (ey_generic.hip) as k_nuts_mfma restates it: the
    // dual-averaging step on the draw's rate, then the f64 Welford moments of the state the chain is left in (theta of this
    // scope), in the diagonal form.  Replicas read the same accumulator and store the same bits: the loads of an element
    // are one instruction, ahead of its store.
    if (H.w.da_state && it < H.w.da_n) {
      eps = (float)ey_da_update(da, H.w.da_table + 3 * it, (double)rate, H.w.d, H.w.has_eub != 0, H.w.logeub,
                                it == H.w.final_it);
      H.step_vec[chain] = eps;
    }
    if (H.w.mean) {
      double* mean_c = H.w.mean + chain * (int64_t)NPAR;
      double* M2_c = H.w.M2 + chain * (int64_t)NPAR;
      const double cnt = (double)(H.w.count + it + 1);
      const double f = (cnt - 1.0) / cnt;
      HM_LANE(le, ce, he);
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
  HmHArgs& H = hm_args().H;
  if (H.w.da_state) {
    H.w.da_state[3 * chain] = da[0];
    H.w.da_state[3 * chain + 1] = da[1];
  }
}

// k_mfma32's frame, as k_nuts_mfma takes it: the data image staged behind the only workgroup barrier, this wave's region, a
// Pace that is off (pace_post / pace_apply return at once, and no wave ever waits for its SIMD partner).
template <int WAVES, int BF3, typename SH>
__global__ void __launch_bounds__(WAVES * 64, 2) k_hmc_metric_mfma(HmKernArgs K) {
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
    hm_chain<BF3, SH>(xs, lw, chain, c, h, lane, pc);
}

// ----------------------------------------------------------------------------------------------- host side
template <int BF3, typename SH>
static int hm_launch_v(HmKernArgs& k, int n_cu, hipStream_t s) {
  const size_t bytes = mf_lds_bytes(k.A.ntiles, 8, 0, BF3);
  const void* fn = reinterpret_cast<const void*>(k_hmc_metric_mfma<8, BF3, SH>);
  // per launch, as mf_launch_v: function attributes are per device
  EY_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)mf_lds_bytes(BF3 == 2 ? MF_TRD_TILES : (BF3 ? MF_BF3_TILES : MF_MAX_TILES), 8, 0, BF3)));
  const unsigned grid = (unsigned)std::min<int64_t>(k.A.C, n_cu > 0 ? n_cu : 256);
  hipLaunchKernelGGL((k_hmc_metric_mfma<8, BF3, SH>), dim3(grid), dim3(512), bytes, s, k);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

#define HM_COMMA ,
// mf_launch's choice of form and shape for an evaluation with its gradient: the headline model in both product forms, the
// other 4-32-32 models in bf16x3; the piece images (BF3 = 2) where the data image leaves room for them
#define HM_SHAPE_LAUNCH(SHAPE)                              \
  do {                                                      \
    if (trd) return hm_launch_v<2, SHAPE>(k, pl->n_cu, s);  \
    return hm_launch_v<1, SHAPE>(k, pl->n_cu, s);           \
  } while (0)

// The caller (hmc_metric_impl / ey_hmc_metric_warmup, ey_api.hip) has checked that the plan is served by the mfma32 family
// with the batch it holds, and the diagonal form.
int ey_hmc_metric_mfma_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                              const void* metric_index, const void* v0, const void* u, double step, void* step_vec, int L,
                              const EyDraw& d, void* rate, void* hcur, void* hprop, const EyWarm& w) {
  const EyModel& m = pl->m;
  hipStream_t s = d.s;
  HmKernArgs k = {};
  MfArgs& a = k.A;
  HmArgs& hm = k.H;
  a.theta = (float*)theta; a.target = (float*)target; a.grad = (float*)grad;
  a.p0 = (const float*)v0; a.u = (const float*)u;
  a.step = (float)step;
  a.L = L;
  a.C = d.C; a.temp = (const float*)d.temp; a.seed = d.seed; a.iter = d.iter; a.chain_offset = d.chain_offset;
  a.recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) ? 1 : 0;
  a.accepted = (unsigned char*)d.accepted;
  a.rate = (float*)rate; a.hcur = (float*)hcur; a.hprop = (float*)hprop;
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
  hm.metric = (const float*)metric; hm.G = G; hm.metric_index = (const int*)metric_index;
  hm.step_vec = (float*)step_vec;
  hm.w = w;
  const bool bf3 = pl->products == EY_PRODUCTS_BF16X3 && a.ntiles <= MF_BF3_TILES && !(t_ey_variant & 1);
  const bool trd = bf3 && a.ntiles <= MF_TRD_TILES && !(t_ey_variant & 4);
  if (pl->mfma32_kind == 2) {
    if (!bf3) EY_FAIL(EY_ERR_UNSUPPORTED, "mfma32: this model is served in the bf16x3 form only");
    const int act = m.act[0];
    if (m.lik == EY_LIK_CE_SUM) {
      if (act == EY_ACT_TANH) HM_SHAPE_LAUNCH(MfShape<3 HM_COMMA EY_ACT_TANH HM_COMMA EY_LIK_CE_SUM>);
      HM_SHAPE_LAUNCH(MfShape<3 HM_COMMA EY_ACT_RELU HM_COMMA EY_LIK_CE_SUM>);
    }
    if (act == EY_ACT_SIGMOID) HM_SHAPE_LAUNCH(MfShape<1 HM_COMMA EY_ACT_SIGMOID HM_COMMA EY_LIK_BCE_SUM>);
    if (act == EY_ACT_TANH) HM_SHAPE_LAUNCH(MfShape<1 HM_COMMA EY_ACT_TANH HM_COMMA EY_LIK_BCE_SUM>);
    HM_SHAPE_LAUNCH(MfShape<1 HM_COMMA EY_ACT_RELU HM_COMMA EY_LIK_BCE_SUM>);
  }
  if (bf3) HM_SHAPE_LAUNCH(MfHeadline);
  return hm_launch_v<0, MfHeadline>(k, pl->n_cu, s);
}
