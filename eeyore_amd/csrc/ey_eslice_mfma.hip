// k_eslice_mfma: elliptical slice sampling (include/eeyore_amd_eslice.h) on the matrix cores for the
// MLP(4-32-32-dK) plans that ey_mfma32.hip serves.  k_eslice's transition, decision for decision, in the
// frame of k_mfma32: one wave per chain, eight chains per persistent workgroup, chain-major; the data image shared in LDS,
// a region of LDS per wave; the state in the lane's Vec register layout; every point of the ellipse evaluated by the
// value-only form of the fused evaluation, eval<..., GRAD = false>.  ey_mfma32.hip is included for all of that (EY_MF_PART 2
// there: every entry point and kernel instantiation of its own left out).
#define EY_MF_PART 2
#include "ey_mfma32.hip"

#include "ey_eslice.h"

// a wave-uniform decision as a scalar (k_eslice's)
#define ES_UNIFORM(cond) (__builtin_amdgcn_readfirstlane((cond) ? 1 : 0) != 0)
// Lane coordinates the compiler cannot identify with those of kernel entry (run_chain's remedy): the element offsets of the
// passes over global tables depend on the lane alone, and left to the compiler all of them are computed once, kept across
// every evaluation and spilled.  Made opaque where a pass begins they are recomputed there and die with it.
#define ES_LANE(le, ce, he) \
  int le = lane;            \
  asm volatile("" : "+v"(le)); \
  const int ce = le & 31, he = le >> 5

// What the kernels take beside MfArgs.  The prior here is the plan's REAL one: without a base the evaluation is launched with
// neutral prior arguments (MfArgs: prior_uniform = 1, iv0 = 0, prior_const = 0), so that eval returns the tempered
// log-likelihood alone -- lik + (0 - 0.5 * 0) * t, exactly -- and the kernel adds the tempered Normal prior itself from
// these; nothing is subtracted in f32.  With a base MfArgs holds the real prior too and eval returns the log-target.
struct EsArgs {
  float* ell;               // [C] in/out (k_eslice_mfma_ell: out, or null)
  const float* base_loc;    // [P] or null (with base_scale)
  const float* base_scale;  // [P] or null
  const float* mu;          // [P]
  const float* inv_var;     // [P]
  int prior_uniform;        // every parameter shares (mu0, iv0)
  float mu0, iv0, prior_const;
  const float* z;           // [C,P] or null
  const float* u;           // [C,S] or null
  int64_t S;
  int max_shrinks;
  int* n_evals;             // [C] or null
  int* n_evals_rec;         // [n_iters,C] or null
};
struct EsKernArgs {
  MfArgs A;
  EsArgs E;
};
typedef const __attribute__((address_space(4))) EsKernArgs EsKArgs;
typedef const __attribute__((address_space(4))) EsArgs EsEArgs;

// The base's location of parameter idx: base_loc, or the prior's mu (one value when the prior is uniform).  Read from global
// memory where it is needed, once per point: held in registers beside x, nu and the point it sends every instantiation of
// the sampling kernel to scratch.
struct EsLoc {
  const float* gm;
  float mu0;
  bool uni;
  __device__ __forceinline__ float operator()(int idx) const { return uni ? mu0 : gm[idx]; }
};
__device__ __forceinline__ EsLoc es_loc(EsEArgs& E) {
  const bool based = E.base_loc != nullptr;
  return EsLoc{based ? E.base_loc : E.mu, E.mu0, !based && E.prior_uniform != 0};
}

// ell and the (tempered) log-target at the point p, whose images this call stages.  Without a base ell is the (tempered)
// log-likelihood, and the target adds the prior, summed here over x = p - mu with each parameter counted once; with one,
// ell is the log-target minus the base's exponent, sum_i -d_i^2 / 2 with d_i = (p_i - m_i) / s_i (eslice_ell_at's).
// Both results are wave-uniform.
// `park` (PARKED: the sampling kernel's nu): a vector that waits in this wave's LDS region while the tile loop runs, as the
// PARK elements of eval do and for the same reason -- x, nu and the point beside the tile loop's own registers are more
// than 256, and what does not fit goes to scratch.  It lies in the two transpose buffers, which a value-only evaluation
// never writes (at most 28 x 64 floats of their 2304), and is stored once the f32 image of W1, which write_images keeps
// there in the bf16x3 form, is dead.
template <int BF3, typename SH, bool PARKED>
__device__ __forceinline__ float es_ell_at(KArgs& A, EsEArgs& E, const float* xs, float* lw, Vec<SH::DK>& p,
                                           const EsLoc& loc, bool has_temp, float temp, int c, int h, int lane, Pace& pc,
                                           float* target_out, Vec<SH::DK>& park) {
  constexpr int DKV = SH::DK;
  W1Lo wl;
  Vec<DKV> g;  // (a value-only evaluation leaves it alone)
  write_images<BF3, SH>(lw, p, c, h, lane, wl);
  if constexpr (PARKED) {
    float* pk = lw + O_STAGE + lane;
    int k = 0;
    for_each2(park, park, [&](float& v, float&) { pk[64 * k] = v; ++k; });
  }
  const float v = eval_any<0, false, BF3, SH, false>(A, xs, lw, p, g, has_temp, temp, c, h, lane, true, pc, wl);
  if constexpr (PARKED) {
    int at = O_STAGE + lane;
    asm volatile("" : "+v"(at));  // an offset the compiler cannot match with the stores above: no forwarding
    int k = 0;
    for_each2(park, park, [&](float& v, float&) { v = lw[at + 64 * k]; ++k; });
    wave_lds_fence();
  }
  float q = 0.0f;
  ES_LANE(le, ce, he);
  if (E.base_loc) {  // (a kernel argument: the branch is scalar)
    const float* bs = E.base_scale;
    for_each(p, ce, he, le, [&](float& pv, int idx, bool counts) {
      const float d = (pv - loc(idx)) / bs[idx];
      if (counts) q += d * d;
    });
    *target_out = v;
    return v + 0.5f * wsum(q);
  }
  if (E.prior_uniform) {
    const float iv0 = E.iv0;
    const float mu0 = E.mu0;
    for_each(p, ce, he, le, [&](float& pv, int, bool counts) {
      const float d = pv - mu0;
      if (counts) q += d * d * iv0;
    });
  } else {
    const float* iv = E.inv_var;
    const float* mu = E.mu;
    for_each(p, ce, he, le, [&](float& pv, int idx, bool counts) {
      const float d = pv - mu[idx];
      if (counts) q += d * d * iv[idx];
    });
  }
  float prior = E.prior_const - 0.5f * wsum(q);
  if (has_temp) prior *= temp;
  *target_out = v + prior;
  return v;
}

// The arguments re-read from the kernarg segment (k_mfma32's remedy, once per evaluation here): taken once per draw they
// all stay live in scalar registers across the shrink loop, with the ten round keys of the uniform stream beside them, and
// the allocator spills scalars to scratch.
__device__ __forceinline__ EsKArgs& es_args() {
  EsKArgs* Kp = (EsKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(Kp));
  return *Kp;
}
// the uniform at block word `word` of the draw: the caller's table, or the chain's stream
__device__ __forceinline__ float es_uniform(EsKArgs& K, int64_t chain, int it, int word) {
  if (K.E.u) return K.E.u[chain * K.E.S + word];
  const EyRng ru = ey_rng_make(K.A.seed, K.A.chain_offset + (uint64_t)chain, K.A.iter + (uint64_t)it, EY_STREAM_UNIFORM);
  return ey_rng_uniform_at<float>(ru, (uint32_t)word);
}

// One draw of one chain.  e_state and t_state are the carried ell and target (wave-uniform).
template <int BF3, typename SH>
__device__ __forceinline__ void es_draw(EsKArgs& K, const float* xs, float* lw, const int64_t chain, const int it,
                                        const int c, const int h, const int lane, Pace& pc, float& e_state,
                                        float& t_state) {
  constexpr int DKV = SH::DK;
  typedef Vec<DKV> Vec;
  KArgs& A = K.A;
  EsEArgs& E = K.E;
  // (run_chain's fences: later iterations read what this wave's lanes wrote at the end of the one before)
  if (it > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const uint64_t iter = A.iter + (uint64_t)it;
  float* thg = A.theta + chain * NPAR;
  const bool has_temp = A.temp != nullptr;
  const float temp = has_temp ? A.temp[chain] : 1.0f;
  const bool based = E.base_loc != nullptr;

  Vec p, x, nu;
  const EsLoc loc = es_loc(E);
  // 1. nu = s z, x = theta - m.  Without a base s is the prior's sigma / sqrt(t): 1 / sqrt(t / sigma^2)
  {
    const EyRng rn = ey_rng_make(A.seed, A.chain_offset + (uint64_t)chain, iter, EY_STREAM_NORMAL);
    const float* zin = E.z ? E.z + chain * NPAR : nullptr;
    const float* zst = zin ? nullptr : stage_normals<BF3, DKV>(lw, rn, lane);
    const float* bs = E.base_scale;
    const float* ivt = E.inv_var;
    const bool uni = E.prior_uniform != 0;
    const float iv0 = E.iv0;
    for_each_pair(x, nu, c, h, lane, [&](float& xv, float& nv, int idx, bool) {
      const float zi = zin ? zin[idx] : zst[idx];
      float si;
      if (based) {
        si = bs[idx];
      } else {
        const float ivi = uni ? iv0 : ivt[idx];
        si = 1.0f / sqrtf(has_temp ? ivi * temp : ivi);
      }
      xv = thg[idx] - loc(idx);
      nv = si * zi;
    });
    wave_lds_fence();  // the staged normals have been read; the evaluations reuse that LDS
  }
  int n = 0;
  bool moved = false;
  float t_new = t_state, e_new = e_state;
  // 5. a chain whose carried ell is not finite stays put without evaluating
  if (ES_UNIFORM(e_state - e_state == 0.0f)) {
    // 2. the slice height; 3. the first angle and its bracket
    const float logy = e_state + logf(es_uniform(es_args(), chain, it, 0));
    float a = es_uniform(es_args(), chain, it, 1);
    float lo = a - 1.0f, hi = a;
#pragma unroll 1
    for (int k = 0;; ++k) {
      EsKArgs& Kq = es_args();
      const float ca = cospif(2.0f * a), sa = sinpif(2.0f * a);
      const EsLoc locq = es_loc(Kq.E);
      {
        ES_LANE(le, ce, he);
        for_each3(p, x, nu, ce, he, le, [&](float& pv, float& xv, float& nv, int idx, bool) { pv = locq(idx) + xv * ca + nv * sa; });
      }
      float t;
      const float e = es_ell_at<BF3, SH, true>(Kq.A, Kq.E, xs, lw, p, locq, has_temp, temp, c, h, lane, pc, &t, nu);
      n += 1;
      if (ES_UNIFORM(e > logy)) {  // (a NaN compares false)
        moved = true;
        t_new = t;
        e_new = e;
        break;
      }
      if (k == es_args().E.max_shrinks) break;  // the bracket is exhausted: the chain stays
      if (a < 0.0f) lo = a; else hi = a;
      a = lo + (hi - lo) * es_uniform(es_args(), chain, it, 2 + k);
    }
  }
  // (`moved` is a scalar: the stores below are behind scalar branches, and every lane stores the same value where one
  // would do -- no store behind a per-lane branch)
  EsKArgs& Kw = es_args();
  KArgs& Aw = Kw.A;
  EsEArgs& Ew = Kw.E;
  thg = Aw.theta + chain * NPAR;
  ES_LANE(le, ce, he);
  if (moved) {
    t_state = t_new;
    e_state = e_new;
    for_each(p, ce, he, le, [&](float& v, int idx, bool) { thg[idx] = v; });
    Aw.target[chain] = t_state;
    Ew.ell[chain] = e_state;
    if (Aw.accept_count) Aw.accept_count[chain] += 1;
  }
  if (Aw.rec_samples) {  // the state this chain is left in
    float* so = Aw.rec_samples + ((int64_t)it * Aw.C + chain) * NPAR;
    if (!moved) for_each(p, ce, he, le, [&](float& v, int idx, bool) { v = thg[idx]; });
    for_each(p, ce, he, le, [&](float& v, int idx, bool) { so[idx] = v; });
  }
  Aw.accepted[chain] = moved ? 1 : 0;
  if (Aw.rec_targets) Aw.rec_targets[(int64_t)it * Aw.C + chain] = t_state;
  if (Aw.rec_accepted) Aw.rec_accepted[(int64_t)it * Aw.C + chain] = moved ? 1 : 0;
  if (Ew.n_evals) Ew.n_evals[chain] = n;
  if (Ew.n_evals_rec) Ew.n_evals_rec[(int64_t)it * Aw.C + chain] = n;
  if (Aw.n_iters > 1) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}

// what the two kernels share of k_mfma32's frame: the data image, this wave's region, a Pace that is off (a draw's number of
// evaluations is not known in advance, so there is nothing to pace by: pace_post / pace_apply return at once)
#define ES_FRAME()                                                                                       \
  extern __shared__ __attribute__((aligned(16))) float smem[];                                           \
  const int tid = threadIdx.x;                                                                           \
  const int lane = tid & 63;                                                                             \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                             \
  const int c = lane & 31, h = lane >> 5;                                                                \
  const int xfloats = K.A.ntiles * XTILE_FLOATS;                                                         \
  for (int i = tid; i < xfloats; i += WAVES * 64) smem[i] = K.A.xpack[i];                                \
  const float* xs = smem;                                                                                \
  float* lw = smem + xfloats + wave * WAVE_FLOATS;                                                       \
  __syncthreads();                                                                                       \
  Pace pc;                                                                                               \
  pc.prog = nullptr; pc.junk = nullptr; pc.wave = wave; pc.partner = wave; pc.left = 0; pc.bias = 0;     \
  pc.on = false; pc.hi = false;                                                                          \
  const int64_t first = (int64_t)blockIdx.x + (int64_t)gridDim.x * wave, stride = (int64_t)gridDim.x * WAVES

// Chains of one workgroup make different numbers of evaluations: there is no workgroup synchronisation below the chain loop
// (as in k_mfma32), so none waits for another.
template <int WAVES, int BF3, typename SH>
__global__ void __launch_bounds__(WAVES * 64, 2) k_eslice_mfma(EsKernArgs K) {
  ES_FRAME();
  for (int64_t chain = first; chain < K.A.C; chain += stride) {  // whole waves; no workgroup synchronisation below
    float t_state = K.A.target[chain], e_state = K.E.ell[chain];
    const int n_iters = K.A.n_iters;
    for (int it = 0; it < n_iters; ++it) {
      EsKArgs* Kp = (EsKArgs*)__builtin_amdgcn_kernarg_segment_ptr();  // (see k_mfma32)
      asm volatile("" : "+s"(Kp));
      es_draw<BF3, SH>(*Kp, xs, lw, chain, it, c, h, lane, pc, e_state, t_state);
    }
  }
}

// ell and the target at given theta (ey_eslice_ell): a chain's carried ell comes from the evaluation that will be compared
// with it.
template <int WAVES, int BF3, typename SH>
__global__ void __launch_bounds__(WAVES * 64, 2) k_eslice_mfma_ell(EsKernArgs K) {
  constexpr int DKV = SH::DK;
  ES_FRAME();
  for (int64_t chain = first; chain < K.A.C; chain += stride) {
    EsKArgs* Kp = (EsKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(Kp));
    KArgs& A = Kp->A;
    EsEArgs& E = Kp->E;
    const float* thg = A.theta + chain * NPAR;
    const bool has_temp = A.temp != nullptr;
    const float temp = has_temp ? A.temp[chain] : 1.0f;
    Vec<DKV> p;
    const EsLoc loc = es_loc(E);
    for_each(p, c, h, lane, [&](float& v, int idx, bool) { v = thg[idx]; });
    float t;
    const float e = es_ell_at<BF3, SH, false>(A, E, xs, lw, p, loc, has_temp, temp, c, h, lane, pc, &t, p);
    if (E.ell) E.ell[chain] = e;
    if (A.target) A.target[chain] = t;
  }
}

// ----------------------------------------------------------------------------------------------- host side
template <bool ELL, int BF3, typename SH>
static int es_launch_v(EsKernArgs& k, int n_cu, hipStream_t s) {
  const size_t bytes = mf_lds_bytes(k.A.ntiles, 8, 0, BF3);
  const void* fn = ELL ? reinterpret_cast<const void*>(k_eslice_mfma_ell<8, BF3, SH>)
                       : reinterpret_cast<const void*>(k_eslice_mfma<8, BF3, SH>);
  // per launch, as mf_launch_v: function attributes are per device
  EY_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)mf_lds_bytes(BF3 ? MF_BF3_TILES : MF_MAX_TILES, 8, 0, BF3)));
  const unsigned grid = (unsigned)std::min<int64_t>(k.A.C, n_cu > 0 ? n_cu : 256);
  if (ELL) hipLaunchKernelGGL((k_eslice_mfma_ell<8, BF3, SH>), dim3(grid), dim3(512), bytes, s, k);
  else hipLaunchKernelGGL((k_eslice_mfma<8, BF3, SH>), dim3(grid), dim3(512), bytes, s, k);
  EY_HIP(hipGetLastError());
  return EY_OK;
}

#define ES_COMMA ,
// mf_launch's choice of form and shape: the headline model in both product forms, the other 4-32-32 models in bf16x3
template <bool ELL>
static int es_launch(ey_plan* pl, EsKernArgs& k, const void* base_loc, const void* base_scale, hipStream_t s) {
  const EyModel& m = pl->m;
  MfArgs& a = k.A;
  EsArgs& e = k.E;
  e.base_loc = (const float*)base_loc;
  e.base_scale = (const float*)base_scale;
  e.mu = (const float*)m.mu;
  e.inv_var = (const float*)m.inv_var;
  e.prior_uniform = pl->prior_uniform ? 1 : 0;
  e.mu0 = (float)pl->prior_mu0;
  e.iv0 = (float)pl->prior_iv0;
  e.prior_const = (float)m.prior_const;
  a.xpack = (const float*)pl->d_xpack;
  a.mu = e.mu;
  a.inv_var = e.inv_var;
  if (base_loc) {  // eval returns the log-target: the real prior
    a.prior_uniform = e.prior_uniform;
    a.mu0 = e.mu0;
    a.iv0 = e.iv0;
    a.prior_const = e.prior_const;
  } else {         // eval returns the (tempered) log-likelihood: a prior that adds exactly nothing
    a.prior_uniform = 1;
    a.mu0 = 0.0f;
    a.iv0 = 0.0f;
    a.prior_const = 0.0f;
  }
  a.ntiles = (m.N + 31) / 32;
  a.short_last = (m.N - 32 * (a.ntiles - 1)) <= 24 ? 1 : 0;
  const bool bf3 = pl->products == EY_PRODUCTS_BF16X3 && a.ntiles <= MF_BF3_TILES && !(t_ey_variant & 1);
  if (pl->mfma32_kind == 2) {
    if (!bf3) EY_FAIL(EY_ERR_UNSUPPORTED, "mfma32: this model is served in the bf16x3 form only");
    const int act = m.act[0];
    if (m.lik == EY_LIK_CE_SUM) {
      if (act == EY_ACT_TANH) return es_launch_v<ELL, 1, MfShape<3 ES_COMMA EY_ACT_TANH ES_COMMA EY_LIK_CE_SUM>>(k, pl->n_cu, s);
      return es_launch_v<ELL, 1, MfShape<3 ES_COMMA EY_ACT_RELU ES_COMMA EY_LIK_CE_SUM>>(k, pl->n_cu, s);
    }
    if (act == EY_ACT_SIGMOID) return es_launch_v<ELL, 1, MfShape<1 ES_COMMA EY_ACT_SIGMOID ES_COMMA EY_LIK_BCE_SUM>>(k, pl->n_cu, s);
    if (act == EY_ACT_TANH) return es_launch_v<ELL, 1, MfShape<1 ES_COMMA EY_ACT_TANH ES_COMMA EY_LIK_BCE_SUM>>(k, pl->n_cu, s);
    return es_launch_v<ELL, 1, MfShape<1 ES_COMMA EY_ACT_RELU ES_COMMA EY_LIK_BCE_SUM>>(k, pl->n_cu, s);
  }
  if (bf3) return es_launch_v<ELL, 1, MfHeadline>(k, pl->n_cu, s);
  return es_launch_v<ELL, 0, MfHeadline>(k, pl->n_cu, s);
}

int ey_eslice_mfma_launch(ey_plan* pl, void* theta, void* target, const EyEslice& es, const EyDraw& d) {
  EsKernArgs k = {};
  MfArgs& a = k.A;
  a.theta = (float*)theta; a.target = (float*)target; a.grad = (float*)theta;  // grad unused
  a.C = d.C; a.temp = (const float*)d.temp; a.seed = d.seed; a.iter = d.iter; a.chain_offset = d.chain_offset;
  a.accepted = (unsigned char*)d.accepted;
  a.n_iters = 1;
  if (const EyRun* run = d.run) {
    a.n_iters = run->n_iters;
    a.rec_samples = (float*)run->samples;
    a.rec_targets = (float*)run->targets;
    a.rec_accepted = (unsigned char*)run->accepted;
    a.accept_count = run->accept_count;
  }
  k.E.ell = (float*)es.ell; k.E.z = (const float*)es.z; k.E.u = (const float*)es.u; k.E.S = es.S;
  k.E.max_shrinks = es.max_shrinks; k.E.n_evals = es.n_evals; k.E.n_evals_rec = es.n_evals_rec;
  return es_launch<false>(pl, k, es.base_loc, es.base_scale, d.s);
}

int ey_eslice_mfma_ell_launch(ey_plan* pl, const void* theta, const void* base_loc, const void* base_scale,
                              const void* temp, int64_t C, void* ell, void* target, hipStream_t s) {
  EsKernArgs k = {};
  k.A.theta = (float*)theta; k.A.target = (float*)target; k.A.temp = (const float*)temp; k.A.C = C;
  k.A.n_iters = 1;
  k.E.ell = (float*)ell;
  return es_launch<true>(pl, k, base_loc, base_scale, s);
}
