// k_nuts: the No-U-Turn sampler under a fixed metric (include/eeyore_amd_nuts.h).  A sibling of k_hmc_metric
// in a translation unit of its own, so that it builds beside ey_generic.hip: that file is included for what the kernels share
// (EY_GEN_PART 1 there: the evaluation, the LDS image, EY_METRIC_KICK / EY_METRIC_DRIFT, the launch helpers) with every entry
// point and kernel instantiation of its own left out.
#define EY_GEN_PART 1
#include "ey_generic.hip"

#include "ey_nuts.h"

// The tree lives in LDS behind k_hmc_metric's image (and the packed factor where there is one): NUTS_NVEC vectors of P
// rounded up to 4 elements, in the order ey_nuts_draw.h lists.
#define NUTS_NVEC (12 + 2 * EY_NUTS_MAX_DEPTH)

__host__ __device__ static size_t nuts_lds(const EyModel& m, int form, size_t esz) {
  return hmc_metric_lds(m, form, esz) + esz * (size_t)NUTS_NVEC * ((m.P + 3) & ~3);
}

// the draw itself: ey_nuts_draw.h writes the body of the kernel named here
#define NUTS_TREE_IN_WS 0
#define NUTS_KERNEL_HEAD                                                                                             \
  template <typename T, class TINY, int FORM>                                                                        \
  __global__ void __launch_bounds__(WAVE) k_nuts(EyModel m, T* theta, T* target, T* grad, const T* metric, int64_t G, \
                                                 const int* metric_index, const T* v0, const T* u_in, int64_t S_u, T step, \
                                                 T* step_vec, int max_depth, int recompute, EyNuts nu, EyWarm w,     \
                                                 const T* temp, uint64_t seed, uint64_t iter0, uint64_t chain_offset, \
                                                 unsigned char* accepted, T* rate_o, EyRun run, int64_t C)
#include "ey_nuts_draw.h"

template <typename T, class TINY>
static int launch_nuts(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                       const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                       const EyWarm& w) {
  const size_t bytes = ey_nuts_lds(pl, form);
  const int recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) != 0;
  if (form == EY_METRIC_TRIL)
    return launch_nuts_kernel(&pl->nuts_attr, k_nuts<T, TINY, EY_METRIC_TRIL>, d.C, bytes, d.s, pl->m, (T*)theta,
                              (T*)target, (T*)grad, (const T*)metric, G, (const int*)metric_index, (const T*)nu.v0,
                              (const T*)nu.u, nu.S, (T)step, (T*)step_vec, nu.max_depth, recompute, nu, w,
                              EY_DRAW_ARGS(T, d));
  return launch_nuts_kernel(&pl->nuts_attr, k_nuts<T, TINY, EY_METRIC_DIAG>, d.C, bytes, d.s, pl->m, (T*)theta,
                            (T*)target, (T*)grad, (const T*)metric, G, (const int*)metric_index, (const T*)nu.v0,
                            (const T*)nu.u, nu.S, (T)step, (T*)step_vec, nu.max_depth, recompute, nu, w,
                            EY_DRAW_ARGS(T, d));
}

size_t ey_nuts_lds(const ey_plan* pl, int form) { return nuts_lds(pl->m, form, pl->dtype == EY_F32 ? 4 : 8); }

int ey_nuts_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                   const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                   const EyWarm& w) {
  if (int rc = tril_limits(pl, "NUTS", "the tree", "the tree's vectors, the metric", ey_nuts_lds(pl, form))) return rc;
  return EY_TINY_DISPATCH(tiny_dispatch, launch_nuts, pl, theta, target, grad, metric, form, G, metric_index, step,
                          step_vec, d, nu, w);
}
