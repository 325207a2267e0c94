// k_nuts_ws: k_nuts (ey_nuts.hip) under a DIAGONAL metric with the tree's vectors in a caller-provided device workspace
// instead of LDS, so that P is bounded by the evaluation image alone (include/eeyore_amd_nuts_tree.h).  A
// translation unit of its own beside ey_nuts.hip, on the same share of ey_generic.hip (EY_GEN_PART 1) and on the same text
// of the draw (ey_nuts_draw.h): the same Philox words, the same per-lane partial sums through wave_sum, the same epilogues.
#define EY_GEN_PART 1
#include "ey_generic.hip"

#include "ey_nuts.h"

// LDS holds k_hmc_metric's diagonal image only: theta, the gradient, v, the scales and the model's image.  The workspace of
// chain c is nvec = 12 + 2 max_depth vectors of Ppad = P rounded up to 64 elements at ws + c nvec Ppad, in k_nuts's order.
__host__ __device__ static int nuts_ws_ppad(int P) { return (P + WAVE - 1) & ~(WAVE - 1); }
__host__ __device__ static int nuts_ws_nvec(int max_depth) { return 12 + 2 * max_depth; }

// the draw itself: ey_nuts_draw.h writes the body of the kernel named here
#define NUTS_TREE_IN_WS 1
#define NUTS_KERNEL_HEAD                                                                                                \
  template <typename T, class TINY>                                                                                     \
  __global__ void __launch_bounds__(WAVE) k_nuts_ws(EyModel m, T* theta, T* target, T* grad, const T* metric, int64_t G, \
                                                    const int* metric_index, const T* v0, const T* u_in, int64_t S_u,   \
                                                    T step, T* step_vec, int max_depth, int recompute, EyNuts nu,       \
                                                    EyWarm w, T* ws,                                                    \
                                                    const T* temp, uint64_t seed, uint64_t iter0, uint64_t chain_offset, \
                                                    unsigned char* accepted, T* rate_o, EyRun run, int64_t C)
#include "ey_nuts_draw.h"

template <typename T, class TINY>
static int launch_nuts_ws(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                          const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                          const EyWarm& w) {
  const size_t bytes = hmc_metric_lds(pl->m, EY_METRIC_DIAG, sizeof(T));
  const int recompute = (d.flags & EY_RECOMPUTE_INITIAL_GRAD) != 0;
  return launch_nuts_kernel(&pl->nuts_ws_attr, k_nuts_ws<T, TINY>, d.C, bytes, d.s, pl->m, (T*)theta, (T*)target,
                            (T*)grad, (const T*)metric, G, (const int*)metric_index, (const T*)nu.v0, (const T*)nu.u, nu.S,
                            (T)step, (T*)step_vec, nu.max_depth, recompute, nu, w, (T*)pl->nuts_tree, EY_DRAW_ARGS(T, d));
}

int64_t ey_nuts_ws_bytes(const ey_plan* pl, int64_t C, int max_depth) {
  return C * (int64_t)nuts_ws_nvec(max_depth) * nuts_ws_ppad(pl->m.P) * (pl->dtype == EY_F32 ? 4 : 8);
}

// The caller (nuts_impl, ey_api.hip) has checked the form, the attached workspace and its size for this (C, max_depth).
int ey_nuts_ws_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                      const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                      const EyWarm& w) {
  const size_t bytes = hmc_metric_lds(pl->m, EY_METRIC_DIAG, pl->dtype == EY_F32 ? 4 : 8);
  if (int rc = diag_limit("NUTS", bytes)) return rc;
  if (!pl->nuts_tree || pl->nuts_tree_bytes < ey_nuts_ws_bytes(pl, d.C, nu.max_depth))  // (never: see above)
    EY_FAIL(EY_ERR_INVALID, "NUTS with the tree in device memory: no workspace of this call's size is attached");
  return EY_TINY_DISPATCH(tiny_dispatch, launch_nuts_ws, pl, theta, target, grad, metric, G, metric_index, step, step_vec,
                          d, nu, w);
}
