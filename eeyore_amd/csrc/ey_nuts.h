// What ey_api.hip, ey_nuts.hip, ey_nuts_ws.hip and ey_nuts_mfma.hip share about the No-U-Turn sampler
// (include/eeyore_amd_nuts.h, include/eeyore_amd_nuts_tree.h, include/eeyore_amd_nuts_fused.h).
#pragma once

#include "../../include/eeyore_amd_nuts_fused.h"  // includes eeyore_amd_nuts_tree.h, eeyore_amd_nuts.h and the other six
#include "ey_common.h"

// the arguments of k_nuts beside those of ey_generic_hmc_metric_warmup: parity inputs, the depth cap, the outputs of a draw
struct EyNuts {
  const void* v0;  // [C,P] or null
  const void* u;   // [C,S] or null
  int64_t S;
  int max_depth;
  int* depth;                // [C] or null
  int* n_leapfrog;           // [C] or null
  unsigned char* divergent;  // [C] or null
  void* energy;              // [C] of the plan's dtype, or null (accept_stat travels as EyDraw::log_rate)
  int* depth_rec;            // [n_iters,C] or null
  unsigned char* div_rec;    // [n_iters,C] or null
};

size_t ey_nuts_lds(const ey_plan* pl, int form);  // dynamic LDS of one chain's workgroup
// the limits (P, LDS), before any launch; then the launch of k_nuts.  step_vec is in/out when w carries a dual averaging.
int ey_nuts_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int form, int64_t G,
                   const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                   const EyWarm& w);

// k_nuts_ws (ey_nuts_ws.hip): the diagonal form with the tree in the plan's attached workspace (ey_plan::nuts_tree), any P
// the evaluation image holds.  The bytes of the workspace for C chains at max_depth; the LDS limit, then the launch.
int64_t ey_nuts_ws_bytes(const ey_plan* pl, int64_t C, int max_depth);
int ey_nuts_ws_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                      const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                      const EyWarm& w);

// k_nuts_mfma (ey_nuts_mfma.hip): the same draw on the matrix cores for the plans the mfma32 family serves, the tree in the
// same workspace and layout.  The caller has checked the family, the form and the workspace.
int ey_nuts_mfma_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                        const void* metric_index, double step, void* step_vec, const EyDraw& d, const EyNuts& nu,
                        const EyWarm& w);

// The launch of one wave per chain.  The LDS limit of an instantiation is raised once per plan, to the whole 160 KiB
// (DESIGN.md 4.9.1): the limit belongs to the kernel, not to a launch, and `attr` is the plan's slot for the kernel that has
// it (ey_plan::nuts_attr, ey_plan::nuts_ws_attr).
template <typename... Ps, typename... As>
static int launch_nuts_kernel(const void** attr, void (*kernel)(Ps...), int64_t C, size_t bytes, hipStream_t s, As... args) {
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (bytes > 48 * 1024 && *attr != fn) {
    EY_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    *attr = fn;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)C), dim3(64), bytes, s, args...);
  EY_HIP(hipGetLastError());
  return EY_OK;
}
