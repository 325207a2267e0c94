// What ey_api.hip and ey_eslice.hip share about elliptical slice sampling (include/eeyore_amd_eslice.h).
#pragma once

#include "../../include/eeyore_amd_eslice_fused.h"  // includes eeyore_amd_eslice.h and the other four
#include "ey_common.h"

// the arguments of k_eslice beside a draw's: the base, parity inputs, the shrink cap, what a draw carries and leaves
struct EyEslice {
  const void* base_loc;    // [P] or null (with base_scale: the plan's Normal prior)
  const void* base_scale;  // [P] or null
  const void* z;           // [C,P] or null
  const void* u;           // [C,S] or null
  int64_t S;
  int max_shrinks;
  void* ell;         // [C] of the plan's dtype, in/out
  int* n_evals;      // [C] or null
  int* n_evals_rec;  // [n_iters,C] or null
};

size_t ey_eslice_lds(const ey_plan* pl);  // dynamic LDS of one chain's workgroup
// the LDS limit, before any launch; then the launch of k_eslice
int ey_eslice_launch(ey_plan* pl, void* theta, void* target, const EyEslice& es, const EyDraw& d);
// ... of k_eslice_ell: ell and target [C] at theta, either may be null
int ey_eslice_ell_launch(ey_plan* pl, const void* theta, const void* base_loc, const void* base_scale, const void* temp,
                         int64_t C, void* ell, void* target, hipStream_t s);

// The same two on the matrix cores (ey_eslice_mfma.hip: k_eslice_mfma, k_eslice_mfma_ell), for the f32 plans
// the mfma32 family serves.  The caller has checked that it does: these refuse nothing but a form that is not built.
int ey_eslice_mfma_launch(ey_plan* pl, void* theta, void* target, const EyEslice& es, const EyDraw& d);
int ey_eslice_mfma_ell_launch(ey_plan* pl, const void* theta, const void* base_loc, const void* base_scale,
                              const void* temp, int64_t C, void* ell, void* target, hipStream_t s);
