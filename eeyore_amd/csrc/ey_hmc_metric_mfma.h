// What ey_api.hip and ey_hmc_metric_mfma.hip share about HMC under a diagonal metric on the matrix cores
// (include/eeyore_amd_hmc_metric_fused.h).
#pragma once

#include "../../include/eeyore_amd_hmc_metric_fused.h"  // includes the other eight headers
#include "ey_common.h"

// k_hmc_metric_mfma (ey_hmc_metric_mfma.hip): the draw of k_hmc_metric's diagonal form and the epilogues of
// k_hmc_metric_warmup for the plans the mfma32 family serves.  The caller has checked the family and the form.  v0, u,
// rate, hcur, hprop: those of a step, null in a run; step_vec is in/out when w carries a dual averaging.
int ey_hmc_metric_mfma_launch(ey_plan* pl, void* theta, void* target, void* grad, const void* metric, int64_t G,
                              const void* metric_index, const void* v0, const void* u, double step, void* step_vec, int L,
                              const EyDraw& d, void* rate, void* hcur, void* hprop, const EyWarm& w);
