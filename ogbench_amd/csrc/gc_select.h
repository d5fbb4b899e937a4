// gc_select.h -- row-selector arithmetic shared by the sample kernels
// (gcsample.hip) and the visual gather (visual.hip).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ogbx {

// HGC column selectors: 0 idx, 1 next, 2 high value goal, 3 high actor goal,
// 4 high value next, 5 low value next, 6 low value goal, 7 high actor next,
// 8 low actor goal, 9 low actor next (ogbx_hgc_sample).
constexpr int kHgcSel = 10;

// HGCDataset.compute_high_next_idxs (datasets.py:478-491) for one sample.
__device__ inline void high_next(int64_t idx, int64_t fin, int64_t goal, int64_t K, int64_t* next,
                                 int64_t* steps) {
  int64_t st = K < fin - idx ? K : fin - idx;
  const int64_t diff = goal - idx;
  if (0 <= diff && diff < st) st = diff;
  *steps = st;
  *next = idx + st;
}

}  // namespace ogbx
