// visual.hip -- image batches of the offline samplers on gfx950: frame
// stacking and the random crop of GCDataset / HGCDataset in one launch
// (include/ogbx_visual.h).
//
// Reference (hliuson/ogbench impls/utils/datasets.py):
//   random_crop / batched_random_crop        17-33
//   GCDataset.augment                        329-339
//   GCDataset.get_stacked_observations       359-366
//
// One workgroup per (sample, image column).  It recomputes the column's row
// selector from the index outputs of the fused sample kernel, resolves the F
// source rows from traj_end, stages those F frames (or a band of their rows
// when they exceed the LDS budget) in LDS with the widest aligned loads, and
// composes the output -- pixels of F * px_bytes bytes, shifted by the crop --
// from LDS in 16-byte units aligned to the destination.  An unstacked,
// uncropped column is a plain row copy and skips LDS.  The staging and the
// compose are visual_tile.h's, shared with atc.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ogbx_visual.h"
#include "common.h"
#include "gc_select.h"
#include "visual_tile.h"

namespace ogbx {

struct VisColumns {
  ogbx_visual_column c[OGBX_VISUAL_MAX_COLS];
};

struct VisArgs {
  const int64_t* traj_end;
  int64_t num_rows;
  const int64_t *idxs, *vg, *ag, *lvg;
  int64_t k_value, k_low, k_actor;  // HGC subgoal steps
  int32_t hgc;  // unread; kept so that every kernel-argument offset stays
  int32_t frame_stack, padding;
  int32_t draw;
  const int64_t* crop_from;
  int64_t* crop_out;
  uint32_t k0, k1, call_lo, call_hi;
  uint32_t lds_bytes;
  int32_t num_cols;
  int64_t total;
};

// The row a column's selector picks for sample s (numbering of
// ogbx_gc_column.select; every index clamped into the buffer).
__device__ inline int64_t select_row(const VisArgs& a, int sel, int64_t s) {
  const int64_t R = a.num_rows;
  const int64_t idx = clamp_row(a.idxs[s], R);
  if (sel == 0) return idx;
  if (sel == 1) return idx + 1 < R ? idx + 1 : R - 1;
  if (sel == 2) return clamp_row(a.vg[s], R);
  if (sel == 3) return clamp_row(a.ag[s], R);
  if (sel == 6) return clamp_row(a.lvg[s], R);
  const int64_t fin = a.traj_end[idx];
  int64_t next, steps;
  if (sel == 4 || sel == 5) {
    high_next(idx, fin, clamp_row(a.vg[s], R), sel == 4 ? a.k_value : a.k_low, &next, &steps);
  } else if (sel == 8) {
    next = idx + a.k_actor < fin ? idx + a.k_actor : fin;
  } else {  // 7 high actor next, 9 low actor next
    high_next(idx, fin, clamp_row(a.ag[s], R), sel == 7 ? a.k_actor : a.k_low, &next, &steps);
  }
  return clamp_row(next, R);
}

__global__ void __launch_bounds__(kVisThreads) visual_gather_kernel(VisArgs a, VisColumns cols) {
  extern __shared__ uint4 vis_lds4[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(vis_lds4);
  // consecutive workgroup ids go round-robin to the 8 XCDs: all columns of a
  // sample run on one XCD, so the frames its columns share (observations /
  // next_observations: F - 1 of F) are read from HBM once into that XCD's L2
  const int64_t b = blockIdx.x;
  const int64_t x = b & 7, i = b >> 3;
  const int64_t grp = i / a.num_cols;
  const int c = (int)(i - grp * a.num_cols);
  const int64_t s = grp * 8 + x;
  if (s >= a.total) return;
  const ogbx_visual_column& col = cols.c[c];
  const int t = threadIdx.x;

  const int64_t r = select_row(a, col.select, s);
  const int F = col.stack ? a.frame_stack : 1;
  const int64_t start = stack_start(a.traj_end, r, F);

  const int p = a.padding;
  int cy = p, cx = p;  // identity
  if (a.crop_from || a.draw) {
    int64_t oy, ox;
    crop_offsets(a.crop_from, s, p, a.k0, a.k1, a.call_lo, a.call_hi, &oy, &ox);
    if (col.crop) {
      cy = (int)oy;
      cx = (int)ox;
    }
    if (a.crop_out && c == 0 && t == 0) {
      a.crop_out[2 * s] = oy;
      a.crop_out[2 * s + 1] = ox;
    }
  }

  const int orb = col.width * (F * col.px_bytes);  // output row bytes
  uint8_t* dst = static_cast<uint8_t*>(col.dst) + s * ((int64_t)col.height * orb);
  compose_image(lds, a.lds_bytes, VisGeom{col.src, col.height, col.width, col.px_bytes}, r, start, F, cy, cx, p,
                dst);
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_visual_api_version(void) { return OGBX_VISUAL_API_VERSION; }

ogbx_status ogbx_visual_gather(const ogbx_gc_buffer* buf, const ogbx_hgc_config* hcfg,
                               const ogbx_visual_column* cols, int32_t num_cols, int64_t total,
                               const ogbx_visual_indices* indices, int32_t frame_stack, int32_t padding,
                               const int64_t* crop_from, int32_t draw_crop, uint64_t seed,
                               uint64_t call_index, int64_t* crop_out, void* stream) {
  const std::string who = "ogbx_visual_gather: ";
  OGBX_CHECK(buf && indices && (cols || num_cols == 0), OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(buf->num_rows > 0 && buf->traj_end, OGBX_EINVAL, who + "empty trajectory buffer");
  VisColumns vc{};
  uint32_t lds;
  int64_t blocks;
  const VisualCall v{indices,   hcfg,      total,    num_cols, frame_stack, padding,
                     crop_from, draw_crop, crop_out, seed,     call_index};
  GC_TRY(check_visual_gather(who, v, cols, 0, "at most 16 columns", true, &vc, &lds, &blocks));
  if (num_cols == 0) return OGBX_OK;

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  OGBX_CHECK(on_device(buf->traj_end, dev) &&
                 visual_pointers_on_device(dev, v, cols),
             OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  VisArgs a{};
  a.traj_end = buf->traj_end;
  a.num_rows = buf->num_rows;
  a.hgc = hcfg != nullptr;
  fill_visual_args(a, v, lds);
  hipLaunchKernelGGL(visual_gather_kernel, dim3((uint32_t)blocks), dim3(kVisThreads), lds, (hipStream_t)stream, a,
                     vc);
  OGBX_LAUNCHED("visual_gather_kernel");
  return OGBX_OK;
}

}  // extern "C"
