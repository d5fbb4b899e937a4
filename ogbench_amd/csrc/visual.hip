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
  int32_t hgc;
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
  OGBX_CHECK(indices->idxs, OGBX_EINVAL, who + "indices->idxs is required");
  OGBX_CHECK(num_cols >= 0 && num_cols <= OGBX_VISUAL_MAX_COLS, OGBX_EINVAL, who + "at most 16 columns");
  OGBX_CHECK(total > 0, OGBX_EINVAL, who + "total must be > 0");
  OGBX_CHECK(frame_stack >= 1 && frame_stack <= OGBX_VISUAL_MAX_STACK, OGBX_EINVAL,
             who + "frame_stack must be in 1..8");
  OGBX_CHECK(padding >= 0 && padding < (1 << 20), OGBX_EINVAL, who + "padding must be >= 0");
  OGBX_CHECK(!crop_out || crop_from || draw_crop, OGBX_EINVAL, who + "crop_out without crop offsets");
  if (hcfg)
    OGBX_CHECK(hcfg->value_subgoal_steps >= 0 && hcfg->low_subgoal_steps >= 0 && hcfg->actor_subgoal_steps >= 0,
               OGBX_EINVAL, who + "negative subgoal steps");
  const int max_select = hcfg ? kHgcSel - 1 : 3;
  VisColumns vc{};
  uint32_t lds = 16;
  for (int i = 0; i < num_cols; ++i) {
    const ogbx_visual_column& c = cols[i];
    OGBX_CHECK(c.src && c.dst, OGBX_EINVAL, who + "null column pointer");
    OGBX_CHECK(c.height > 0 && c.width > 0 && c.px_bytes > 0, OGBX_EINVAL, who + "bad image shape");
    OGBX_CHECK(c.select >= 0 && c.select <= max_select, OGBX_EINVAL, who + "selector out of range");
    const int s = c.select;
    const bool need_v = s == 2 || s == 4 || s == 5, need_a = s == 3 || s == 7 || s == 9, need_l = s == 6;
    OGBX_CHECK((!need_v || indices->value_goal_idxs) && (!need_a || indices->actor_goal_idxs) &&
                   (!need_l || indices->low_value_goal_idxs),
               OGBX_EINVAL, who + "a column selects through a missing index output");
    const int64_t F = c.stack ? frame_stack : 1;
    const int64_t row_bytes = (int64_t)c.width * c.px_bytes, frame = row_bytes * c.height;
    OGBX_CHECK(frame * F <= (1ll << 30), OGBX_EINVAL, who + "image too large");
    lds = std::max<uint32_t>(lds, vis_lds_bytes(frame, F));
    vc.c[i] = c;
  }
  for (int i = 0; i < num_cols; ++i) {  // at least one image row per staged frame
    const uint32_t F = cols[i].stack ? (uint32_t)frame_stack : 1u;
    OGBX_CHECK((int64_t)((lds / F) & ~15u) >= (int64_t)cols[i].width * cols[i].px_bytes, OGBX_EINVAL,
               who + "image row too wide to stage");
  }
  const int64_t blocks = ((total + 7) / 8) * 8 * num_cols;
  OGBX_CHECK(blocks <= 0x7fffffffll, OGBX_EINVAL, who + "too many (sample, column) pairs for one launch");
  if (num_cols == 0) return OGBX_OK;

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = on_device(buf->traj_end, dev) && on_device(indices->idxs, dev);
  for (const int64_t* q : {indices->value_goal_idxs, indices->actor_goal_idxs, indices->low_value_goal_idxs,
                           crop_from, (const int64_t*)crop_out})
    ok = ok && (!q || on_device(q, dev));
  for (int i = 0; i < num_cols; ++i) ok = ok && on_device(cols[i].src, dev) && on_device(cols[i].dst, dev);
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  VisArgs a{};
  a.traj_end = buf->traj_end;
  a.num_rows = buf->num_rows;
  a.idxs = indices->idxs;
  a.vg = indices->value_goal_idxs;
  a.ag = indices->actor_goal_idxs;
  a.lvg = indices->low_value_goal_idxs;
  if (hcfg) {
    a.k_value = hcfg->value_subgoal_steps;
    a.k_low = hcfg->low_subgoal_steps;
    a.k_actor = hcfg->actor_subgoal_steps;
    a.hgc = 1;
  }
  a.frame_stack = frame_stack;
  a.padding = padding;
  a.draw = draw_crop != 0 && !crop_from;
  a.crop_from = crop_from;
  a.crop_out = crop_out;
  seed_key(seed, hcfg ? kTagHgcSample : kTagGcSample, &a.k0, &a.k1);
  a.call_lo = (uint32_t)call_index;
  a.call_hi = (uint32_t)(call_index >> 32);
  a.lds_bytes = lds;
  a.num_cols = num_cols;
  a.total = total;
  hipLaunchKernelGGL(visual_gather_kernel, dim3((uint32_t)blocks), dim3(kVisThreads), lds, (hipStream_t)stream, a,
                     vc);
  OGBX_LAUNCHED("visual_gather_kernel");
  return OGBX_OK;
}

}  // extern "C"
