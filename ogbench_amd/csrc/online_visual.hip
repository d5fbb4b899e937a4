// online_visual.hip -- image batches over the on-device episode ring on
// gfx950: frame stacking and the random crop of GCDataset / HGCDataset over
// the snapshot of an ogbx_online_ring in one launch
// (include/ogbx_online_visual.h).
//
// Reference (hliuson/ogbench impls/utils/datasets.py):
//   random_crop / batched_random_crop        17-33
//   GCDataset.augment                        329-339
//   GCDataset.get_stacked_observations       359-366
// over the snapshot of the ring (include/ogbx_online.h): the live rows
// unrolled env-major, flat index u = e * L + k for env e at step S - L + k.
//
// online_visual_gather_kernel: visual_gather_kernel's work layout (visual.hip)
// -- one workgroup per (sample, image column), all columns of a sample on one
// XCD -- with the index loads replaced by the ring's.  The workgroup
// recomputes the column's selector from the flat index outputs of the sample
// kernel (split_flat, episode_seq / episode_end_flat of online_device.h,
// high_next of gc_select.h: the arithmetic of online_gc_sample_kernel and
// online_hgc_sample_kernel), which leaves it with an env e and a live offset
// k.  The stack's first row comes from the row's own ep_seq and at most F - 1
// candidates, loaded together: offsets below 0 are dead steps and are not
// read, for their slots hold newer rows of the same env.  The F source frames
// then sit at unrelated physical rows ((slot0 + k') % T) * N + e, one of them
// possibly in a second array (a column's alt: next_observations on selector
// 0), and visual_tile.h stages and composes them through compose_frames.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ogbx_online_visual.h"
#include "common.h"
#include "gc_select.h"
#include "online_device.h"
#include "visual_tile.h"

namespace ogbx {

struct OnVisColumns {
  ogbx_online_visual_column c[OGBX_VISUAL_MAX_COLS];
};

struct OnVisArgs {
  OnlineView ring;
  const int64_t *idxs, *vg, *ag, *lvg;
  int64_t k_value, k_low, k_actor;  // HGC subgoal steps
  int32_t frame_stack, padding;
  int32_t draw;
  int32_t num_cols;
  const int64_t* crop_from;
  int64_t* crop_out;
  uint32_t k0, k1, call_lo, call_hi;
  uint32_t lds_bytes;
  int64_t total;
};

// The env and the live offset of the row a column's selector picks for sample
// s (numbering of ogbx_online_hgc_sample; every flat index clamped into
// [0, L * N)).  The five derived selectors stay in [idx, fin], the sample's
// env, as in online_hgc_sample_kernel: e < N and k < L either way.
__device__ inline void select_ring_row(const OnVisArgs& a, int sel, int64_t s, int64_t* e, int64_t* k) {
  const OnlineView& ring = a.ring;
  const int64_t np = ring.npick;
  const int64_t* direct = sel == 2 ? a.vg : (sel == 3 ? a.ag : (sel == 6 ? a.lvg : a.idxs));
  const int64_t u = clamp_row(direct[s], np);
  split_flat(ring, u, e, k);
  if (sel == 0 || sel == 2 || sel == 3 || sel == 6) return;
  // u is the sample's row; its episode's end, then the subgoal arithmetic
  const int64_t fin = episode_end_flat(ring, episode_seq(ring, *e, phys_row(ring, *e, *k)), u, *e, *k);
  int64_t next, steps;
  if (sel == 4 || sel == 5) {
    high_next(u, fin, clamp_row(a.vg[s], np), sel == 4 ? a.k_value : a.k_low, &next, &steps);
  } else if (sel == 8) {
    steps = a.k_actor < fin - u ? a.k_actor : fin - u;
  } else {  // 7 high actor next, 9 low actor next
    high_next(u, fin, clamp_row(a.ag[s], np), sel == 7 ? a.k_actor : a.k_low, &next, &steps);
  }
  *k += steps;  // 0 <= steps <= fin - u, and fin <= e * L + L - 1
}

__global__ void __launch_bounds__(kVisThreads) online_visual_gather_kernel(OnVisArgs a, OnVisColumns cols) {
  extern __shared__ uint4 onvis_lds4[];  // 16-byte aligned
  uint8_t* lds = reinterpret_cast<uint8_t*>(onvis_lds4);
  // all columns of a sample on one XCD: see visual_gather_kernel
  const int64_t b = blockIdx.x;
  const int64_t x = b & 7, i = b >> 3;
  const int64_t grp = i / a.num_cols;
  const int c = (int)(i - grp * a.num_cols);
  const int64_t s = grp * 8 + x;
  if (s >= a.total) return;
  const ogbx_online_visual_column& col = cols.c[c];
  const int t = threadIdx.x;
  const OnlineView& ring = a.ring;

  int64_t e, k;
  select_ring_row(a, col.select, s, &e, &k);
  const int F = col.stack ? a.frame_stack : 1;
  const uint8_t* __restrict__ src = static_cast<const uint8_t*>(col.src);
  const uint8_t* __restrict__ alt = static_cast<const uint8_t*>(col.alt);
  const int n = alt ? F - 1 : F;  // frames from src; alt's is the newest block
  const int64_t kfirst = stack_first(ring, e, k, n);

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

  const int64_t fb = (int64_t)col.height * (col.width * col.px_bytes);  // source frame bytes
  uint8_t* dst = static_cast<uint8_t*>(col.dst) + s * (fb * F);
  compose_frames(lds, a.lds_bytes, col.height, col.width, col.px_bytes, F, cy, cx, p, dst,
                 [&](int j) -> const uint8_t* {
                   if (alt && j == F - 1) return alt + phys_row(ring, e, k) * fb;
                   int64_t kj = k - (n - 1 - j);
                   kj = kj < kfirst ? kfirst : kj;  // kfirst >= 0: a live row
                   return src + phys_row(ring, e, kj) * fb;
                 });
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_online_visual_api_version(void) { return OGBX_ONLINE_VISUAL_API_VERSION; }

ogbx_status ogbx_online_visual_gather(const ogbx_online_ring* ring, const ogbx_hgc_config* hcfg,
                                      const ogbx_online_visual_column* cols, int32_t num_cols, int64_t total,
                                      const ogbx_visual_indices* indices, int32_t frame_stack, int32_t padding,
                                      const int64_t* crop_from, int32_t draw_crop, uint64_t seed,
                                      uint64_t call_index, int64_t* crop_out, void* stream) {
  const std::string who = "ogbx_online_visual_gather: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(cols && indices, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  OnVisColumns vc{};
  uint32_t lds;
  int64_t blocks;
  const VisualCall v{indices,   hcfg,      total,    num_cols, frame_stack, padding,
                     crop_from, draw_crop, crop_out, seed,     call_index};
  GC_TRY(check_visual_gather(who, v, cols, 1, "1 to 16 columns", false, &vc, &lds, &blocks));

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = all_on_device(dev, {ring->ep_seq, ring->cur_seq, ring->ep_end}) &&
            visual_pointers_on_device(dev, v, cols);
  for (int i = 0; i < num_cols && ok; ++i) ok = all_on_device(dev, {cols[i].alt});
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  OnVisArgs a{};
  a.ring = online_view(*ring);
  fill_visual_args(a, v, lds);
  hipLaunchKernelGGL(online_visual_gather_kernel, dim3((uint32_t)blocks), dim3(kVisThreads), lds,
                     (hipStream_t)stream, a, vc);
  OGBX_LAUNCHED("online_visual_gather_kernel");
  return OGBX_OK;
}

}  // extern "C"
