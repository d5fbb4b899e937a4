/* ogbx_visual.h -- visual (image) batches for the offline samplers: frame
 * stacking and the random crop of GCDataset / HGCDataset
 * (hliuson/ogbench impls/utils/datasets.py:17-33, 329-366).
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_visual_api_version()); OGBX_ABI_VERSION covers ogbx.h
 * alone.  Conventions (status codes, ogbx_last_error(), streams, device
 * pointers) are those of ogbx.h.
 *
 * A sampler runs ogbx_gc_sample / ogbx_hgc_sample over its non-image columns
 * with the index outputs requested, then ONE ogbx_visual_gather over the image
 * columns on the same stream.  The gather recomputes the row selectors of
 * every sample from those indices (same numbering as ogbx_gc_column.select),
 * resolves the frame_stack source rows of each selector from traj_end, and
 * writes every image column of every sample.
 */
#ifndef OGBX_VISUAL_H_
#define OGBX_VISUAL_H_

#include "ogbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_VISUAL_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_visual_api_version(void);

#define OGBX_VISUAL_MAX_COLS 16
#define OGBX_VISUAL_MAX_STACK 8
/* Philox draw slot (counter word 2) of the crop offsets.  The sample kernels
 * use slots 0..6 of the counter {sample_lo, call_lo, slot, sample_hi ^
 * call_hi}; this one is theirs never, so no existing stream moves
 * (OGBX_STREAM_VERSION is unchanged). */
#define OGBX_VISUAL_CROP_SLOT 8

/* One image column.  The source holds UNSTACKED frames, dense
 * [R, height, width, px_bytes]; a row of a non-image array is a 1 x 1 image
 * with px_bytes = its row bytes.  The destination is dense
 * [total, height, width, F * px_bytes] with F = frame_stack when `stack` is
 * set, else 1.  Channel block j (0..F-1) of selector row r is the frame at
 * row max(r - (F-1-j), first row of r's trajectory)
 * (get_stacked_observations, datasets.py:359-366); row r-s belongs to r's
 * trajectory iff r-s >= 0 and traj_end[r-s] == traj_end[r]. */
typedef struct {
  const void* src;
  void* dst;
  int32_t height, width;
  int32_t px_bytes; /* bytes of one pixel of ONE frame (channels * itemsize) */
  int32_t select;   /* row selector, numbered as ogbx_gc_column.select:
                       0..3 (GC) or 0..9 (HGC, see ogbx_hgc_sample)           */
  int32_t stack;    /* 1: stack frame_stack frames; 0: the selector's frame   */
  int32_t crop;     /* 1: apply the sample's crop offsets; 0: never cropped   */
} ogbx_visual_column;

/* The index outputs of the fused sample call, device int64 [total].
 * value_goal_idxs / actor_goal_idxs are the GC value / actor goals or the HGC
 * high-level value / actor goals.  A pointer may be NULL when no column
 * selects through it (GC: 2 needs value, 3 actor; HGC: 2, 4, 5 need value,
 * 3, 7, 9 actor, 6 low_value). */
typedef struct {
  const int64_t* idxs;
  const int64_t* value_goal_idxs;
  const int64_t* actor_goal_idxs;
  const int64_t* low_value_goal_idxs;
} ogbx_visual_indices;

/* Gather every image column of `total` samples in ONE launch.
 *
 * hcfg: NULL for GCDataset selectors (0 idx, 1 min(idx+1, R-1), 2 value goal,
 *   3 actor goal); the sampler's ogbx_hgc_config for the ten HGC selectors
 *   (only its *_subgoal_steps are read).
 * frame_stack: F in 1..OGBX_VISUAL_MAX_STACK.
 * padding >= 0: the crop pads by `padding` edge pixels and cuts an image-sized
 *   window at crop_from = (cy, cx), cy, cx in [0, 2 padding]:
 *     out[y, x, :] = img[clamp(y + cy - padding, 0, H-1),
 *                        clamp(x + cx - padding, 0, W-1), :]
 *   (random_crop, datasets.py:17-27), one (cy, cx) per sample shared by all of
 *   its cropped columns, applied after stacking.
 * Crop offsets: crop_from (device int64 [total, 2]) when non-NULL; else, when
 *   draw_crop != 0, Philox words x, y of the counter
 *   {sample_lo, call_lo, OGBX_VISUAL_CROP_SLOT, sample_hi ^ call_hi} under the
 *   sampler's key (seed and the GC or HGC stream tag), each reduced to
 *   [0, 2 padding] by multiply-high; else no crop (identity).
 * crop_out: optional device int64 [total, 2], receives the offsets used (only
 *   with crop_from or draw_crop).
 * Every pointer must be device memory of the current device (OGBX_EINVAL
 * otherwise).  Indices outside [0, R) are clamped into the buffer. */
ogbx_status ogbx_visual_gather(const ogbx_gc_buffer* buf, const ogbx_hgc_config* hcfg,
                               const ogbx_visual_column* cols, int32_t num_cols, int64_t total,
                               const ogbx_visual_indices* indices, int32_t frame_stack, int32_t padding,
                               const int64_t* crop_from, int32_t draw_crop, uint64_t seed,
                               uint64_t call_index, int64_t* crop_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_VISUAL_H_ */
