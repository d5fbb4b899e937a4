/* ogbx_online_visual.h -- visual (image) batches over the on-device episode
 * ring: frame stacking and the random crop of GCDataset / HGCDataset
 * (hliuson/ogbench impls/utils/datasets.py:17-33, 329-366) over the snapshot
 * of an ogbx_online_ring (include/ogbx_online.h).
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_online_visual_api_version()); OGBX_ABI_VERSION,
 * OGBX_STREAM_VERSION and the versions of the other extension headers are
 * unchanged.  Conventions (status codes, ogbx_last_error(), streams, device
 * pointers) are those of ogbx.h; the index outputs, the crop and its Philox
 * slot are those of ogbx_visual.h.
 *
 * A sampler runs ogbx_online_gc_sample / ogbx_online_hgc_sample over its
 * non-image columns with the index outputs requested, then ONE
 * ogbx_online_visual_gather over the image columns on the same stream, with
 * the same ring->steps.  The ring holds UNSTACKED frames; the gather
 * recomputes the row selectors of every sample from the flat index outputs
 * (u = e * L + k), resolves the frame_stack source rows of each selector from
 * ep_seq, and writes every image column of every sample.
 *
 * The stack.  Let t = S - L + k be the logical step of a selector row of env
 * e.  A row at step t' <= t of env e belongs to its episode iff t' >= S - L
 * (the row is live: the slot of a dead step holds a newer step of the same
 * env, whose ep_seq is equal for an env that is never done) and
 * ep_seq[(t' % T) * N + e] == ep_seq[(t % T) * N + e].  With s0 the earliest
 * such step among t - (F-1) .. t, channel block j (0..F-1) is the frame at
 * step max(t - (F-1-j), s0): get_stacked_observations (datasets.py:359-366)
 * over the snapshot, where an episode whose head was overwritten starts at its
 * oldest live row.
 */
#ifndef OGBX_ONLINE_VISUAL_H_
#define OGBX_ONLINE_VISUAL_H_

#include "ogbx.h"
#include "ogbx_online.h"
#include "ogbx_visual.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_ONLINE_VISUAL_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_online_visual_api_version(void);

/* One image column.  src is a column of the ring, dense
 * [T * N, height, width, px_bytes]; a row of a non-image array is a 1 x 1
 * image with px_bytes = its row bytes.  The destination is dense
 * [total, height, width, F * px_bytes] with F = frame_stack when `stack` is
 * set, else 1.
 *
 * alt: optional second source of the same geometry (another column of the
 * ring).  Its frame at the selector's row replaces the newest block, and the
 * F - 1 blocks before it are the F - 1 newest blocks of the stack over src:
 * block j < F-1 is the src frame at step max(t - (F-2-j), s0), block F-1 the
 * alt frame at step t.  With src = observations, alt = next_observations and
 * select 0 this is the stacked next_observations of a ring that stores its
 * own: on histories with next_observations[t] == observations[t+1] inside an
 * episode, get_observations(idxs + 1) over the compact unrolling of the
 * snapshot. */
typedef struct {
  const void* src;
  const void* alt;
  void* dst;
  int32_t height, width;
  int32_t px_bytes; /* bytes of one pixel of ONE frame (channels * itemsize) */
  int32_t select;   /* row selector: 0, 2, 3 (ogbx_online_gc_sample) or 0,
                       2..9 (ogbx_online_hgc_sample); 1, the next row, is
                       refused: the ring stores its own next_observations     */
  int32_t stack;    /* 1: stack frame_stack frames; 0: the selector's frame   */
  int32_t crop;     /* 1: apply the sample's crop offsets; 0: never cropped   */
} ogbx_online_visual_column;

/* Gather every image column of `total` samples in ONE launch of
 * online_visual_gather_kernel.  Needs ring->steps >= 1.
 *
 * hcfg: NULL for the GC selectors; the sampler's ogbx_hgc_config for the HGC
 *   selectors (only its *_subgoal_steps are read).
 * indices: the flat index outputs of the sample call (ogbx_visual.h); a
 *   pointer may be NULL when no column selects through it.
 * frame_stack, padding, crop_from, draw_crop, seed, call_index, crop_out: as
 *   ogbx_visual_gather; the drawn offsets are Philox words x, y of the counter
 *   {sample_lo, call_lo, OGBX_VISUAL_CROP_SLOT, sample_hi ^ call_hi} under the
 *   sampler's key (the GC or HGC stream tag), so no existing stream moves.
 * Every flat index is clamped into [0, L * N), every derived selector into
 * its sample's env and every stack row to the live steps, so every physical
 * row lies below T * N whatever the tables and the injected indices hold.
 * Returns OGBX_EINVAL (message in ogbx_last_error()) before any device work
 * for a NULL ring / table / cols / indices / column pointer, a ring outside
 * its ranges, steps < 1, total <= 0, num_cols outside
 * 1..OGBX_VISUAL_MAX_COLS, frame_stack outside 1..OGBX_VISUAL_MAX_STACK,
 * padding < 0, a selector outside its set or through a missing index output,
 * a non-positive geometry, crop_out without crop offsets, or a pointer that
 * is not device memory of the current device. */
ogbx_status ogbx_online_visual_gather(const ogbx_online_ring* ring, const ogbx_hgc_config* hcfg,
                                      const ogbx_online_visual_column* cols, int32_t num_cols, int64_t total,
                                      const ogbx_visual_indices* indices, int32_t frame_stack, int32_t padding,
                                      const int64_t* crop_from, int32_t draw_crop, uint64_t seed,
                                      uint64_t call_index, int64_t* crop_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_ONLINE_VISUAL_H_ */
