/* ogbx_atc.h -- ATC batches: anchor / positive observation pairs (o_t, o_{t+k})
 * of one trajectory, frame stacked and randomly cropped, for the pretraining
 * of visual encoders (hliuson/ogbench impls/utils/datasets.py:369-464; consumed
 * by impls/pretrain_atc.py:167-251).
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_atc_api_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h; OGBX_VISUAL_MAX_STACK and OGBX_VISUAL_CROP_SLOT are ogbx_visual.h's.
 *
 * Scope: the direct path only, one batch per call; there is no look-ahead /
 * sampler-plan form.
 */
#ifndef OGBX_ATC_H_
#define OGBX_ATC_H_

#include "ogbx.h"
#include "ogbx_visual.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_ATC_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_atc_api_version(void);

/* valid(k), the anchor table of temporal offset k (get_valid_atc_idxs,
 * datasets.py:417-436): the candidates c, in order, with
 *   c + k <= traj_end[c]
 * (the reference's first filter c + k < num_rows is implied).  The candidates
 * are buf->valid_idxs (buf->num_valid of them), or the rows 0..num_rows-1 when
 * that is NULL.  Only num_rows, valid_idxs, num_valid, traj_end and the three
 * period fields of the ogbx_gc_buffer are read by this header.
 *
 * Philox words.  The key is (lo32(seed), hi32(seed) ^ 0x41540001), a stream
 * tag of ATC's own; the counter is {sample_lo, call_lo, slot, sample_hi ^
 * call_hi} as everywhere.
 *   pick      slot 0, words x, y:  mulhi64((x << 32) | y, size of valid(k)),
 *             a position into valid(k)  (np.random.choice(valid(k), size=B))
 *   crop_from slot OGBX_VISUAL_CROP_SLOT, words x, y, each reduced to
 *             [0, 2 padding] by mulhi32(word, 2 padding + 1): (cy, cx)
 *             (np.random.randint(0, 2 padding + 1, (B, 2)))
 * No existing tag or slot moves. */

/* The observations and the two outputs.  src holds UNSTACKED frames, dense
 * [R, height, width, px_bytes]; a non-image row is a 1-row image (height 1,
 * width = its leading elements, px_bytes = bytes of its last axis).  anchor and
 * positive are dense [total, height, width, F * px_bytes], F = frame_stack:
 * channel block j (0..F-1) of row r is the frame at row
 * max(r - (F-1-j), first row of r's trajectory); anchor is built at r = idx,
 * positive at r = idx + k. */
typedef struct {
  const void* src;
  void* anchor;
  void* positive;
  int32_t height, width;
  int32_t px_bytes; /* bytes of one pixel of ONE frame (channels * itemsize) */
  int32_t crop;     /* 1: apply the sample's crop offsets (4-D observations);
                       0: never cropped                                       */
} ogbx_atc_column;

/* Optional per-call outputs; every pointer may be NULL. */
typedef struct {
  int64_t* idxs;      /* [total] the anchor rows used                         */
  int64_t* pick;      /* [total] the positions into valid(k); -1 with explicit
                         idxs                                                 */
  int64_t* crop_from; /* [total, 2] the offsets (only with crop_from or
                         draw_crop)                                           */
  /* One int64, zeroed by the caller.  The kernel adds the number of samples
   * whose idx lies outside [0, num_rows) or whose idx + k passes
   * traj_end[idx]: possible only with explicit idxs.  Such a sample's rows
   * are clamped into the buffer, so nothing is read out of bounds. */
  int64_t* bad_count;
} ogbx_atc_outputs;

/* The ordered select valid(k) to out (device int64, room for every candidate)
 * and its size to *count (device int64).  k < 0 is OGBX_EINVAL. */
ogbx_status ogbx_atc_valid_idxs(const ogbx_gc_buffer* buf, int64_t k, int64_t* out, int64_t* count,
                                void* stream);

/* ATCDataset.sample (datasets.py:401-415) in ONE launch: one workgroup per
 * (sample, side), side = anchor or positive; the two workgroups of a sample
 * run on one XCD (for k < F they share frames).
 *
 * The anchor row of sample s, in this order of precedence:
 *   idxs[s]            when idxs is non-NULL (device int64 [total]);
 *   else row(pick[s])  when pick is non-NULL (device int64 [total], positions
 *                      into valid(k), clamped into it);
 *   else row(the Philox pick).
 * row(p) = valid[p] when `valid` (device int64 [num_valid], the output of
 *   ogbx_atc_valid_idxs for this k) is non-NULL.  With valid NULL and
 *   buf->period > 0 (candidates at offsets 0..period_picks-1 of every period,
 *   their trajectory ending at offset period_end), the closed form
 *     m = min(period_picks, period_end - k + 1)      picks per period
 *     size of valid(k) = (num_rows / period) * m
 *     row(p) = (p / m) * period + p % m
 *   and num_valid is ignored.  valid NULL, period 0 and idxs NULL is
 *   OGBX_EINVAL, as is an empty valid(k) without explicit idxs.
 * frame_stack: F in 1..OGBX_VISUAL_MAX_STACK.  padding >= 0, crop_from (device
 *   int64 [total, 2]), draw_crop: the crop as ogbx_visual_gather defines it,
 *   drawn under the ATC key (above); one (cy, cx) per sample for both sides.
 * Returns OGBX_EINVAL (message in ogbx_last_error()) before any device work
 * for a NULL buf / col / column pointer, non-positive sizes, k < 0, an image
 * too large or too wide to stage, or a pointer that is not device memory of
 * the current device. */
ogbx_status ogbx_atc_sample(const ogbx_gc_buffer* buf, const ogbx_atc_column* col, int64_t total, int64_t k,
                            const int64_t* valid, int64_t num_valid, int32_t frame_stack, int32_t padding,
                            const int64_t* idxs, const int64_t* pick, const int64_t* crop_from,
                            int32_t draw_crop, uint64_t seed, uint64_t call_index,
                            const ogbx_atc_outputs* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_ATC_H_ */
