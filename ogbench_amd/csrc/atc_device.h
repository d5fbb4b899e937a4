// atc_device.h -- what the ATC sample kernels over a dataset (atc.hip) and over
// the episode ring (online_atc.hip) share around their own anchor select: the
// workgroup's (sample, side) on the device; the argument checks, the launch
// shape and the argument fill of ogbx_atc_sample / ogbx_online_atc_sample on
// the host.  Internal to libogbx.
#pragma once

#include "../../include/ogbx_atc.h"
#include "common.h"
#include "visual_tile.h"

namespace ogbx {

// Workgroup b -> sample s and side (0 anchor, 1 positive).  Consecutive
// workgroup ids go round-robin to the 8 XCDs: the anchor and the positive
// workgroup of a sample run on one XCD, so the frames they share (F - k of F
// when k < F) are read from HBM once into that XCD's L2.
__device__ __forceinline__ int64_t atc_sample_of_block(int64_t b, int* side) {
  const int64_t x = b & 7, i = b >> 3;
  const int64_t grp = i >> 1;
  *side = (int)(i & 1);
  return grp * 8 + x;
}

// ---------------------------------------------------------------- host side
// What both entry points take besides their source and tables.
struct AtcCall {
  const ogbx_atc_column* col;
  int64_t total, k;
  int32_t frame_stack, padding;
  const int64_t *idxs, *pick, *crop_from;
  int32_t draw_crop;
  uint64_t seed, call_index;
  ogbx_atc_outputs out;  // all NULL when the caller passed none
};

// The argument checks the two entry points share, in their order.
static ogbx_status check_atc_call(const std::string& who, const AtcCall& c) {
  const ogbx_atc_column* col = c.col;
  OGBX_CHECK(col->src && col->anchor && col->positive, OGBX_EINVAL, who + "null column pointer");
  OGBX_CHECK(col->height > 0 && col->width > 0 && col->px_bytes > 0, OGBX_EINVAL, who + "bad image shape");
  OGBX_CHECK(c.total > 0, OGBX_EINVAL, who + "total must be > 0");
  OGBX_CHECK(c.k >= 0, OGBX_EINVAL, who + "k must be >= 0");
  OGBX_CHECK(c.frame_stack >= 1 && c.frame_stack <= OGBX_VISUAL_MAX_STACK, OGBX_EINVAL,
             who + "frame_stack must be in 1..8");
  OGBX_CHECK(c.padding >= 0 && c.padding < (1 << 20), OGBX_EINVAL, who + "padding must be >= 0");
  OGBX_CHECK(!c.out.crop_from || c.crop_from || c.draw_crop, OGBX_EINVAL,
             who + "crop_from output without crop offsets");
  return OGBX_OK;
}

// The launch's dynamic LDS and its grid, one workgroup per (sample, side).
static ogbx_status atc_launch_shape(const std::string& who, const AtcCall& c, uint32_t* lds_bytes, int64_t* blocks) {
  const int64_t F = c.frame_stack;
  const int64_t row_bytes = (int64_t)c.col->width * c.col->px_bytes, frame = row_bytes * c.col->height;
  OGBX_CHECK(frame * F <= (1ll << 30), OGBX_EINVAL, who + "image too large");
  *lds_bytes = std::max<uint32_t>(16u, vis_lds_bytes(frame, F));
  // at least one image row per staged frame
  OGBX_CHECK((int64_t)((*lds_bytes / (uint32_t)F) & ~15u) >= row_bytes, OGBX_EINVAL,
             who + "image row too wide to stage");
  *blocks = ((c.total + 7) / 8) * 8 * 2;
  OGBX_CHECK(*blocks <= 0x7fffffffll, OGBX_EINVAL, who + "too many (sample, side) pairs for one launch");
  return OGBX_OK;
}

// The fields AtcArgs and OnlineAtcArgs have in common, by name.
template <class Args>
static void fill_atc_args(Args& a, const AtcCall& c, uint32_t lds_bytes) {
  a.k = c.k;
  a.idxs = c.idxs;
  a.pick = c.pick;
  a.crop_from = c.crop_from;
  a.out = c.out;
  a.col = *c.col;
  a.frame_stack = c.frame_stack;
  a.padding = c.padding;
  a.draw = c.draw_crop != 0 && !c.crop_from;
  seed_key(c.seed, kTagAtcSample, &a.k0, &a.k1);
  a.call_lo = (uint32_t)c.call_index;
  a.call_hi = (uint32_t)(c.call_index >> 32);
  a.lds_bytes = lds_bytes;
  a.total = c.total;
}

}  // namespace ogbx
