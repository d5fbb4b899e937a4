// visual_tile.h -- what the image kernels of visual.hip, atc.hip and
// online_visual.hip share: one workgroup stages the F source frames of one
// selector row (or a band of their rows when they exceed the LDS budget) in
// LDS with the widest aligned loads and composes one output image -- pixels of
// F * px_bytes bytes, shifted by the crop -- from LDS in 16-byte units aligned
// to the destination.  compose_frames takes the address of each block's frame,
// so the unrelated physical rows of the episode ring compose with the code of
// the offline datasets' consecutive rows (compose_image).  The two gathers
// over (sample, column) pairs (visual.hip, online_visual.hip) also take their
// host path from here.  Internal to
// libogbx.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/ogbx_visual.h"
#include "common.h"
#include "gc_select.h"

namespace ogbx {

constexpr int kVisThreads = 256;
constexpr uint32_t kVisLdsMax = 64u * 1024u;  // dynamic LDS without an attribute call

// Geometry of one image column: the source holds UNSTACKED frames, dense
// [R, height, width, px_bytes].
struct VisGeom {
  const void* src;
  int32_t height, width;
  int32_t px_bytes;  // bytes of one pixel of ONE frame
};

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Global -> LDS (or global) copy of len bytes by the whole workgroup: 16-byte
// units when both sides allow it, else 4-byte units, the remainder in bytes.
__device__ inline void copy_bytes(uint8_t* __restrict__ d, const uint8_t* __restrict__ g, int64_t len) {
  const int t = threadIdx.x;
  const uintptr_t a = (uintptr_t)g | (uintptr_t)d;
  int64_t done = 0;
  if ((a & 15) == 0) {
    const int64_t n = len >> 4;
    for (int64_t i = t; i < n; i += kVisThreads)
      reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(g)[i];
    done = n << 4;
  } else if ((a & 3) == 0) {
    const int64_t n = len >> 2;
    for (int64_t i = t; i < n; i += kVisThreads)
      reinterpret_cast<uint32_t*>(d)[i] = reinterpret_cast<const uint32_t*>(g)[i];
    done = n << 2;
  }
  for (int64_t i = done + t; i < len; i += kVisThreads) d[i] = g[i];
}

// First row of r's trajectory among the F - 1 rows before r (r inside the
// buffer): row r-s belongs to r's trajectory iff r-s >= 0 and
// traj_end[r-s] == traj_end[r].
__device__ __forceinline__ int64_t stack_start(const int64_t* __restrict__ traj_end, int64_t r, int F) {
  int64_t start = r;
  if (F > 1) {
    const int64_t te = traj_end[r];
    for (int k = 1; k < F; ++k) {
      const int64_t cand = r - k;
      if (cand < 0 || traj_end[cand] != te) break;
      start = cand;
    }
  }
  return start;
}

// One output image by the whole workgroup of kVisThreads threads, from F
// source frames that may lie anywhere: frame_at(j) is the address of the
// dense [H, W, px] frame of channel block j (0..F-1); the window starts at
// (cy, cx) of the image padded by p edge pixels ((p, p) is the identity).
// lds: lds_bytes of 16-byte aligned LDS with at least one image row per staged
// frame ((lds_bytes / F) & ~15 >= W * px); dst: the dense [H, W, F * px]
// destination.
template <class FrameAt>
__device__ __forceinline__ void compose_frames(uint8_t* lds, uint32_t lds_bytes, int H, int W, int px, int F, int cy,
                                               int cx, int p, uint8_t* __restrict__ dst, FrameAt frame_at) {
  const int t = threadIdx.x;
  const int rb = W * px;               // source row bytes
  const int64_t fb = (int64_t)H * rb;  // source frame bytes
  const int opx = F * px;              // output pixel bytes
  const int orb = W * opx;             // output row bytes

  if (F == 1 && cy == p && cx == p) {  // a row copy
    copy_bytes(dst, frame_at(0), fb);
    return;
  }

  const int fstride = (int)((lds_bytes / (uint32_t)F) & ~15u);  // LDS bytes per staged frame
  const int band = H < fstride / rb ? H : fstride / rb;         // output rows per pass (>= 1)
  for (int y0 = 0; y0 < H; y0 += band) {
    const int y1 = y0 + band < H ? y0 + band : H;
    const int sy_lo = clampi(y0 + cy - p, H - 1), sy_hi = clampi(y1 - 1 + cy - p, H - 1);
    const int len = (sy_hi - sy_lo + 1) * rb;  // <= band * rb <= fstride
    if (y0 > 0) __syncthreads();               // the previous band was composed
    for (int j = 0; j < F; ++j) copy_bytes(lds + j * fstride, frame_at(j) + (int64_t)sy_lo * rb, len);
    __syncthreads();

    // compose rows [y0, y1) in 16-byte units aligned to the destination; the
    // first and last unit may be partial (the neighbouring bytes belong to
    // another band or another sample) and are stored bytewise
    uint8_t* __restrict__ D = dst + (int64_t)y0 * orb;
    const int L = (y1 - y0) * orb;
    const int head = (int)((uintptr_t)D & 15);
    const int nunits = (head + L + 15) >> 4;
    for (int u = t; u < nunits; u += kVisThreads) {
      const int o0 = u * 16 - head;
      const int b0 = o0 < 0 ? -o0 : 0;
      const int b1 = L - o0 < 16 ? L - o0 : 16;
      const int o = o0 + b0;
      int yy = o / orb;
      const int rem = o - yy * orb;
      int xx = rem / opx;
      const int r2 = rem - xx * opx;
      int jj = r2 / px;
      int kk = r2 - jj * px;
      int pix = (clampi(y0 + yy + cy - p, H - 1) - sy_lo) * rb + clampi(xx + cx - p, W - 1) * px;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (q >= b0 && q < b1) {
          w[q >> 2] |= (uint32_t)lds[jj * fstride + pix + kk] << (8 * (q & 3));
          if (++kk == px) {
            kk = 0;
            if (++jj == F) {
              jj = 0;
              if (++xx == W) {
                xx = 0;
                ++yy;
              }
              pix = (clampi(y0 + yy + cy - p, H - 1) - sy_lo) * rb + clampi(xx + cx - p, W - 1) * px;
            }
          }
        }
      }
      if (b0 == 0 && b1 == 16) {
        *reinterpret_cast<uint4*>(D + o0) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (q >= b0 && q < b1) D[o0 + q] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
      }
    }
  }
}

// The output image of selector row r of a dense [R, height, width, px_bytes]
// source: channel block j (0..F-1) is the frame at row max(r - (F-1-j), start)
// with start = stack_start(traj_end, r, F).
__device__ __forceinline__ void compose_image(uint8_t* lds, uint32_t lds_bytes, const VisGeom& g, int64_t r,
                                              int64_t start, int F, int cy, int cx, int p,
                                              uint8_t* __restrict__ dst) {
  const int64_t fb = (int64_t)g.height * (g.width * g.px_bytes);  // source frame bytes
  const uint8_t* __restrict__ src = static_cast<const uint8_t*>(g.src);
  compose_frames(lds, lds_bytes, g.height, g.width, g.px_bytes, F, cy, cx, p, dst, [=](int j) {
    int64_t row = r - (F - 1 - j);
    row = row < start ? start : row;
    return src + row * fb;
  });
}

// The crop offsets (cy, cx) of sample s, each in [0, 2 p]: the injected pair
// moved into range (lax.dynamic_slice moves an out-of-range window start),
// else Philox words x, y of the counter {sample_lo, call_lo,
// OGBX_VISUAL_CROP_SLOT, sample_hi ^ call_hi} reduced by multiply-high
// (include/ogbx_visual.h).
__device__ __forceinline__ void crop_offsets(const int64_t* __restrict__ crop_from, int64_t s, int p, uint32_t k0,
                                             uint32_t k1, uint32_t call_lo, uint32_t call_hi, int64_t* oy,
                                             int64_t* ox) {
  if (crop_from) {
    const int64_t y = crop_from[2 * s], x = crop_from[2 * s + 1];
    *oy = y < 0 ? 0 : (y > 2 * p ? 2 * p : y);
    *ox = x < 0 ? 0 : (x > 2 * p ? 2 * p : x);
  } else {
    const uint64_t su = (uint64_t)s;
    const u32x4 w = philox4x32_10(
        {(uint32_t)su, call_lo, (uint32_t)OGBX_VISUAL_CROP_SLOT, (uint32_t)(su >> 32) ^ call_hi}, k0, k1);
    *oy = bounded_u32(w.x, (uint32_t)(2 * p + 1));
    *ox = bounded_u32(w.y, (uint32_t)(2 * p + 1));
  }
}

// ---------------------------------------------------------------- host side
// Dynamic LDS for images of `frame` bytes stacked F deep: all F frames padded
// to 16 bytes when they fit the budget, else the budget (the band loop).
static uint32_t vis_lds_bytes(int64_t frame, int64_t F) {
  const int64_t need = F * ((frame + 15) & ~15ll);
  return (uint32_t)(need < (int64_t)kVisLdsMax ? need : (int64_t)kVisLdsMax);
}

// What a gather call passes besides its buffer and columns.
struct VisualCall {
  const ogbx_visual_indices* indices;
  const ogbx_hgc_config* hcfg;
  int64_t total;
  int32_t num_cols, frame_stack, padding;
  const int64_t* crop_from;
  int32_t draw_crop;
  int64_t* crop_out;
  uint64_t seed, call_index;
};

// The argument checks the two gathers share, from indices->idxs on, in their
// order; copies the columns into the kernel argument table and gives the launch
// its dynamic LDS and grid.  min_cols, count_words: the entry point's column
// count and its wording; next_selector: select code 1 is allowed (not over the
// ring, which stores its own next_observations).
template <class Col, class Table>
static ogbx_status check_visual_gather(const std::string& who, const VisualCall& v, const Col* cols, int min_cols,
                                       const char* count_words, bool next_selector, Table* table, uint32_t* lds_bytes,
                                       int64_t* blocks) {
  const ogbx_hgc_config* hcfg = v.hcfg;
  const int32_t num_cols = v.num_cols, frame_stack = v.frame_stack;
  OGBX_CHECK(v.indices->idxs, OGBX_EINVAL, who + "indices->idxs is required");
  OGBX_CHECK(num_cols >= min_cols && num_cols <= OGBX_VISUAL_MAX_COLS, OGBX_EINVAL, who + count_words);
  OGBX_CHECK(v.total > 0, OGBX_EINVAL, who + "total must be > 0");
  OGBX_CHECK(frame_stack >= 1 && frame_stack <= OGBX_VISUAL_MAX_STACK, OGBX_EINVAL,
             who + "frame_stack must be in 1..8");
  OGBX_CHECK(v.padding >= 0 && v.padding < (1 << 20), OGBX_EINVAL, who + "padding must be >= 0");
  OGBX_CHECK(!v.crop_out || v.crop_from || v.draw_crop, OGBX_EINVAL, who + "crop_out without crop offsets");
  if (hcfg)
    OGBX_CHECK(hcfg->value_subgoal_steps >= 0 && hcfg->low_subgoal_steps >= 0 && hcfg->actor_subgoal_steps >= 0,
               OGBX_EINVAL, who + "negative subgoal steps");
  const int max_select = hcfg ? kHgcSel - 1 : 3;
  uint32_t lds = 16;
  for (int i = 0; i < num_cols; ++i) {
    const Col& c = cols[i];
    OGBX_CHECK(c.src && c.dst, OGBX_EINVAL, who + "null column pointer");
    OGBX_CHECK(c.height > 0 && c.width > 0 && c.px_bytes > 0, OGBX_EINVAL, who + "bad image shape");
    OGBX_CHECK(c.select >= 0 && c.select <= max_select && (next_selector || c.select != 1), OGBX_EINVAL,
               who + "selector out of range");
    const int s = c.select;
    const bool need_v = s == 2 || s == 4 || s == 5, need_a = s == 3 || s == 7 || s == 9, need_l = s == 6;
    OGBX_CHECK((!need_v || v.indices->value_goal_idxs) && (!need_a || v.indices->actor_goal_idxs) &&
                   (!need_l || v.indices->low_value_goal_idxs),
               OGBX_EINVAL, who + "a column selects through a missing index output");
    const int64_t F = c.stack ? frame_stack : 1;
    const int64_t row_bytes = (int64_t)c.width * c.px_bytes, frame = row_bytes * c.height;
    OGBX_CHECK(frame * F <= (1ll << 30), OGBX_EINVAL, who + "image too large");
    lds = std::max<uint32_t>(lds, vis_lds_bytes(frame, F));
    table->c[i] = c;
  }
  for (int i = 0; i < num_cols; ++i) {  // at least one image row per staged frame
    const uint32_t F = cols[i].stack ? (uint32_t)frame_stack : 1u;
    OGBX_CHECK((int64_t)((lds / F) & ~15u) >= (int64_t)cols[i].width * cols[i].px_bytes, OGBX_EINVAL,
               who + "image row too wide to stage");
  }
  *blocks = ((v.total + 7) / 8) * 8 * num_cols;
  OGBX_CHECK(*blocks <= 0x7fffffffll, OGBX_EINVAL, who + "too many (sample, column) pairs for one launch");
  *lds_bytes = lds;
  return OGBX_OK;
}

// The index outputs, the crop arrays and both ends of every column are device
// memory of `dev` (a column's alt, where its type has one, is the caller's).
template <class Col>
static bool visual_pointers_on_device(int dev, const VisualCall& v, const Col* cols) {
  bool ok = all_on_device(dev, {v.indices->idxs, v.indices->value_goal_idxs, v.indices->actor_goal_idxs,
                                v.indices->low_value_goal_idxs, v.crop_from, v.crop_out});
  for (int i = 0; i < v.num_cols && ok; ++i) ok = all_on_device(dev, {cols[i].src, cols[i].dst});
  return ok;
}

// The fields VisArgs and OnVisArgs have in common, by name.
template <class Args>
static void fill_visual_args(Args& a, const VisualCall& v, uint32_t lds_bytes) {
  a.idxs = v.indices->idxs;
  a.vg = v.indices->value_goal_idxs;
  a.ag = v.indices->actor_goal_idxs;
  a.lvg = v.indices->low_value_goal_idxs;
  if (v.hcfg) {
    a.k_value = v.hcfg->value_subgoal_steps;
    a.k_low = v.hcfg->low_subgoal_steps;
    a.k_actor = v.hcfg->actor_subgoal_steps;
  }
  a.frame_stack = v.frame_stack;
  a.padding = v.padding;
  a.draw = v.draw_crop != 0 && !v.crop_from;
  a.crop_from = v.crop_from;
  a.crop_out = v.crop_out;
  seed_key(v.seed, v.hcfg ? kTagHgcSample : kTagGcSample, &a.k0, &a.k1);
  a.call_lo = (uint32_t)v.call_index;
  a.call_hi = (uint32_t)(v.call_index >> 32);
  a.lds_bytes = lds_bytes;
  a.num_cols = v.num_cols;
  a.total = v.total;
}

}  // namespace ogbx
