// replay_device.h -- what the insert kernels of replay.hip (the SAC ring) and
// online.hip (the episode ring) share: the row moves and casts of one tile of
// offered rows, the column dispatch, and the host-side column checks and tile
// rule of the ogbx_replay_insert / ogbx_online_insert entry points.  Internal
// to libogbx.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ogbx_replay.h"
#include "common.h"

namespace ogbx {

constexpr int kInsRows = 256;     // most rows per workgroup
constexpr int kInsThreads = 256;  // one row per thread in the rank pass
constexpr int kInsMinRows = 16;
constexpr int64_t kInsMaxRowBytes = 1 << 22;  // tile-local item indices stay 32-bit
// Non-temporal stores: nothing in the launch reads the rows back.  A/B on the
// kernel trace (profiles/replay_insert_ab.txt): 10.39 -> 9.72 us at the antmaze
// share (8.4 MB written), 8.42 -> 8.45 us at the pointmaze share.
constexpr bool kInsNt = true;
typedef uint32_t u32v4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32v2 __attribute__((ext_vector_type(2)));

// Element e of a source of type sdt as D, converted as a NumPy assignment
// converts it: integers go through int64 straight to D (one rounding into a
// float), floats through double (float32 -> double is exact; double -> float32
// rounds to nearest even, double -> integer truncates).
template <typename D>
__device__ __forceinline__ D load_as(const void* __restrict__ p, int sdt, int64_t e) {
  switch (sdt) {
    case OGBX_REPLAY_BOOL: return (D)(int64_t)(static_cast<const uint8_t*>(p)[e] != 0);
    case OGBX_REPLAY_U8: return (D)(int64_t) static_cast<const uint8_t*>(p)[e];
    case OGBX_REPLAY_I32: return (D)(int64_t) static_cast<const int32_t*>(p)[e];
    case OGBX_REPLAY_I64: return (D) static_cast<const int64_t*>(p)[e];
    case OGBX_REPLAY_F32: return (D)(double)static_cast<const float*>(p)[e];
    default: return (D) static_cast<const double*>(p)[e];
  }
}

// The rows of one column of this tile, `units` items of T (or D) per row;
// item f of the tile is (row f / units, item f % units), advanced without a
// division per item.  slot_of(b): the destination row, or -1 (not kept).
template <bool kNt, typename T>
__device__ __forceinline__ void put(T* p, T v) {
  if constexpr (kNt) __builtin_nontemporal_store(v, p);
  else *p = v;
}

template <bool kNt, typename T, class SlotOf>
__device__ inline void move_rows(const ogbx_replay_insert_column& col, const uint8_t* __restrict__ sel, int64_t base,
                                 int n_here, int64_t units, SlotOf slot_of) {
  const T* __restrict__ src = static_cast<const T*>(col.src);
  const T* __restrict__ alt = static_cast<const T*>(col.alt);
  T* __restrict__ dst = static_cast<T*>(col.dst);
  const uint32_t u = (uint32_t)units, total = u * (uint32_t)n_here;  // < 2^30 (kInsMaxRowBytes)
  const uint32_t tid = threadIdx.x;
  uint32_t b = tid / u, k = tid % u;
  const uint32_t sb = kInsThreads / u, sk = kInsThreads % u;
  for (uint32_t f = tid; f < total; f += kInsThreads) {
    const int64_t s = slot_of((int)b);
    if (s >= 0) {
      const int64_t row = base + b;
      const T* from = (alt && sel[row]) ? alt : src;
      put<kNt>(dst + s * units + k, from[row * units + k]);
    }
    k += sk;
    b += sb;
    if (k >= u) {
      k -= u;
      b += 1;
    }
  }
}

template <bool kNt, typename D, class SlotOf>
__device__ inline void cast_rows(const ogbx_replay_insert_column& col, const uint8_t* __restrict__ sel, int64_t base,
                                 int n_here, SlotOf slot_of) {
  const int64_t units = col.row_elems;
  D* __restrict__ dst = static_cast<D*>(col.dst);
  const int sdt = col.src_dtype;
  const bool one_minus = col.op == OGBX_REPLAY_OP_ONE_MINUS;
  const uint32_t u = (uint32_t)units, total = u * (uint32_t)n_here;  // < 2^30 (kInsMaxRowBytes)
  const uint32_t tid = threadIdx.x;
  uint32_t b = tid / u, k = tid % u;
  const uint32_t sb = kInsThreads / u, sk = kInsThreads % u;
  for (uint32_t f = tid; f < total; f += kInsThreads) {
    const int64_t s = slot_of((int)b);
    if (s >= 0) {
      const int64_t row = base + b;
      const void* from = (col.alt && sel[row]) ? col.alt : col.src;
      const D v = load_as<D>(from, sdt, row * units + k);
      put<kNt>(dst + s * units + k, one_minus ? (D)((D)1 - v) : v);
    }
    k += sk;
    b += sb;
    if (k >= u) {
      k -= u;
      b += 1;
    }
  }
}

__host__ __device__ inline int dtype_bytes(int dt) {
  switch (dt) {
    case OGBX_REPLAY_BOOL:
    case OGBX_REPLAY_U8: return 1;
    case OGBX_REPLAY_I32:
    case OGBX_REPLAY_F32: return 4;
    default: return 8;
  }
}

// Rows move as bytes: equal types (BOOL -> U8: torch's bool bytes are 0 / 1) and no op.
__host__ __device__ inline bool moves_raw(const ogbx_replay_insert_column& c) {
  const bool same = c.src_dtype == c.dst_dtype || (c.src_dtype == OGBX_REPLAY_BOOL && c.dst_dtype == OGBX_REPLAY_U8);
  return same && c.op == OGBX_REPLAY_OP_NONE;
}

// Every column of this tile: rows [base, base + n_here) of the sources to the
// rows slot_of names.
template <bool kNt, class SlotOf>
__device__ __forceinline__ void insert_columns(const ogbx_replay_insert_column* cols, int num_cols,
                                               const uint8_t* __restrict__ sel, int64_t base, int n_here,
                                               SlotOf slot_of) {
  for (int c = 0; c < num_cols; ++c) {
    const ogbx_replay_insert_column& col = cols[c];
    if (moves_raw(col)) {
      const int64_t rb = col.row_elems * dtype_bytes(col.dst_dtype);
      const uintptr_t align = (uintptr_t)col.src | (uintptr_t)col.dst | (uintptr_t)col.alt;
      if (rb % 16 == 0 && align % 16 == 0) move_rows<kNt, u32v4>(col, sel, base, n_here, rb / 16, slot_of);
      else if (rb % 8 == 0 && align % 8 == 0) move_rows<kNt, u32v2>(col, sel, base, n_here, rb / 8, slot_of);
      else if (rb % 4 == 0 && align % 4 == 0) move_rows<kNt, uint32_t>(col, sel, base, n_here, rb / 4, slot_of);
      else move_rows<kNt, uint8_t>(col, sel, base, n_here, rb, slot_of);
    } else {
      switch (col.dst_dtype) {
        case OGBX_REPLAY_U8: cast_rows<kNt, uint8_t>(col, sel, base, n_here, slot_of); break;
        case OGBX_REPLAY_I32: cast_rows<kNt, int32_t>(col, sel, base, n_here, slot_of); break;
        case OGBX_REPLAY_I64: cast_rows<kNt, int64_t>(col, sel, base, n_here, slot_of); break;
        case OGBX_REPLAY_F32: cast_rows<kNt, float>(col, sel, base, n_here, slot_of); break;
        default: cast_rows<kNt, double>(col, sel, base, n_here, slot_of); break;
      }
    }
  }
}

// ---------------------------------------------------------------- host side
// The column descriptors of an insert; `who` ends in ": ".
static ogbx_status check_insert_columns(const ogbx_replay_insert_column* cols, int32_t num_cols,
                                        const uint8_t* alt_select, const std::string& who) {
  for (int i = 0; i < num_cols; ++i) {
    const ogbx_replay_insert_column& c = cols[i];
    OGBX_CHECK(c.dst && c.src, OGBX_EINVAL, who + "null column pointer");
    OGBX_CHECK(c.row_elems > 0, OGBX_EINVAL, who + "row_elems must be > 0");
    OGBX_CHECK(c.row_elems <= kInsMaxRowBytes / 8, OGBX_EINVAL, who + "a row of more than 4 MiB");
    OGBX_CHECK(c.src_dtype >= OGBX_REPLAY_BOOL && c.src_dtype <= OGBX_REPLAY_F64, OGBX_EINVAL,
               who + "unknown source dtype");
    OGBX_CHECK(c.dst_dtype >= OGBX_REPLAY_U8 && c.dst_dtype <= OGBX_REPLAY_F64, OGBX_EINVAL,
               who + "unknown destination dtype");
    OGBX_CHECK(c.op == OGBX_REPLAY_OP_NONE || c.op == OGBX_REPLAY_OP_ONE_MINUS, OGBX_EINVAL, who + "unknown op");
    OGBX_CHECK(!c.alt || alt_select, OGBX_EINVAL, who + "a column has alt but the call has no alt_select");
  }
  return OGBX_OK;
}

// Rows per workgroup: halved from kInsRows while the launch has fewer than
// 1,024 workgroups (four per CU) and a workgroup still moves 16 KB or more.
// Kernel trace, profiles/replay_insert_ab.txt: 512-B rows at N = 16,384 run
// 23.7 us at 256 rows per workgroup (64 workgroups), 12.0 at 64, 10.4 at 16;
// 56-B rows at N = 65,536 run 7.8 us at 256 and 8.4 at 64, so they stay at 256
static int insert_tile(const ogbx_replay_insert_column* cols, int32_t num_cols, int64_t n) {
  int64_t row_bytes = 0;
  for (int i = 0; i < num_cols; ++i) row_bytes += cols[i].row_elems * dtype_bytes(cols[i].dst_dtype);
  int tile = kInsRows;
  while (tile > kInsMinRows && n / tile < 1024 && tile * row_bytes >= 16384) tile >>= 1;
  return tile;
}

}  // namespace ogbx
