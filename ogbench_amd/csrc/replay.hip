// replay.hip -- the on-device replay buffer on gfx950 (include/ogbx_replay.h):
// batched ring inserts of what a vectorized env's step returned, and uniform
// sampling over the rows held so far.
//
// Reference (hliuson/ogbench):
//   ReplayBuffer                impls/utils/datasets.py:86-146
//   Dataset.sample / get_subset impls/utils/datasets.py:65-83
//   the SAC transition layout   data_gen_scripts/main_sac.py:115-123
//
// replay_insert_kernel: one workgroup per tile of up to kInsRows rows, all columns.
// A row's slot is (pointer + its rank among the kept rows) % max_size; with a
// keep mask a workgroup's first rank is the number of kept rows before its
// tile, which it sums itself from the mask bytes (at most 64 KB at N = 65,536,
// from L2), so ranks are deterministic and in row order.  Workgroup 0 also
// sums the whole mask and writes the new (pointer, size) to the header copy of
// the other parity: nobody reads that copy during the launch.
//
// replay_sample_kernel: gc_sample_kernel's tile structure (gc_device.h) with
// one Philox call per sample and two selectors, idx and next; size comes from
// the header.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ogbx_replay.h"
#include "common.h"
#include "gc_device.h"
#include "visual_tile.h"

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

template <int N>
struct InsArgs {
  const int64_t* hdr_in;
  int64_t* hdr_out;
  int64_t max_size, n;
  int32_t tile;  // rows per workgroup, <= kInsRows
  const uint8_t* keep;
  const uint8_t* sel;
  int32_t num_cols;
  ogbx_replay_insert_column c[N];
};

// Nonzero bytes of m[0, len), summed by the whole workgroup (every thread
// calls it and gets the sum).  16-byte loads between the aligned ends.
__device__ inline int64_t count_nonzero(const uint8_t* __restrict__ m, int64_t len, int64_t* red) {
  const int t = threadIdx.x;
  int64_t head = (int64_t)((16 - ((uintptr_t)m & 15)) & 15);
  head = head < len ? head : len;
  int64_t c = 0;
  if (t < head) c += m[t] != 0;
  const uint4* __restrict__ w = reinterpret_cast<const uint4*>(m + head);
  const int64_t nw = (len - head) >> 4;
  auto bytes_set = [](uint32_t v) {
    v |= v >> 4;
    v |= v >> 2;
    v |= v >> 1;
    return __popc(v & 0x01010101u);
  };
  for (int64_t i = t; i < nw; i += kInsThreads) {
    const uint4 v = w[i];
    c += bytes_set(v.x) + bytes_set(v.y) + bytes_set(v.z) + bytes_set(v.w);
  }
  const int64_t tail = head + (nw << 4);
  if (t < 16 && tail + t < len) c += m[tail + t] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  __syncthreads();  // red may still be read by an earlier call
  if ((t & 63) == 0) red[t >> 6] = c;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

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

template <bool kKeep, int N, bool kNt>
__global__ void __launch_bounds__(kInsThreads) replay_insert_kernel(InsArgs<N> a) {
  __shared__ int64_t slot[kInsRows];
  __shared__ int64_t red[4];
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * a.tile;
  const int n_here = (int)((a.n - base) < a.tile ? (a.n - base) : a.tile);
  const int64_t max_size = a.max_size;
  int64_t p = a.hdr_in[0];
  const int64_t size = a.hdr_in[1];
  // the caller keeps pointer < max_size; whatever the header holds, no slot leaves the buffer
  if ((uint64_t)p >= (uint64_t)max_size) p = 0;
  auto wrap = [max_size](int64_t s) { return s >= max_size ? s - max_size : s; };  // s < 2 max_size

  int64_t kept_total = a.n;
  if constexpr (kKeep) {
    // kept rows before this tile; workgroup 0 (none before it) sums the whole mask for the header
    const int64_t cnt = count_nonzero(a.keep, blockIdx.x == 0 ? a.n : base, red);
    const int64_t before = blockIdx.x == 0 ? 0 : cnt;
    kept_total = cnt;
    const bool kept = t < n_here && a.keep[base + t] != 0;
    const uint64_t bal = __ballot(kept);
    const int lane = t & 63, wave = t >> 6;
    const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    slot[t] = kept ? wrap(p + before + off + prefix) : -1;
    __syncthreads();
  }
  if (blockIdx.x == 0 && t == 0) {
    // size' = max(size, the largest pointer value the sequential adds visit):
    // the reference takes size = max(pointer, size) after the modulo
    const int64_t end = p + kept_total;  // <= 2 max_size - 1
    const int64_t top = end < max_size ? end : (p < max_size - 1 ? max_size - 1 : kept_total - 1);
    a.hdr_out[0] = end >= max_size ? end - max_size : end;
    a.hdr_out[1] = (size > top || kept_total == 0) ? size : top;  // no row kept: unchanged
  }
  auto slot_of = [&](int b) -> int64_t {
    if constexpr (kKeep) return slot[b];
    else return wrap(p + base + b);
  };

  for (int c = 0; c < a.num_cols; ++c) {
    const ogbx_replay_insert_column& col = a.c[c];
    if (moves_raw(col)) {
      const int64_t rb = col.row_elems * dtype_bytes(col.dst_dtype);
      const uintptr_t align = (uintptr_t)col.src | (uintptr_t)col.dst | (uintptr_t)col.alt;
      if (rb % 16 == 0 && align % 16 == 0) move_rows<kNt, u32v4>(col, a.sel, base, n_here, rb / 16, slot_of);
      else if (rb % 8 == 0 && align % 8 == 0) move_rows<kNt, u32v2>(col, a.sel, base, n_here, rb / 8, slot_of);
      else if (rb % 4 == 0 && align % 4 == 0) move_rows<kNt, uint32_t>(col, a.sel, base, n_here, rb / 4, slot_of);
      else move_rows<kNt, uint8_t>(col, a.sel, base, n_here, rb, slot_of);
    } else {
      switch (col.dst_dtype) {
        case OGBX_REPLAY_U8: cast_rows<kNt, uint8_t>(col, a.sel, base, n_here, slot_of); break;
        case OGBX_REPLAY_I32: cast_rows<kNt, int32_t>(col, a.sel, base, n_here, slot_of); break;
        case OGBX_REPLAY_I64: cast_rows<kNt, int64_t>(col, a.sel, base, n_here, slot_of); break;
        case OGBX_REPLAY_F32: cast_rows<kNt, float>(col, a.sel, base, n_here, slot_of); break;
        default: cast_rows<kNt, double>(col, a.sel, base, n_here, slot_of); break;
      }
    }
  }
}

// Dataset.sample / get_subset over rows [0, size) (datasets.py:65-83).
__global__ void __launch_bounds__(256) replay_sample_kernel(
    const int64_t* __restrict__ hdr, int64_t max_size, GcColumnsSmall cols, int32_t num_cols, int64_t total, int tile,
    const int64_t* __restrict__ idxs, uint32_t k0, uint32_t k1, uint32_t call_lo, uint32_t call_hi,
    int64_t* idxs_out, int64_t* empty_count, bool flat4) {
  __shared__ int64_t sel[2][kGcMaxTile];
  const int64_t tile_id = xcd_tile();
  const int64_t base = tile_id * tile;
  const int n_here = (int)((total - base) < tile ? (total - base) : tile);
  // the whole first wave runs the draw (lane b % n_here; lanes b < n_here
  // store): see gc_sample_kernel
  if (threadIdx.x < 64 && n_here > 0) {
    const int b = (int)threadIdx.x % n_here;
    const int64_t s = base + b;
    const uint64_t su = (uint64_t)s;
    int64_t size = hdr[1];
    size = size < 0 ? 0 : (size > max_size ? max_size : size);
    int64_t idx;
    if (idxs) {
      idx = clamp_row(idxs[s], max_size);
    } else {
      const u32x4 w = philox4x32_10({(uint32_t)su, call_lo, 0u, (uint32_t)(su >> 32) ^ call_hi}, k0, k1);
      idx = (int64_t)bounded64(w.x, w.y, (uint64_t)size);  // size 0: row 0
    }
    int64_t next = idx + 1 < size - 1 ? idx + 1 : size - 1;  // np.minimum(idxs + 1, size - 1)
    next = next < 0 ? 0 : next;
    if ((int)threadIdx.x < n_here) {
      sel[0][b] = idx;
      sel[1][b] = next;
      if (idxs_out) idxs_out[s] = idx;
    }
    if (size == 0 && empty_count && tile_id == 0 && threadIdx.x == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(empty_count), (unsigned long long)total);
  }
  __syncthreads();
  copy_tile<0, false, GcColumnsSmall>(cols, num_cols, sel, base, n_here, flat4);
}

template <bool kKeep, int N>
static ogbx_status launch_insert(int64_t* header, int32_t parity, int64_t max_size,
                                 const ogbx_replay_insert_column* cols, int32_t num_cols, int64_t n,
                                 const uint8_t* keep, const uint8_t* alt_select, hipStream_t s) {
  InsArgs<N> a{};
  a.hdr_in = header + 2 * parity;
  a.hdr_out = header + 2 * (1 - parity);
  a.max_size = max_size;
  a.n = n;
  a.keep = keep;
  a.sel = alt_select;
  a.num_cols = num_cols;
  for (int i = 0; i < num_cols; ++i) a.c[i] = cols[i];
  // rows per workgroup: halved from kInsRows while the launch has fewer than
  // 1,024 workgroups (four per CU) and a workgroup still moves 16 KB or more.
  // Kernel trace, profiles/replay_insert_ab.txt: 512-B rows at N = 16,384 run
  // 23.7 us at 256 rows per workgroup (64 workgroups), 12.0 at 64, 10.4 at 16;
  // 56-B rows at N = 65,536 run 7.8 us at 256 and 8.4 at 64, so they stay at 256
  int64_t row_bytes = 0;
  for (int i = 0; i < num_cols; ++i) row_bytes += cols[i].row_elems * dtype_bytes(cols[i].dst_dtype);
  int tile = kInsRows;
  while (tile > kInsMinRows && n / tile < 1024 && tile * row_bytes >= 16384) tile >>= 1;
  a.tile = tile;
  const int64_t blocks = (n + tile - 1) / tile;
  hipLaunchKernelGGL((replay_insert_kernel<kKeep, N, kInsNt>), dim3((uint32_t)blocks),
                     dim3(kInsThreads), 0, s, a);
  OGBX_LAUNCHED("replay_insert_kernel");
  return OGBX_OK;
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_replay_api_version(void) { return OGBX_REPLAY_API_VERSION; }

ogbx_status ogbx_replay_insert(int64_t* header, int32_t parity, int64_t max_size,
                               const ogbx_replay_insert_column* cols, int32_t num_cols, int64_t n,
                               const uint8_t* keep, const uint8_t* alt_select, void* stream) {
  const std::string who = "ogbx_replay_insert: ";
  OGBX_CHECK(header && cols, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(parity == 0 || parity == 1, OGBX_EINVAL, who + "parity must be 0 or 1");
  OGBX_CHECK(max_size > 0 && n > 0, OGBX_EINVAL, who + "max_size and n must be > 0");
  OGBX_CHECK(n <= max_size, OGBX_EINVAL, who + "n exceeds max_size (two rows would race for one slot)");
  OGBX_CHECK(num_cols >= 1 && num_cols <= OGBX_REPLAY_MAX_COLS, OGBX_EINVAL, who + "1 to 16 columns");
  // (a launch this large keeps kInsRows rows per workgroup)
  OGBX_CHECK((n + kInsRows - 1) / kInsRows <= 0x7fffffffll, OGBX_EINVAL, who + "too many rows for one launch");
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
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = on_device(header, dev) && (!keep || on_device(keep, dev)) && (!alt_select || on_device(alt_select, dev));
  for (int i = 0; i < num_cols && ok; ++i)
    ok = on_device(cols[i].dst, dev) && on_device(cols[i].src, dev) && (!cols[i].alt || on_device(cols[i].alt, dev));
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  hipStream_t s = (hipStream_t)stream;
  // the kernel arguments grow the host's launch cost (gc_device.h kGcSmallCols): 8 columns hold the SAC layout
  if (num_cols <= 8)
    return keep ? launch_insert<true, 8>(header, parity, max_size, cols, num_cols, n, keep, alt_select, s)
                : launch_insert<false, 8>(header, parity, max_size, cols, num_cols, n, keep, alt_select, s);
  return keep ? launch_insert<true, 16>(header, parity, max_size, cols, num_cols, n, keep, alt_select, s)
              : launch_insert<false, 16>(header, parity, max_size, cols, num_cols, n, keep, alt_select, s);
}

ogbx_status ogbx_replay_clear(int64_t* header, void* stream) {
  const std::string who = "ogbx_replay_clear: ";
  OGBX_CHECK(header, OGBX_EINVAL, who + "null argument");
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  OGBX_CHECK(on_device(header, dev), OGBX_EINVAL, who + "every pointer must be device memory of the current device");
  OGBX_HIP(hipMemsetAsync(header, 0, OGBX_REPLAY_HEADER_WORDS * sizeof(int64_t), (hipStream_t)stream));
  return OGBX_OK;
}

ogbx_status ogbx_replay_sample(const int64_t* header, int32_t parity, int64_t max_size,
                               const ogbx_gc_column* cols, int32_t num_cols, int64_t total,
                               const int64_t* idxs, uint64_t seed, uint64_t call_index, int64_t* idxs_out,
                               int64_t* empty_count, void* stream) {
  const std::string who = "ogbx_replay_sample: ";
  OGBX_CHECK(header && cols, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(parity == 0 || parity == 1, OGBX_EINVAL, who + "parity must be 0 or 1");
  OGBX_CHECK(max_size > 0 && total > 0, OGBX_EINVAL, who + "max_size and total must be > 0");
  OGBX_CHECK(num_cols >= 1 && num_cols <= OGBX_REPLAY_MAX_COLS, OGBX_EINVAL, who + "1 to 16 columns");
  GcColumnsSmall cc{};
  bool flat4 = true;
  for (int i = 0; i < num_cols; ++i) {
    const ogbx_gc_column& c = cols[i];
    OGBX_CHECK(c.src && c.dst, OGBX_EINVAL, who + "null column pointer");
    OGBX_CHECK(c.row_bytes > 0 && (c.select == 0 || c.select == 1), OGBX_EINVAL, who + "bad column descriptor");
    OGBX_CHECK(c.src_stride == 0 || c.src_stride >= c.row_bytes, OGBX_EINVAL, who + "src_stride below row_bytes");
    cc.c[i] = c;
    // copy_tile's per-wave job copy: 4-byte granular, aligned rows of <= 128 words
    flat4 = flat4 && c.row_bytes % 4 == 0 && c.row_bytes <= 512 &&
            ((uintptr_t)c.src | (uintptr_t)c.dst | (uintptr_t)c.src_stride) % 4 == 0;
  }
  const int64_t tile = gc_tile(total);
  const int64_t blocks = (total + tile - 1) / tile;
  OGBX_CHECK(blocks <= 0x7fffffffll, OGBX_EINVAL, who + "too many samples for one launch");
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = on_device(header, dev) && (!idxs || on_device(idxs, dev)) && (!idxs_out || on_device(idxs_out, dev)) &&
            (!empty_count || on_device(empty_count, dev));
  for (int i = 0; i < num_cols && ok; ++i) ok = on_device(cols[i].src, dev) && on_device(cols[i].dst, dev);
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  uint32_t k0, k1;
  seed_key(seed, kTagGcSample, &k0, &k1);
  hipLaunchKernelGGL(replay_sample_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream,
                     header + 2 * parity, max_size, cc, num_cols, total, (int)tile, idxs, k0, k1,
                     (uint32_t)call_index, (uint32_t)(call_index >> 32), idxs_out, empty_count,
                     flat4 && tile <= 4);
  OGBX_LAUNCHED("replay_sample_kernel");
  return OGBX_OK;
}

}  // extern "C"
