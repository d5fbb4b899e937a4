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
// the header.  Its column table is checked by gc_device.h's
// check_gather_columns, as the ring samplers' are.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ogbx_replay.h"
#include "common.h"
#include "gc_device.h"
#include "replay_device.h"

namespace ogbx {

// The row moves and casts, the column dispatch and the tile rule: replay_device.h
// (online.hip builds its insert kernel from the same pieces).

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

  insert_columns<kNt>(a.c, a.num_cols, a.sel, base, n_here, slot_of);
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
  const int tile = insert_tile(cols, num_cols, n);  // rows per workgroup
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
  if (ogbx_status st = check_insert_columns(cols, num_cols, alt_select, who)) return st;
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = all_on_device(dev, {header, keep, alt_select});
  for (int i = 0; i < num_cols && ok; ++i) ok = all_on_device(dev, {cols[i].dst, cols[i].src, cols[i].alt});
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
  bool flat4;
  GC_TRY(check_gather_columns<true>(cols, num_cols, 0b11u, "ogbx_replay_sample", &cc, &flat4));  // idx, next
  int64_t tile, blocks;
  OGBX_CHECK(sample_grid(total, &tile, &blocks), OGBX_EINVAL, who + "too many samples for one launch");
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = all_on_device(dev, {header, idxs, idxs_out, empty_count});
  for (int i = 0; i < num_cols && ok; ++i) ok = all_on_device(dev, {cols[i].src, cols[i].dst});
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
