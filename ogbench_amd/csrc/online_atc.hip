// online_atc.hip -- ATC batches over the on-device episode ring on gfx950
// (include/ogbx_online_atc.h): ATCDataset.sample(B, k) over the snapshot of the
// ring, whose anchor table valid(k) -- every live row whose offset + k stays
// inside its episode -- changes with every insert and is never built.
//
// Reference (hliuson/ogbench impls/utils/datasets.py):
//   ATCDataset.sample                   401-415
//   ATCDataset.get_valid_atc_idxs       417-436
//   ATCDataset.augment                  438-448
//   ATCDataset.get_stacked_observations 457-464
//
// ogbx_online_atc_table: online_atc_count_kernel, one wave per env, takes the
// env's c + 1 live segments 64 at a time -- the ep_end loads of a round are
// independent, their addresses follow from seq0 + i -- carries the running
// segment end and anchor count by wave scans, and writes W_i of each segment
// and the env's total A[e] (one lane per env walked 256 live segments in 74 us
// at N = 1,024: profiles/online_atc_sampler.json, earlier_forms); one device-wide
// exclusive scan (rocPRIM, its tile this file's to fix, as online_trl.hip)
// turns A into P.  An episode shorter than k + 1 holds no anchor, so A[e] is a
// sum over the segments and no closed form of two ordinals (as the TRL table).
//
// online_atc_sample_kernel keeps atc_sample_kernel's work layout (atc.hip):
// one workgroup per (sample, side), both sides of a sample on one XCD.  Each
// workgroup runs the select itself, on values uniform over the workgroup: a
// halving search over P for the env, the env's two ordinals, a binary search
// over W for the segment, one ep_end load for the segment's first offset;
// then stack_first at the side's offset (online_device.h) and compose_frames
// (visual_tile.h), the code online_visual_gather_kernel runs.  What the kernel
// and ogbx_online_atc_sample share with the dataset's is in atc_device.h.  The
// table and the sample are separate launches: P crosses workgroups and XCDs,
// and the kernel boundary is what makes it visible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/ogbx_online_atc.h"
#include "atc_device.h"
#include "common.h"
#include "gc_device.h"
#include "online_device.h"
#include "visual_tile.h"

namespace ogbx {

// ------------------------------------------------------------------ the table
constexpr int kCountThreads = 256;
constexpr int kCountWaves = kCountThreads / 64;  // envs per workgroup

// Inclusive scans over the 64 lanes of a wave (shuffles; every lane takes part).
__device__ __forceinline__ int64_t wave_scan_max(int64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(v, d, 64);
    if (lane >= d) v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int64_t wave_scan_sum(int64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// One wave per env e < N: lane l takes segments l, l + 64, ...; each round
// loads 64 ep_end entries at once and carries the running end and the running
// anchor count from round to round.  The serial rule end_i = max(E_i,
// end_{i-1} + 1) is a running maximum of E_i - i, so both carries are wave
// scans.  The wave of e = N writes A[N] = 0 (the scan's last output is the
// total).
__global__ void __launch_bounds__(kCountThreads) online_atc_count_kernel(OnlineView r, int64_t k,
                                                                         int32_t* __restrict__ W,
                                                                         int64_t* __restrict__ A) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * kCountWaves + ((int)threadIdx.x >> 6);  // uniform over the wave
  if (e > r.n) return;
  if (e == r.n) {
    if (lane == 0) A[e] = 0;
    return;
  }
  const int64_t L = r.live;
  const uint32_t T = (uint32_t)r.horizon;
  const uint32_t s0 = (uint32_t)r.ep_seq[phys_row(r, e, 0)], sn = (uint32_t)r.ep_seq[phys_row(r, e, L - 1)];
  const int64_t c = clamp_row((int64_t)(sn - s0), L);  // closed before the newest row, in [0, L - 1]
  int64_t top = INT64_MIN / 2;  // max of E_j - j over the rounds so far
  int64_t prev_end = -1;        // end of the last segment of the round before
  int64_t run = 0;              // anchors of the rounds so far
  for (int64_t i0 = 0; i0 <= c; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool live = i <= c;
    const int64_t slot = (int64_t)((s0 + (uint32_t)i) % T) * r.n + e;  // below T * N whatever i is
    int64_t E = L - 1;  // segment c ends at the newest row
    if (i < c) E = r.ep_end[slot] - r.first;
    E = E < 0 ? 0 : (E > L - 1 ? L - 1 : E);  // whatever the table holds
    int64_t m = wave_scan_max(live ? E - i : INT64_MIN / 2, lane);
    m = m > top ? m : top;
    int64_t end = m + i;
    end = end > L - 1 ? L - 1 : end;
    int64_t before = __shfl_up(end, 1, 64);  // end of segment i - 1
    if (lane == 0) before = prev_end;
    int64_t b = before + 1;
    b = b > L - 1 ? L - 1 : b;
    int64_t w = end - b + 1 - k;
    w = (live && w > 0) ? w : 0;
    const int64_t incl = wave_scan_sum(w, lane);
    if (live) W[slot] = (int32_t)(run + incl - w);
    run += __shfl(incl, 63, 64);
    top = __shfl(m, 63, 64);
    prev_end = __shfl(end, 63, 64);
  }
  if (lane == 0) A[e] = run;
}

static_assert(OGBX_ONLINE_ATC_TABLE_TILE % kTableScanThreads == 0, "whole items per thread");
using AtcScanConfig = TableScanConfig<OGBX_ONLINE_ATC_TABLE_TILE>;

static hipError_t table_scan(void* temp, size_t& temp_bytes, const int64_t* A, int64_t* P, int64_t n,
                             hipStream_t s) {
  return rocprim::exclusive_scan<AtcScanConfig>(temp, temp_bytes, A, P, (int64_t)0, (size_t)(n + 1),
                                                rocprim::plus<int64_t>(), s);
}

// temp = A, int64 [N + 1] padded to 256 bytes, then the scan's storage
static size_t counts_bytes(int64_t n) { return ((size_t)(n + 1) * sizeof(int64_t) + 255) & ~(size_t)255; }

// ----------------------------------------------------------------- the sample
struct OnlineAtcArgs {
  OnlineView ring;
  const int32_t* W;  // [T, N]
  const int64_t* P;  // [N + 1]
  int32_t env_iters;  // ceil(log2 N): halvings that bring [0, N) down to one env
  int64_t k;
  const int64_t *idxs, *pick, *crop_from;
  ogbx_atc_outputs out;
  ogbx_atc_column col;
  int32_t frame_stack, padding;
  int32_t draw;
  uint32_t k0, k1, call_lo, call_hi;
  uint32_t lds_bytes;
  int64_t total;
};

// Pick j of valid(k) (already in [0, max(P[N], 1))) -> env and anchor offset.
// Every index is in bounds whatever W, P and the tables hold: the env search
// stays inside [0, N), ordinals are reduced mod T, the rank, the segment's
// first offset and the result are clamped into [0, L - 1].
__device__ __forceinline__ void select_anchor(const OnlineAtcArgs& a, int64_t j, int64_t* e_out, int64_t* o_out) {
  const OnlineView& r = a.ring;
  const int64_t* __restrict__ P = a.P;
  const int32_t* __restrict__ W = a.W;
  // 1. the env: the largest e in [0, N) with P[e] <= j
  int64_t lo = 0, hi = r.n;
  for (int it = 0; it < a.env_iters; ++it) {
    const int64_t m = (lo + hi) >> 1;  // in [lo, hi) while lo < hi
    if (P[m] <= j) lo = m; else hi = m;
  }
  const int64_t e = lo;
  // 2. the rank, and the env's ordinals at its oldest and newest live row
  const int64_t base = P[e];
  const uint32_t s0 = (uint32_t)r.ep_seq[phys_row(r, e, 0)], sn = (uint32_t)r.ep_seq[phys_row(r, e, r.live - 1)];
  const int64_t rank = clamp_row(j - base, r.live);
  const uint32_t c = (uint32_t)clamp_row((int64_t)(sn - s0), r.live);
  // 3. the segment: the largest i in [0, c] with W_i <= rank (W_0 = 0)
  const uint32_t T = (uint32_t)r.horizon;
  uint32_t a0 = 0, z0 = c;
  int64_t wi = 0;
  while (a0 < z0) {
    const uint32_t m = (a0 + z0 + 1) >> 1;  // in (a0, z0]
    const int64_t w = W[(int64_t)((s0 + m) % T) * r.n + e];
    if (w <= rank) {
      a0 = m;
      wi = w;
    } else {
      z0 = m - 1;
    }
  }
  // 4. its first offset: one past the end of the segment before it
  int64_t b = 0;
  if (a0 > 0) b = clamp_row(r.ep_end[(int64_t)((s0 + a0 - 1) % T) * r.n + e] - r.first + 1, r.live);
  *e_out = e;
  *o_out = clamp_row(b + (rank - wi), r.live);
}

__global__ void __launch_bounds__(kVisThreads) online_atc_sample_kernel(OnlineAtcArgs a) {
  extern __shared__ uint4 onatc_lds4[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(onatc_lds4);
  int side;  // 0 anchor, 1 positive
  const int64_t s = atc_sample_of_block(blockIdx.x, &side);
  if (s >= a.total) return;
  const int t = threadIdx.x;
  const OnlineView& ring = a.ring;
  const int64_t L = ring.live;

  const int64_t far = a.k < L ? a.k : L;  // k as far as it matters: no row + far overflows
  int64_t e, o, pick = -1;
  bool bad = false;
  if (a.idxs) {  // an explicit flat row: its episode from the row's own ordinal, as online_gc_sample_kernel
    const int64_t raw = a.idxs[s];
    const int64_t u = clamp_row(raw, ring.npick);
    split_flat(ring, u, &e, &o);
    const int64_t fin = episode_end_flat(ring, episode_seq(ring, e, phys_row(ring, e, o)), u, e, o);
    bad = raw != u || u + far > fin;  // fin - u < L
  } else {
    const int64_t table = a.P[ring.n];
    const int64_t npick = table < 1 ? 1 : table;  // an empty table draws over one entry, and is counted
    if (a.pick) {
      pick = clamp_row(a.pick[s], npick);
    } else {
      const uint64_t su = (uint64_t)s;
      const u32x4 w = philox4x32_10({(uint32_t)su, a.call_lo, 0u, (uint32_t)(su >> 32) ^ a.call_hi}, a.k0, a.k1);
      pick = (int64_t)bounded64(w.x, w.y, (uint64_t)npick);
    }
    select_anchor(a, pick, &e, &o);
    bad = table < 1;
  }
  const int64_t os = side ? clamp_row(o + far, L) : o;
  const int F = a.frame_stack;
  const int64_t ofirst = stack_first(ring, e, os, F);

  const int p = a.padding;
  // the crop block and the lane-0 records stay written out in both ATC kernels: a
  // helper moved this kernel's code or the other's (profiles/atc_device_refactor_isa.txt)
  int cy = p, cx = p;  // identity
  if (a.crop_from || a.draw) {
    int64_t oy, ox;
    crop_offsets(a.crop_from, s, p, a.k0, a.k1, a.call_lo, a.call_hi, &oy, &ox);
    if (a.col.crop) {
      cy = (int)oy;
      cx = (int)ox;
    }
    if (a.out.crop_from && side == 0 && t == 0) {
      a.out.crop_from[2 * s] = oy;
      a.out.crop_from[2 * s + 1] = ox;
    }
  }
  if (side == 0 && t == 0) {
    if (a.out.idxs) a.out.idxs[s] = e * L + o;
    if (a.out.pick) a.out.pick[s] = pick;
    if (bad && a.out.bad_count) atomicAdd(reinterpret_cast<unsigned long long*>(a.out.bad_count), 1ull);
  }

  const ogbx_atc_column& col = a.col;
  const int64_t fb = (int64_t)col.height * (col.width * col.px_bytes);  // source frame bytes
  const uint8_t* __restrict__ src = static_cast<const uint8_t*>(col.src);
  uint8_t* dst = static_cast<uint8_t*>(side ? col.positive : col.anchor) + s * (fb * F);
  compose_frames(lds, a.lds_bytes, col.height, col.width, col.px_bytes, F, cy, cx, p, dst,
                 [&](int j) -> const uint8_t* {
                   int64_t oj = os - (F - 1 - j);
                   oj = oj < ofirst ? ofirst : oj;  // ofirst >= 0: a live row
                   return src + phys_row(ring, e, oj) * fb;
                 });
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_online_atc_api_version(void) { return OGBX_ONLINE_ATC_API_VERSION; }

ogbx_status ogbx_online_atc_table_bytes(int64_t num_envs, size_t* bytes) {
  const std::string who = "ogbx_online_atc_table_bytes: ";
  OGBX_CHECK(bytes, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(num_envs >= 1 && num_envs <= 0x7fffffffll, OGBX_EINVAL, who + "num_envs must lie in [1, 2^31)");
  size_t need = 0;
  OGBX_HIP(table_scan(nullptr, need, nullptr, nullptr, num_envs, nullptr));
  *bytes = counts_bytes(num_envs) + (need > 0 ? need : 1);
  return OGBX_OK;
}

ogbx_status ogbx_online_atc_table(const ogbx_online_ring* ring, int64_t k, int32_t* W, int64_t* P, void* temp,
                                  size_t temp_bytes, void* stream) {
  const std::string who = "ogbx_online_atc_table: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(W && P && temp, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  OGBX_CHECK(k >= 0, OGBX_EINVAL, who + "k must be >= 0");
  OGBX_CHECK(((uintptr_t)temp & 7) == 0, OGBX_EINVAL, who + "temp must be 8-byte aligned");
  const OnlineView v = online_view(*ring);
  int64_t* A = static_cast<int64_t*>(temp);
  const size_t head = counts_bytes(v.n);
  size_t need = 0;
  OGBX_HIP(table_scan(nullptr, need, A, P, v.n, (hipStream_t)stream));
  OGBX_CHECK(temp_bytes >= head + (need > 0 ? need : 1), OGBX_EINVAL,
             who + "temp_bytes below ogbx_online_atc_table_bytes");
  const int64_t blocks = (v.n + 1 + kCountWaves - 1) / kCountWaves;  // one wave per env, and one for A[N]
  hipLaunchKernelGGL(online_atc_count_kernel, dim3((uint32_t)blocks), dim3(kCountThreads), 0, (hipStream_t)stream, v,
                     k, W, A);
  OGBX_LAUNCHED("online_atc_count_kernel");
  size_t scan_bytes = temp_bytes - head;
  OGBX_HIP(table_scan(static_cast<uint8_t*>(temp) + head, scan_bytes, A, P, v.n, (hipStream_t)stream));
  return OGBX_OK;
}

ogbx_status ogbx_online_atc_sample(const ogbx_online_ring* ring, int64_t k, const int32_t* W, const int64_t* P,
                                   const ogbx_atc_column* col, int64_t total, int32_t frame_stack, int32_t padding,
                                   const int64_t* idxs, const int64_t* pick, const int64_t* crop_from,
                                   int32_t draw_crop, uint64_t seed, uint64_t call_index,
                                   const ogbx_atc_outputs* out, void* stream) {
  const std::string who = "ogbx_online_atc_sample: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(W && P && col, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  const AtcCall c{col,       total,     k,    frame_stack, padding, idxs, pick,
                  crop_from, draw_crop, seed, call_index,  out ? *out : ogbx_atc_outputs{}};
  if (ogbx_status st = check_atc_call(who, c)) return st;
  const ogbx_atc_outputs& o = c.out;
  uint32_t lds = 0;
  int64_t blocks = 0;
  if (ogbx_status st = atc_launch_shape(who, c, &lds, &blocks)) return st;

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  const bool ok = all_on_device(dev, {ring->ep_seq, ring->cur_seq, ring->ep_end, W, P, col->src, col->anchor,
                                      col->positive, idxs, pick, crop_from, o.idxs, o.pick, o.crop_from, o.bad_count});
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  OnlineAtcArgs a{};
  a.ring = online_view(*ring);
  a.W = W;
  a.P = P;
  while (((int64_t)1 << a.env_iters) < a.ring.n) ++a.env_iters;
  fill_atc_args(a, c, lds);
  hipLaunchKernelGGL(online_atc_sample_kernel, dim3((uint32_t)blocks), dim3(kVisThreads), lds, (hipStream_t)stream,
                     a);
  OGBX_LAUNCHED("online_atc_sample_kernel");
  return OGBX_OK;
}

}  // extern "C"
