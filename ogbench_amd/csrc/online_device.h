// online_device.h -- what the sample kernels over the episode ring share
// (online.hip, online_hgc.hip, online_visual.hip, online_trl.hip,
// online_atc.hip; include/ogbx_online.h): the ring as a kernel argument, the
// flat-to-physical row map, the episode-end lookup, the first row of a frame
// stack, and the host-side ring check.  Internal to libogbx.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include <rocprim/device/device_scan_config.hpp>

#include "../../include/ogbx_online.h"
#include "../../include/ogbx_visual.h"
#include "common.h"

namespace ogbx {

// What a sample kernel needs of the ring, derived on the host from (N, T, S).
struct OnlineView {
  const int32_t* ep_seq;
  const int32_t* cur_seq;
  const int64_t* ep_end;
  int64_t n;         // N
  int64_t live;      // L = min(S, T)
  int64_t first;     // S - L, the step of k = 0
  int64_t last;      // S - 1
  int64_t slot0;     // first % T
  int64_t horizon;   // T
  int64_t npick;     // L * N
  double inv_live;   // 1 / L
};

// Flat index u in [0, L * N) -> (e, k) with u = e * L + k.  The quotient
// estimate by the reciprocal is within one of floor(u / L) (u < 2^46 is exact
// in a double); the remainder test makes it exact (as periodic_row).
__device__ __forceinline__ void split_flat(const OnlineView& r, int64_t u, int64_t* e, int64_t* k) {
  int64_t q = (int64_t)((double)u * r.inv_live);
  int64_t rem = u - q * r.live;
  if (rem < 0) {
    --q;
    rem += r.live;
  } else if (rem >= r.live) {
    ++q;
    rem -= r.live;
  }
  *e = q;
  *k = rem;
}

// Physical row of env e < N at live offset k < L: slot0 + k < 2 T.
__device__ __forceinline__ int64_t phys_row(const OnlineView& r, int64_t e, int64_t k) {
  int64_t s = r.slot0 + k;
  s = s >= r.horizon ? s - r.horizon : s;
  return s * r.n + e;
}

__device__ __forceinline__ int64_t phys_of_flat(const OnlineView& r, int64_t u) {
  int64_t e, k;
  split_flat(r, u, &e, &k);
  return phys_row(r, e, k);
}

// The episode of flat row idx = e * L + k (physical row prow), in two steps.
// First the row's ordinal and the env's open one, which load together.
struct EpisodeSeq {
  uint32_t seq, cur;
};

__device__ __forceinline__ EpisodeSeq episode_seq(const OnlineView& ring, int64_t e, int64_t prow) {
  return EpisodeSeq{(uint32_t)ring.ep_seq[prow], (uint32_t)ring.cur_seq[e]};
}

// Then the episode's end as a flat index of the same env; the table entry of a
// closed episode loads after the two ordinals.  The end step is clamped into
// [row's step, S - 1] whatever the table holds, so
// idx <= result <= e * L + L - 1.  A kernel puts what does not depend on the
// ordinals between the two calls, where it runs while they are in flight.
__device__ __forceinline__ int64_t episode_end_flat(const OnlineView& ring, const EpisodeSeq& s, int64_t idx,
                                                    int64_t e, int64_t k) {
  const int64_t step = ring.first + k;
  int64_t end = ring.last;  // an open episode ends now
  if (s.seq != s.cur) {
    end = ring.ep_end[(int64_t)(s.seq % (uint32_t)ring.horizon) * ring.n + e];
    end = end < step ? step : (end > ring.last ? ring.last : end);  // whatever the table holds
  }
  return idx + (end - step);  // same env: e * L + (end - first)
}

// The live offset of the first row of the stack of n frames that ends at
// offset k of env e: the earliest of k - (n-1) .. k that is live (>= 0) and
// has the row's ep_seq.  The ordinals load together (no load waits for a
// compare); ep_seq does not decrease along an env's live steps, so the rows
// of the episode are the run that ends at k.
__device__ __forceinline__ int64_t stack_first(const OnlineView& ring, int64_t e, int64_t k, int n) {
  if (n <= 1) return k;
  int32_t seq[OGBX_VISUAL_MAX_STACK] = {};
#pragma unroll
  for (int i = 0; i < OGBX_VISUAL_MAX_STACK; ++i)
    if (i < n && k - i >= 0) seq[i] = ring.ep_seq[phys_row(ring, e, k - i)];
  int run = 0;  // rows before k that belong
  bool open = true;
#pragma unroll
  for (int i = 1; i < OGBX_VISUAL_MAX_STACK; ++i) {
    open = open && i < n && k - i >= 0 && seq[i] == seq[0];
    run += open ? 1 : 0;
  }
  return k - run;
}

// ---------------------------------------------------------------- host side
// The device-wide scan that turns the per-env counts of a ring table into its
// prefix table P (online_trl.hip, online_atc.hip), its tile fixed at Tile items.
constexpr unsigned kTableScanThreads = 256;
template <unsigned Tile>
using TableScanConfig =
    rocprim::scan_config<kTableScanThreads, Tile / kTableScanThreads, rocprim::block_load_method::block_load_transpose,
                         rocprim::block_store_method::block_store_transpose,
                         rocprim::block_scan_algorithm::using_warp_scan>;

constexpr int64_t kOnlineMaxRows = (int64_t)1 << 46;  // flat indices stay exact in a double

static ogbx_status check_ring(const ogbx_online_ring* r, const std::string& who) {
  OGBX_CHECK(r, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(r->ep_seq && r->cur_seq && r->ep_end, OGBX_EINVAL, who + "null episode table");
  OGBX_CHECK(r->num_envs >= 1 && r->num_envs <= 0x7fffffffll, OGBX_EINVAL, who + "num_envs must lie in [1, 2^31)");
  OGBX_CHECK(r->horizon >= 1 && r->horizon <= 0x7fffffffll, OGBX_EINVAL, who + "horizon must lie in [1, 2^31)");
  OGBX_CHECK(r->num_envs * r->horizon < kOnlineMaxRows, OGBX_EINVAL, who + "num_envs * horizon must be below 2^46");
  OGBX_CHECK(r->steps >= 0, OGBX_EINVAL, who + "steps must be >= 0");
  return OGBX_OK;
}

// The view of a checked ring with steps >= 1.
static OnlineView online_view(const ogbx_online_ring& ring) {
  OnlineView v{};
  v.ep_seq = ring.ep_seq;
  v.cur_seq = ring.cur_seq;
  v.ep_end = ring.ep_end;
  v.n = ring.num_envs;
  v.horizon = ring.horizon;
  v.live = std::min(ring.steps, ring.horizon);
  v.first = ring.steps - v.live;
  v.last = ring.steps - 1;
  v.slot0 = v.first % v.horizon;
  v.npick = v.live * v.n;
  v.inv_live = 1.0 / (double)v.live;
  return v;
}

}  // namespace ogbx
