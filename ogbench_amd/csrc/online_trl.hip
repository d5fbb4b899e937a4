// online_trl.hip -- TRL batches over the on-device episode ring on gfx950
// (include/ogbx_online_trl.h): GCDataset.sample with a TRL agent name over the
// snapshot of the ring, whose pick table -- every live row that is not the
// last of its trajectory -- changes with every insert and is never built.
//
// Reference (hliuson/ogbench impls/utils/datasets.py):
//   GCDataset.__post_init__, TRL pick table   198-204
//   GCDataset.sample, TRL branch              254-276
//
// ogbx_online_trl_table: per env the count of pickable rows V[e] follows from
// the two ep_seq rows of the oldest and the newest live step; one device-wide
// exclusive scan (rocPRIM, the backend of the hipCUB select of gcsample.hip /
// trl.hip, taken directly so that its tile is this file's to fix) writes
// P[0 .. N] from a transform iterator, so V itself never reaches memory.
//
// online_trl_sample_kernel is organised as online_gc_sample_kernel
// (online.hip) and trl_sample_kernel (trl.hip): tiles of at most 64 samples
// numbered XCD-major, the first wave runs the draw chains into LDS selectors,
// then the whole workgroup copies rows (prologue: gc_device.h; bad-sample count,
// record check, pointer list: trl_device.h).  A pick j of the table becomes a row by
// select_pair: a search over P for the env, then a search over the env's live
// closed episodes (ep_end) for the terminal rows before the pick.  The sample's
// pick and the actor side's random goal are two independent chains; both
// searches advance them in one loop body, so their loads are in flight
// together.  The picked row's episode is known from the search, so its end
// costs one ep_end load and none of ep_seq.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/ogbx_online_trl.h"
#include "common.h"
#include "gc_device.h"
#include "online_device.h"
#include "trl_device.h"

namespace ogbx {

constexpr int kOnlineTrlSel = OGBX_TRL_SELECT_MIDPOINT + 1;

// ------------------------------------------------------------------ the table
// V[e] for e < N, 0 for the scan's last item (so that P[N] is the total).
struct PickableRows {
  const int32_t* seq0;  // ep_seq row of step S - L
  const int32_t* seqn;  // ep_seq row of step S - 1
  int64_t n, live;
  __device__ int64_t operator()(int64_t e) const {
    if (e >= n) return 0;
    const uint32_t closed = (uint32_t)seqn[e] - (uint32_t)seq0[e];
    const int64_t v = live - 1 - (int64_t)closed;
    return v < 0 ? 0 : (v > live - 1 ? live - 1 : v);  // whatever the rows hold
  }
};

static_assert(OGBX_ONLINE_TRL_TABLE_TILE % kTableScanThreads == 0, "whole items per thread");
using TrlScanConfig = TableScanConfig<OGBX_ONLINE_TRL_TABLE_TILE>;

static hipError_t table_scan(void* temp, size_t& temp_bytes, const PickableRows& rows, int64_t* P, hipStream_t s) {
  auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), rows);
  return rocprim::exclusive_scan<TrlScanConfig>(temp, temp_bytes, in, P, (int64_t)0, (size_t)(rows.n + 1),
                                                rocprim::plus<int64_t>(), s);
}

// ----------------------------------------------------------------- the select
// What the sample kernel needs of the table besides the ring's view.
struct OnlineTrlTable {
  const int64_t* P;   // [N + 1]
  int32_t env_iters;  // ceil(log2 N): halvings that bring [0, N) down to one env
};

// A selected pick: env, live offset, and its episode as episode_end_flat takes
// it (seq: the row's ordinal; cur: the ordinal of the env's newest row, whose
// episode ends at step S - 1 whether it is open or closes there).
struct PickedRow {
  int64_t e, k;
  EpisodeSeq ep;
};

// Picks j0, j1 of the table (each already in [0, max(P[N], 1))) -> rows.
// Every index is in bounds whatever P and the tables hold: the env search stays
// inside [0, N), ordinals are reduced mod T, the rank and k are clamped into
// [0, L - 1].
__device__ __forceinline__ void select_pair(const OnlineView& r, const OnlineTrlTable& t, int64_t j0, int64_t j1,
                                            PickedRow* o0, PickedRow* o1) {
  const int64_t* __restrict__ P = t.P;
  // 1. the env: the largest e in [0, N) with P[e] <= j
  // (halvings: eight-way rounds with seven pivots loaded together, 4 and 6
  // rounds instead of 10 and 16, measured 0.8 and 0.9 us slower per launch at
  // N = 1,024 and N = 65,536: profiles/online_trl_sampler.json, earlier_forms)
  int64_t lo0 = 0, hi0 = r.n, lo1 = 0, hi1 = r.n;
  for (int it = 0; it < t.env_iters; ++it) {
    const int64_t m0 = (lo0 + hi0) >> 1, m1 = (lo1 + hi1) >> 1;  // in [lo, hi) while lo < hi
    const int64_t p0 = P[m0], p1 = P[m1];
    if (p0 <= j0) lo0 = m0; else hi0 = m0;
    if (p1 <= j1) lo1 = m1; else hi1 = m1;
  }
  const int64_t e0 = lo0, e1 = lo1;
  // 2. the rank, and the env's ordinals at its oldest and newest live row
  const int64_t first0 = phys_row(r, e0, 0), last0 = phys_row(r, e0, r.live - 1);
  const int64_t first1 = phys_row(r, e1, 0), last1 = phys_row(r, e1, r.live - 1);
  const int64_t b0 = P[e0], b1 = P[e1];
  const uint32_t s0 = (uint32_t)r.ep_seq[first0], n0 = (uint32_t)r.ep_seq[last0];
  const uint32_t s1 = (uint32_t)r.ep_seq[first1], n1 = (uint32_t)r.ep_seq[last1];
  const int64_t r0 = clamp_row(j0 - b0, r.live), r1 = clamp_row(j1 - b1, r.live);
  const uint32_t c0 = (uint32_t)clamp_row((int64_t)(n0 - s0), r.live);  // closed before the newest row
  const uint32_t c1 = (uint32_t)clamp_row((int64_t)(n1 - s1), r.live);
  // 3. the terminal rows before the pick: the smallest i in [0, c) with G(i) > rank, else c
  const uint32_t T = (uint32_t)r.horizon;
  uint32_t a0 = 0, z0 = c0, a1 = 0, z1 = c1;
  while (a0 < z0 || a1 < z1) {
    const bool go0 = a0 < z0, go1 = a1 < z1;
    const uint32_t m0 = (a0 + z0) >> 1, m1 = (a1 + z1) >> 1;
    int64_t g0 = 0, g1 = 0;
    if (go0) g0 = r.ep_end[(int64_t)((s0 + m0) % T) * r.n + e0];
    if (go1) g1 = r.ep_end[(int64_t)((s1 + m1) % T) * r.n + e1];
    if (go0) {
      if (g0 - r.first - (int64_t)m0 > r0) z0 = m0; else a0 = m0 + 1;
    }
    if (go1) {
      if (g1 - r.first - (int64_t)m1 > r1) z1 = m1; else a1 = m1 + 1;
    }
  }
  o0->e = e0;
  o0->k = clamp_row(r0 + (int64_t)a0, r.live);
  o0->ep = EpisodeSeq{s0 + a0, s0 + c0};
  o1->e = e1;
  o1->k = clamp_row(r1 + (int64_t)a1, r.live);
  o1->ep = EpisodeSeq{s1 + a1, s1 + c1};
}

template <bool kInj>
__global__ void __launch_bounds__(256) online_trl_sample_kernel(
    OnlineView ring, OnlineTrlTable tab, ogbx_gc_config cfg, GcColumns cols, int32_t num_cols, int64_t total, int tile,
    ogbx_gc_draws dr, const int64_t* __restrict__ mid_in, uint32_t k0, uint32_t k1, uint32_t call_lo,
    uint32_t call_hi, double v_log_q, double a_log_q, ogbx_trl_outputs o, ogbx_gc_draw_record rec,
    int64_t* __restrict__ mid_rec, bool flat4) {
  __shared__ int64_t sel[kOnlineTrlSel][kGcMaxTile];
  __shared__ uint4 wb[(!kInj && kGcSpread) ? 5 : 1][kGcMaxTile];
  const int64_t base = xcd_tile() * tile;
  const int n_here = (int)((total - base) < tile ? (total - base) : tile);
  if (!kInj && kGcSpread) {
    tile_philox(wb, 5, n_here, base, call_lo, call_hi, k0, k1);
    __syncthreads();
  }
  if (threadIdx.x < 64 && n_here > 0) {  // the whole first wave: see gc_sample_kernel
    const int b = (int)threadIdx.x % n_here;
    const bool own = (int)threadIdx.x < n_here;
    const int64_t s = base + b;
    u32x4 w[5];
    sample_words<kInj || !kGcSpread>(wb, b, s, call_lo, call_hi, k0, k1, w);
    // the slot layout of trl_sample_kernel over a pick table of P[N] entries;
    // an empty table draws over one entry (every sample is then counted bad)
    const int64_t rows = ring.npick;  // L * N
    const int64_t table = tab.P[ring.n];
    const int64_t npick = table < 1 ? 1 : table;
    const bool given = kInj && dr.idxs != nullptr;
    // written out, not root_picks: it moves this kernel (profiles/sampler_device_refactor_isa.txt)
    int64_t pick = -1;
    if (!given)
      pick = (kInj && dr.pick) ? clamp_row(dr.pick[s], npick) : (int64_t)bounded64(w[0].x, w[0].y, (uint64_t)npick);
    GoalDraws v, a;
    v.pick = (kInj && dr.v_pick) ? clamp_row(dr.v_pick[s], npick) : (int64_t)bounded64(w[0].z, w[0].w, (uint64_t)npick);
    a.pick = (kInj && dr.a_pick) ? clamp_row(dr.a_pick[s], npick) : (int64_t)bounded64(w[1].x, w[1].y, (uint64_t)npick);
    // an injected midpoint row: loaded with the index loads, not after them
    const int64_t mid_given = (kInj && mid_in) ? mid_in[s] : 0;
    PickedRow pr, ar;
    select_pair(ring, tab, given ? 0 : pick, a.pick, &pr, &ar);
    int64_t idx;
    if (given) {  // an explicit flat row: its episode from the row's own ordinal, as online_gc_sample_kernel
      idx = clamp_row(dr.idxs[s], rows);
      split_flat(ring, idx, &pr.e, &pr.k);
      pr.ep = episode_seq(ring, pr.e, phys_row(ring, pr.e, pr.k));
    } else {
      idx = pr.e * ring.live + pr.k;
    }
    const int64_t prow = phys_row(ring, pr.e, pr.k);
    const int64_t final_idx = episode_end_flat(ring, pr.ep, idx, pr.e, pr.k);
    const int64_t a_rand = ar.e * ring.live + ar.k;
    goal_side_draws<kInj>(dr, cfg, s, w[1], w[2], w[3], w[4], v_log_q, a_log_q, v, a);
    // the value side has no random goal (the host refuses such a cfg); only an
    // injected u_traj >= 1 reaches its slot, and then counts as bad
    int64_t vg = sample_goal(idx, final_idx, v, idx, cfg.value_p_curgoal, cfg.value_traj_thresh,
                             cfg.value_geom_sample, cfg.value_cur_is_one);
    int64_t ag = sample_goal(idx, final_idx, a, a_rand, cfg.actor_p_curgoal, cfg.actor_traj_thresh,
                             cfg.actor_geom_sample, cfg.actor_cur_is_one);
    // in [idx, final_idx] or a selected row already; an injected geom / dist may leave
    vg = clamp_row(vg, rows);
    ag = clamp_row(ag, rows);
    // value midpoint: randint(idx, vg) (datasets.py:259), words z, w of slot 4.
    // No row lies in [idx, vg) when vg <= idx: counted, and mid = idx.
    const int64_t span = vg - idx;
    const bool bad = span <= 0 || table < 1;
    int64_t mid = idx;
    if (!bad)
      mid = (kInj && mid_in) ? clamp_row(mid_given, rows) : idx + (int64_t)bounded64(w[4].z, w[4].w, (uint64_t)span);
    count_bad_samples(o.bad_count, bad, own);
    const int64_t next = idx + 1 < rows ? idx + 1 : rows - 1;
    const int64_t nrow = phys_of_flat(ring, next), vrow = phys_of_flat(ring, vg), arow = phys_of_flat(ring, ag),
                  mrow = phys_of_flat(ring, mid);
    if (own) {
      sel[0][b] = prow;
      sel[1][b] = nrow;
      sel[2][b] = vrow;
      sel[3][b] = arow;
      sel[4][b] = mrow;
      // written out, as the midpoint: one helper moved either TRL kernel (profiles/sampler_device_refactor_isa.txt)
      if (o.idxs) o.idxs[s] = idx;
      if (o.value_goal_idxs) o.value_goal_idxs[s] = vg;
      if (o.actor_goal_idxs) o.actor_goal_idxs[s] = ag;
      if (o.value_midpoint_idxs) o.value_midpoint_idxs[s] = mid;
      if (o.value_offsets) o.value_offsets[s] = span;
      if (o.value_midpoint_offsets) o.value_midpoint_offsets[s] = mid - idx;
      const double succ = idx == vg ? 1.0 : 0.0;
      if (o.masks) o.masks[s] = 1.0 - succ;
      if (o.rewards) o.rewards[s] = succ - (cfg.gc_negative ? 1.0 : 0.0);
      if (mid_rec) mid_rec[s] = mid;
      store_draw_record(rec, s, pick, v, a);
    }
  }
  __syncthreads();
  copy_tile<0>(cols, num_cols, sel, base, n_here, flat4);
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_online_trl_api_version(void) { return OGBX_ONLINE_TRL_API_VERSION; }

ogbx_status ogbx_online_trl_table_bytes(int64_t num_envs, size_t* bytes) {
  const std::string who = "ogbx_online_trl_table_bytes: ";
  OGBX_CHECK(bytes, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(num_envs >= 1 && num_envs <= 0x7fffffffll, OGBX_EINVAL, who + "num_envs must lie in [1, 2^31)");
  size_t need = 0;
  OGBX_HIP(table_scan(nullptr, need, PickableRows{nullptr, nullptr, num_envs, 1}, nullptr, nullptr));
  *bytes = need > 0 ? need : 1;
  return OGBX_OK;
}

ogbx_status ogbx_online_trl_table(const ogbx_online_ring* ring, int64_t* P, void* temp, size_t temp_bytes,
                                  void* stream) {
  const std::string who = "ogbx_online_trl_table: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(P && temp, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  const OnlineView v = online_view(*ring);
  const PickableRows rows{ring->ep_seq + v.slot0 * v.n, ring->ep_seq + (v.last % v.horizon) * v.n, v.n, v.live};
  size_t need = 0;
  OGBX_HIP(table_scan(nullptr, need, rows, P, (hipStream_t)stream));
  OGBX_CHECK(temp_bytes >= (need > 0 ? need : 1), OGBX_EINVAL, who + "temp_bytes below ogbx_online_trl_table_bytes");
  OGBX_HIP(table_scan(temp, temp_bytes, rows, P, (hipStream_t)stream));
  return OGBX_OK;
}

ogbx_status ogbx_online_trl_sample(const ogbx_online_ring* ring, const int64_t* P, const ogbx_gc_config* cfg,
                                   const ogbx_gc_column* cols, int32_t num_cols, int64_t total,
                                   const ogbx_gc_draws* draws, const int64_t* midpoint, uint64_t seed,
                                   uint64_t call_index, const ogbx_trl_outputs* out,
                                   const ogbx_gc_draw_record* record, int64_t* midpoint_record, void* stream) {
  const char* name = "ogbx_online_trl_sample";
  const std::string who = std::string(name) + ": ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(P && cfg && out && (cols || num_cols == 0), OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  OGBX_CHECK(total > 0, OGBX_EINVAL, who + "total must be > 0");
  OGBX_CHECK(cfg->value_p_curgoal == 0.0 && cfg->value_traj_thresh >= 1.0 && !cfg->value_cur_is_one, OGBX_EINVAL,
             who + "a TRL batch needs value_p_curgoal == 0 and no random value goals (value_traj_thresh >= 1)");
  GcColumns cc{};
  bool flat4;
  GC_TRY(check_columns(cols, num_cols, total, 1, OGBX_TRL_SELECT_MIDPOINT, name, &cc, &flat4));
  const ogbx_gc_draws dr = draws ? *draws : ogbx_gc_draws{};
  const ogbx_gc_draw_record rec = record ? *record : ogbx_gc_draw_record{};
  GC_TRY(check_draw_record_complete(rec, name));
  int64_t tile, blocks;
  OGBX_CHECK(sample_grid(total, &tile, &blocks), OGBX_EINVAL, who + "too many samples for one launch");

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  OGBX_CHECK(all_on_device(dev, {P, ring->ep_seq, ring->cur_seq, ring->ep_end}) &&
                 trl_pointers_on_device(dev, dr, rec, *out, midpoint, midpoint_record, cols, num_cols),
             OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  const OnlineView v = online_view(*ring);
  OnlineTrlTable tab{P, 0};
  while (((int64_t)1 << tab.env_iters) < v.n) ++tab.env_iters;
  const GcParams pr = gc_params(seed, *cfg, nullptr);  // the GC stream tag: same words as ogbx_trl_sample
  const auto kern = (any_draw(dr) || midpoint) ? online_trl_sample_kernel<true> : online_trl_sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, v, tab, *cfg, cc, num_cols,
                     total, (int)tile, dr, midpoint, pr.k0, pr.k1, (uint32_t)call_index,
                     (uint32_t)(call_index >> 32), pr.v_log_q, pr.a_log_q, *out, rec, midpoint_record,
                     tile <= 4 && flat4);
  OGBX_LAUNCHED("online_trl_sample_kernel");
  return OGBX_OK;
}

}  // extern "C"
