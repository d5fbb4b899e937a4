// online.hip -- hindsight goal sampling over an on-device episode ring on
// gfx950 (include/ogbx_online.h): one row per env and step kept time-major,
// episode tables kept at O(1) per inserted row, and GCDataset.sample over the
// live rows in one launch.
//
// Reference (hliuson/ogbench):
//   GCDataset.sample            impls/utils/datasets.py:213-294
//   GCDataset.sample_goals      impls/utils/datasets.py:296-327
// over the snapshot of the ring: the live rows unrolled env-major, flat index
// u = e * L + k for env e at step S - L + k, a terminal on the last row of
// every closed episode and on every env's newest row.
//
// online_insert_kernel: replay_insert_kernel's tiles and row moves
// (replay_device.h) without a header or a keep mask: row e of step S goes to
// row (S % T) * N + e.  The thread of env e also writes ep_seq and, where done,
// the ep_end entry of the episode it closes and the env's next ordinal; no
// lane reads what another wrote.
//
// online_gc_sample_kernel: gc_sample_kernel's tile structure (gc_device.h) with
// the index loads replaced by the ring's: the flat pick is split into (e, k),
// its episode's end comes from ep_seq / cur_seq / ep_end, the goals are drawn
// on flat indices by sample_goal, and each selector is mapped to its physical
// row.  The ring's view, the row map and the end lookup live in
// online_device.h, shared with online_hgc_sample_kernel (online_hgc.hip); the
// prologue, the picks, the goal draws, the scalar stores, the draw record, the
// column check and the launch grid are gc_device.h's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ogbx_online.h"
#include "common.h"
#include "gc_device.h"
#include "online_device.h"
#include "replay_device.h"

namespace ogbx {

template <int N>
struct OnlineInsArgs {
  int64_t n;     // envs
  int64_t row0;  // (S % T) * N: the first row of this step's slot
  int64_t step;  // S
  uint32_t horizon;
  int32_t tile;  // rows per workgroup, <= kInsRows
  int32_t* ep_seq;
  int32_t* cur_seq;
  int64_t* ep_end;
  const uint8_t* done;
  const uint8_t* sel;
  int32_t num_cols;
  ogbx_replay_insert_column c[N];
};

template <int N, bool kNt>
__global__ void __launch_bounds__(kInsThreads) online_insert_kernel(OnlineInsArgs<N> a) {
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * a.tile;
  const int n_here = (int)((a.n - base) < a.tile ? (a.n - base) : a.tile);
  const int64_t row0 = a.row0;
  // the env's episode tables: tile <= kInsThreads, one env per thread.  Every
  // index lies below T * N: row0 + e by the host's row0, (seq % T) * N + e by
  // the modulo, whatever cur_seq holds.
  if (t < n_here) {
    const int64_t e = base + t;
    const uint32_t seq = (uint32_t)a.cur_seq[e];
    put<kNt>(a.ep_seq + row0 + e, (int32_t)seq);
    if (a.done[e]) {
      a.ep_end[(int64_t)(seq % a.horizon) * a.n + e] = a.step;
      a.cur_seq[e] = (int32_t)(seq + 1u);
    }
  }
  auto slot_of = [row0, base](int b) -> int64_t { return row0 + base + b; };
  insert_columns<kNt>(a.c, a.num_cols, a.sel, base, n_here, slot_of);
}

template <bool kInj>
__global__ void __launch_bounds__(256) online_gc_sample_kernel(
    OnlineView ring, ogbx_gc_config cfg, GcColumnsSmall cols, int32_t num_cols, int64_t total, int tile,
    ogbx_gc_draws dr, uint32_t k0, uint32_t k1, uint32_t call_lo, uint32_t call_hi, double v_log_q, double a_log_q,
    int64_t* idxs_out, int64_t* vgoal_out, int64_t* agoal_out, double* masks, double* rewards,
    ogbx_gc_draw_record rec, bool flat4) {
  __shared__ int64_t sel[4][kGcMaxTile];
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
    const int64_t npick = ring.npick;
    // the slot layout of gc_sample_kernel over npick rows without valid_idxs;
    // injected values are clamped into [0, npick)
    int64_t idx, pick;
    GoalDraws v, a;
    root_picks<kInj, true>(dr, s, w[0], w[1], npick, npick, &idx, &pick, &v.pick, &a.pick);
    // the row's episode end (online_device.h): ep_seq / cur_seq, then ep_end
    int64_t e, k;
    split_flat(ring, idx, &e, &k);
    const int64_t prow = phys_row(ring, e, k);
    const int64_t final_idx = episode_end_flat(ring, episode_seq(ring, e, prow), idx, e, k);
    goal_side_draws<kInj>(dr, cfg, s, w[1], w[2], w[3], w[4], v_log_q, a_log_q, v, a);
    int64_t vg = sample_goal(idx, final_idx, v, v.pick, cfg.value_p_curgoal, cfg.value_traj_thresh,
                             cfg.value_geom_sample, cfg.value_cur_is_one);
    int64_t ag = sample_goal(idx, final_idx, a, a.pick, cfg.actor_p_curgoal, cfg.actor_traj_thresh,
                             cfg.actor_geom_sample, cfg.actor_cur_is_one);
    // in [idx, final_idx] or a pick already; an injected geom / dist may leave
    vg = clamp_row(vg, npick);
    ag = clamp_row(ag, npick);
    const int64_t vrow = phys_of_flat(ring, vg), arow = phys_of_flat(ring, ag);
    if (own) {
      sel[0][b] = prow;
      sel[1][b] = prow;
      sel[2][b] = vrow;
      sel[3][b] = arow;
      store_gc_scalars(idxs_out, vgoal_out, agoal_out, masks, rewards, cfg.gc_negative, s, idx, vg, ag);
      store_draw_record(rec, s, pick, v, a);
    }
  }
  __syncthreads();
  copy_tile<0, false, GcColumnsSmall>(cols, num_cols, sel, base, n_here, flat4);
}

template <int N>
static ogbx_status launch_online_insert(const ogbx_online_ring& r, const ogbx_replay_insert_column* cols,
                                        int32_t num_cols, const uint8_t* done, const uint8_t* alt_select,
                                        hipStream_t s) {
  OnlineInsArgs<N> a{};
  a.n = r.num_envs;
  a.row0 = (r.steps % r.horizon) * r.num_envs;
  a.step = r.steps;
  a.horizon = (uint32_t)r.horizon;
  a.ep_seq = r.ep_seq;
  a.cur_seq = r.cur_seq;
  a.ep_end = r.ep_end;
  a.done = done;
  a.sel = alt_select;
  a.num_cols = num_cols;
  for (int i = 0; i < num_cols; ++i) a.c[i] = cols[i];
  // the rows per workgroup of replay_insert_kernel (the 4 B of ep_seq per row not counted)
  a.tile = insert_tile(cols, num_cols, r.num_envs);
  const int64_t blocks = (r.num_envs + a.tile - 1) / a.tile;
  hipLaunchKernelGGL((online_insert_kernel<N, kInsNt>), dim3((uint32_t)blocks), dim3(kInsThreads), 0, s, a);
  OGBX_LAUNCHED("online_insert_kernel");
  return OGBX_OK;
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_online_api_version(void) { return OGBX_ONLINE_API_VERSION; }

ogbx_status ogbx_online_insert(const ogbx_online_ring* ring, const ogbx_replay_insert_column* cols,
                               int32_t num_cols, const uint8_t* done, const uint8_t* alt_select, void* stream) {
  const std::string who = "ogbx_online_insert: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(done, OGBX_EINVAL, who + "null done");
  OGBX_CHECK(num_cols >= 0 && num_cols <= OGBX_REPLAY_MAX_COLS, OGBX_EINVAL, who + "0 to 16 columns");
  OGBX_CHECK(num_cols == 0 || cols, OGBX_EINVAL, who + "null columns");
  if (ogbx_status st = check_insert_columns(cols, num_cols, alt_select, who)) return st;
  hipStream_t s = (hipStream_t)stream;
  // the kernel arguments grow the host's launch cost (gc_device.h kGcSmallCols)
  if (num_cols <= 8) return launch_online_insert<8>(*ring, cols, num_cols, done, alt_select, s);
  return launch_online_insert<16>(*ring, cols, num_cols, done, alt_select, s);
}

ogbx_status ogbx_online_clear(const ogbx_online_ring* ring, void* stream) {
  const std::string who = "ogbx_online_clear: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_HIP(hipMemsetAsync(ring->cur_seq, 0, (size_t)ring->num_envs * sizeof(int32_t), (hipStream_t)stream));
  return OGBX_OK;
}

ogbx_status ogbx_online_gc_sample(const ogbx_online_ring* ring, const ogbx_gc_config* cfg,
                                  const ogbx_online_batch* batch, const ogbx_gc_draws* draws,
                                  const ogbx_gc_draw_record* record, uint64_t seed, uint64_t call_index,
                                  void* stream) {
  const std::string who = "ogbx_online_gc_sample: ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(cfg && batch, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  OGBX_CHECK(batch->masks && batch->rewards, OGBX_EINVAL, who + "null masks / rewards");
  OGBX_CHECK(batch->total > 0, OGBX_EINVAL, who + "total must be > 0");
  const int32_t num_cols = batch->num_cols;
  OGBX_CHECK(num_cols >= 0 && num_cols <= OGBX_REPLAY_MAX_COLS, OGBX_EINVAL, who + "0 to 16 columns");
  OGBX_CHECK(num_cols == 0 || batch->cols, OGBX_EINVAL, who + "null columns");
  GcColumnsSmall cc{};
  bool flat4;
  // the row itself and the two goals: a ring stores its own next_observations
  GC_TRY(check_gather_columns<true>(batch->cols, num_cols, 0b1101u, "ogbx_online_gc_sample", &cc, &flat4));
  const int64_t total = batch->total;
  int64_t tile, blocks;
  OGBX_CHECK(sample_grid(total, &tile, &blocks), OGBX_EINVAL, who + "too many samples for one launch");

  const OnlineView v = online_view(*ring);
  const ogbx_gc_draws dr = draws ? *draws : ogbx_gc_draws{};
  const GcParams pr = gc_params(seed, *cfg, nullptr);
  const auto kern = any_draw(dr) ? online_gc_sample_kernel<true> : online_gc_sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, v, *cfg, cc, num_cols, total,
                     (int)tile, dr, pr.k0, pr.k1, (uint32_t)call_index, (uint32_t)(call_index >> 32), pr.v_log_q,
                     pr.a_log_q, batch->idxs_out, batch->value_goal_out, batch->actor_goal_out, batch->masks,
                     batch->rewards, record ? *record : ogbx_gc_draw_record{}, flat4 && tile <= 4);
  OGBX_LAUNCHED("online_gc_sample_kernel");
  return OGBX_OK;
}

}  // extern "C"
