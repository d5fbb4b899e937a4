// online_hgc.hip -- hierarchical hindsight sampling over the on-device episode
// ring on gfx950 (include/ogbx_online_hgc.h): HGCDataset.sample over the live
// rows of an ogbx_online_ring in one launch.
//
// Reference (hliuson/ogbench):
//   HGCDataset.compute_high_next_idxs   impls/utils/datasets.py:478-491
//   HGCDataset.sample                   impls/utils/datasets.py:496-643
// over the snapshot of the ring (include/ogbx_online.h): the live rows unrolled
// env-major, flat index u = e * L + k for env e at step S - L + k.
//
// online_hgc_sample_kernel: hgc_sample_kernel's tile structure, slot layout and
// ten selectors (gcsample.hip, gc_device.h, gc_select.h) with the index loads
// replaced by the ring's (online_device.h), as online_gc_sample_kernel does it
// for the two GC goals, with the same pieces of gc_device.h and the host
// checks of ogbx_hgc_sample; the picks, words 5 and 6, the l_* draws and their
// record are written here (profiles/sampler_device_refactor_isa.txt).  All
// goal and subgoal arithmetic runs on flat indices;
// the five derived selectors stay in [idx, fin], i.e. in the sample's env, so
// their physical rows need no second division.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ogbx_online_hgc.h"
#include "common.h"
#include "gc_device.h"
#include "gc_select.h"
#include "online_device.h"

namespace ogbx {

template <bool kInj, class Cols>
__global__ void __launch_bounds__(256) online_hgc_sample_kernel(
    OnlineView ring, ogbx_gc_config cfg, ogbx_hgc_config hc, Cols cols, int32_t num_cols, int64_t total, int tile,
    ogbx_hgc_draws dr, uint32_t k0, uint32_t k1, uint32_t call_lo, uint32_t call_hi, double v_log_q, double a_log_q,
    double l_log_q, ogbx_hgc_outputs o, ogbx_hgc_draw_record rec, bool flat4) {
  __shared__ int64_t sel[kHgcSel][kGcMaxTile];
  __shared__ uint4 wb[7][kGcMaxTile];
  const int64_t base = xcd_tile() * tile;
  const int n_here = (int)((total - base) < tile ? (total - base) : tile);
  // the tile's Philox words, spread over the lanes (gc_device.h), in the
  // instance with injected draws too: its in-lane form spilled four SGPRs
  tile_philox(wb, hc.has_low_value_goals ? 7 : 5, n_here, base, call_lo, call_hi, k0, k1);
  __syncthreads();
  // what a lane of the first wave keeps of its sample for the scalar outputs
  struct {
    bool own = false;
    int64_t s = 0, idx = 0, hvg = 0, hag = 0, lvg = 0, hv_steps = 0, lv_steps = 0;
    double hv_mask = 0, hv_reward = 0, lv_mask = 0, lv_reward = 0;
  } r;
  auto store_scalars = [&]() {
    if (!r.own) return;
    const int64_t s = r.s;
    if (o.idxs) o.idxs[s] = r.idx;
    if (o.high_value_goal_idxs) o.high_value_goal_idxs[s] = r.hvg;
    if (o.high_actor_goal_idxs) o.high_actor_goal_idxs[s] = r.hag;
    if (o.low_value_goal_idxs) o.low_value_goal_idxs[s] = r.lvg;
    const double neg = cfg.gc_negative ? 1.0 : 0.0;
    o.high_value_offsets[s] = r.hvg - r.idx;
    o.high_value_subgoal_steps[s] = r.hv_steps;
    o.high_value_masks[s] = r.hv_mask;
    o.high_value_rewards[s] = r.hv_reward;
    o.low_value_subgoal_steps[s] = r.lv_steps;
    if (hc.has_low_value_goals) {
      const double ls = r.idx == r.lvg ? 1.0 : 0.0;
      o.low_value_masks[s] = 1.0 - ls;
      o.low_value_rewards[s] = ls - neg;
    } else {
      o.low_value_masks[s] = r.lv_mask;
      o.low_value_rewards[s] = r.lv_reward;
    }
    const double succ = r.idx == r.hvg ? 1.0 : 0.0;
    o.masks[s] = 1.0 - succ;
    o.rewards[s] = succ - neg;
  };
  if (threadIdx.x < 64 && n_here > 0) {  // the whole first wave: see gc_sample_kernel
    const int b = (int)threadIdx.x % n_here;
    const bool own = (int)threadIdx.x < n_here;
    const int64_t s = base + b;
    u32x4 w[5];
    sample_words<false>(wb, b, s, call_lo, call_hi, k0, k1, w);
    u32x4 w5{}, w6{};  // read here, not by sample_words: through it the two came out in other registers
    if (hc.has_low_value_goals) w5 = tile_word(wb, 5, b), w6 = tile_word(wb, 6, b);
    const int64_t npick = ring.npick;
    const ogbx_gc_draws& g = dr.gc;
    // the slot layout of hgc_sample_kernel over npick rows without valid_idxs;
    // injected values are clamped into [0, npick)
    // written out, not root_picks: it moves this kernel (profiles/sampler_device_refactor_isa.txt)
    int64_t idx, pick = -1;
    if (kInj && g.idxs) idx = clamp_row(g.idxs[s], npick);
    else
      idx = pick = (kInj && g.pick) ? clamp_row(g.pick[s], npick) : (int64_t)bounded64(w[0].x, w[0].y, (uint64_t)npick);
    GoalDraws v, a, l{};
    // the row's episode (online_device.h): ep_seq / cur_seq are in flight
    // while the draws below, which do not depend on them, are computed
    int64_t e, k;
    split_flat(ring, idx, &e, &k);
    const int64_t prow = phys_row(ring, e, k);
    const EpisodeSeq eps = episode_seq(ring, e, prow);
    v.pick = (kInj && g.v_pick) ? clamp_row(g.v_pick[s], npick) : (int64_t)bounded64(w[0].z, w[0].w, (uint64_t)npick);
    a.pick = (kInj && g.a_pick) ? clamp_row(g.a_pick[s], npick) : (int64_t)bounded64(w[1].x, w[1].y, (uint64_t)npick);
    goal_side_draws<kInj>(g, cfg, s, w[1], w[2], w[3], w[4], v_log_q, a_log_q, v, a);
    if (hc.has_low_value_goals) {
      l.pick = (kInj && dr.l_pick) ? clamp_row(dr.l_pick[s], npick) : (int64_t)bounded64(w5.x, w5.y, (uint64_t)npick);
      l.geom = (kInj && dr.l_geom) ? dr.l_geom[s] : geometric_from(u01_from(w5.z, w5.w), l_log_q);
      l.dist = 0.0;
      l.u_traj = (kInj && dr.l_u_traj) ? dr.l_u_traj[s] : u01_from(w6.x, w6.y);
      l.u_cur = (kInj && dr.l_u_cur) ? dr.l_u_cur[s] : u01_from(w6.z, w6.w);
    }
    // the episode's end: for a closed episode ep_end, the chain's third load
    const int64_t fin = episode_end_flat(ring, eps, idx, e, k);
    // the draw record (the kInj instance alone: a recording call launches it)
    if (kInj && own) {
      store_draw_record(rec.gc, s, pick, v, a);
      if (rec.l_pick && hc.has_low_value_goals) {
        rec.l_pick[s] = l.pick;
        rec.l_geom[s] = l.geom;
        rec.l_u_traj[s] = l.u_traj;
        rec.l_u_cur[s] = l.u_cur;
      }
    }
    // the three goals on flat indices, in the reference's call order; each lies
    // in [idx, fin] or is a pick already, an injected geom / dist may leave
    int64_t hvg = sample_goal(idx, fin, v, v.pick, cfg.value_p_curgoal, cfg.value_traj_thresh, cfg.value_geom_sample,
                              cfg.value_cur_is_one);
    int64_t lvg = idx;
    if (hc.has_low_value_goals)
      lvg = sample_goal(idx, fin, l, l.pick, cfg.value_p_curgoal, cfg.value_traj_thresh, 1, cfg.value_cur_is_one);
    int64_t hag = sample_goal(idx, fin, a, a.pick, cfg.actor_p_curgoal, cfg.actor_traj_thresh, cfg.actor_geom_sample,
                              cfg.actor_cur_is_one);
    hvg = clamp_row(hvg, npick);
    lvg = clamp_row(lvg, npick);
    hag = clamp_row(hag, npick);
    // fin >= idx, so every step count lies in [0, K] and every subgoal in [idx, fin]
    int64_t hv_next, lv_next, ha_next, ha_steps, la_next, la_steps;
    high_next(idx, fin, hvg, hc.value_subgoal_steps, &hv_next, &r.hv_steps);
    high_next(idx, fin, hvg, hc.low_subgoal_steps, &lv_next, &r.lv_steps);
    high_next(idx, fin, hag, hc.actor_subgoal_steps, &ha_next, &ha_steps);
    high_next(idx, fin, hag, hc.low_subgoal_steps, &la_next, &la_steps);
    const int64_t la_steps_goal = hc.actor_subgoal_steps < fin - idx ? hc.actor_subgoal_steps : fin - idx;
    if (own) {
      // the selectors first: the other waves wait for them at the barrier
      sel[0][b] = prow;
      sel[1][b] = prow;  // refused by the host
      sel[2][b] = phys_of_flat(ring, hvg);
      sel[3][b] = phys_of_flat(ring, hag);
      sel[4][b] = phys_row(ring, e, k + r.hv_steps);
      sel[5][b] = phys_row(ring, e, k + r.lv_steps);
      sel[6][b] = hc.has_low_value_goals ? phys_of_flat(ring, lvg) : prow;
      sel[7][b] = phys_row(ring, e, k + ha_steps);
      sel[8][b] = phys_row(ring, e, k + la_steps_goal);
      sel[9][b] = phys_row(ring, e, k + la_steps);
      // the table values load together and stay in flight across the barrier
      // (a load after each store would wait for the one before it: the compiler
      // cannot tell the tables from the outputs)
      r.hv_mask = hc.hv_mask_table[r.hv_steps];
      r.hv_reward = hc.hv_reward_table[r.hv_steps];
      if (!hc.has_low_value_goals) {
        r.lv_mask = hc.lv_mask_table[r.lv_steps];
        r.lv_reward = hc.lv_reward_table[r.lv_steps];
      }
      r.own = true;
      r.s = s;
      r.idx = idx;
      r.hvg = hvg;
      r.hag = hag;
      r.lvg = lvg;
    }
    if (kInj) store_scalars();
  }
  __syncthreads();
  // the scalars of the first wave's samples, beside the other waves' copies
  // (the instance with injected draws stores them before the barrier: holding
  // them across it spilled two SGPRs there)
  if (!kInj) store_scalars();
  copy_tile<0, false, Cols>(cols, num_cols, sel, base, n_here, flat4);
}

template <class Cols>
static ogbx_status launch_online_hgc(const OnlineView& v, const ogbx_gc_config& cfg, const ogbx_hgc_config& hcfg,
                                     const GcParams& pr, const ogbx_gc_column* cols, int32_t num_cols, bool flat4,
                                     int64_t total, int64_t tile, int64_t blocks, uint64_t call,
                                     const ogbx_hgc_draws& dr, const ogbx_hgc_draw_record& rec,
                                     const ogbx_hgc_outputs& o, hipStream_t s) {
  Cols cc{};
  for (int i = 0; i < num_cols; ++i) cc.c[i] = cols[i];
  // injected draws or a draw record: the Philox-only instance carries neither
  const bool inj = any_draw(dr.gc) || dr.l_pick || dr.l_geom || dr.l_u_traj || dr.l_u_cur || rec.gc.pick || rec.l_pick;
  const auto kern = inj ? online_hgc_sample_kernel<true, Cols> : online_hgc_sample_kernel<false, Cols>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, s, v, cfg, hcfg, cc, num_cols, total, (int)tile, dr,
                     pr.k0, pr.k1, (uint32_t)call, (uint32_t)(call >> 32), pr.v_log_q, pr.a_log_q, pr.l_log_q, o, rec,
                     tile <= 4 && flat4);
  OGBX_LAUNCHED("online_hgc_sample_kernel");
  return OGBX_OK;
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_online_hgc_api_version(void) { return OGBX_ONLINE_HGC_API_VERSION; }

ogbx_status ogbx_online_hgc_sample(const ogbx_online_ring* ring, const ogbx_gc_config* cfg,
                                   const ogbx_hgc_config* hcfg, const ogbx_gc_column* cols, int32_t num_cols,
                                   int64_t total, const ogbx_hgc_draws* draws, const ogbx_hgc_outputs* out,
                                   const ogbx_hgc_draw_record* record, uint64_t seed, uint64_t call_index,
                                   void* stream) {
  const char* name = "ogbx_online_hgc_sample";
  const std::string who = std::string(name) + ": ";
  if (ogbx_status st = check_ring(ring, who)) return st;
  OGBX_CHECK(cfg && hcfg && out, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(ring->steps >= 1, OGBX_EINVAL, who + "the ring is empty (steps must be >= 1)");
  OGBX_CHECK(total > 0, OGBX_EINVAL, who + "total must be > 0");
  GC_TRY(check_hgc_config(hcfg, name, 1, "subgoal steps must be >= 1"));
  GC_TRY(check_hgc_outputs(out, name));
  OGBX_CHECK(num_cols >= 0 && num_cols <= kGcMaxCols, OGBX_EINVAL, who + "0 to 32 columns");
  OGBX_CHECK(num_cols == 0 || cols, OGBX_EINVAL, who + "null columns");
  bool flat4;
  // every selector but next (1); the table is copied by launch_online_hgc, at the size it launches with
  GC_TRY(check_gather_columns<true>(cols, num_cols, selects_up_to(kHgcSel - 1) & ~0b10u, name,
                                    (GcColumns*)nullptr, &flat4));
  int64_t tile, blocks;
  OGBX_CHECK(sample_grid(total, &tile, &blocks), OGBX_EINVAL, who + "too many samples for one launch");

  const OnlineView v = online_view(*ring);
  const GcParams pr = gc_params(seed, *cfg, hcfg);
  const ogbx_hgc_draws dr = draws ? *draws : ogbx_hgc_draws{};
  const ogbx_hgc_draw_record rec = record ? *record : ogbx_hgc_draw_record{};
  // the kernel arguments grow the host's launch cost (gc_device.h kGcSmallCols)
  if (num_cols <= kGcSmallCols)
    return launch_online_hgc<GcColumnsSmall>(v, *cfg, *hcfg, pr, cols, num_cols, flat4, total, tile, blocks,
                                             call_index, dr, rec, *out, (hipStream_t)stream);
  return launch_online_hgc<GcColumns>(v, *cfg, *hcfg, pr, cols, num_cols, flat4, total, tile, blocks, call_index, dr,
                                      rec, *out, (hipStream_t)stream);
}

}  // extern "C"
