// gcsample.hip -- offline replay on gfx950: one fused launch draws the sample
// indices, relabels value/actor goals in hindsight and gathers every dataset
// column of the batch from the HBM-resident trajectory buffer.
//
// Reference (hliuson/ogbench):
//   Dataset.get_random_idxs / get_subset   impls/utils/datasets.py:65-83
//   GCDataset.sample                       impls/utils/datasets.py:213-294
//   GCDataset.sample_goals                 impls/utils/datasets.py:296-327
//
// Layout: every column is a dense [R, row_bytes] device array (torch tensor).
// One workgroup handles a tile of TB samples: lanes 0..TB-1 compute the four
// row selectors of their sample into LDS, then all 256 lanes stream the rows
// of every column (widest aligned unit: 16, 8 or 4 bytes) into the batch.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <type_traits>

#include "common.h"
#include "gc_device.h"
#include "gc_select.h"

namespace ogbx {

// The draw chain, the first wave's prologue, the tile helpers and the shared
// argument checks: gc_device.h (trl.hip and the ring samplers build their
// kernels from the same pieces).

template <bool kInj>
__global__ void __launch_bounds__(256) gc_sample_kernel(
    ogbx_gc_buffer buf, ogbx_gc_config cfg, GcColumns cols, int32_t num_cols, int64_t total,
    int tile, ogbx_gc_draws dr, uint32_t k0, uint32_t k1, uint32_t call_lo, uint32_t call_hi,
    double v_log_q, double a_log_q, int64_t* idxs_out, int64_t* vgoal_out, int64_t* agoal_out,
    double* masks, double* rewards, ogbx_gc_draw_record rec, bool flat4) {
  __shared__ int64_t sel[4][kGcMaxTile];
  __shared__ uint4 wb[(!kInj && kGcSpread) ? 5 : 1][kGcMaxTile];
  const int64_t base = xcd_tile() * tile;
  const int n_here = (int)((total - base) < tile ? (total - base) : tile);
  if (!kInj && kGcSpread) {
    tile_philox(wb, 5, n_here, base, call_lo, call_hi, k0, k1);
    __syncthreads();
  }
  // The whole first wave runs the sample chains (lane b % n_here; only lanes
  // b < n_here store): a chain on a few active lanes issues about twice as
  // slowly on gfx950, and a B = 1,024 tile has one sample.
  if (threadIdx.x < 64 && n_here > 0) {
    const int b = (int)threadIdx.x % n_here;
    const bool own = (int)threadIdx.x < n_here;
    const int64_t s = base + b;
    u32x4 w[5];
    sample_words<kInj || !kGcSpread>(wb, b, s, call_lo, call_hi, k0, k1, w);
    const int64_t npick = buf.valid_idxs ? buf.num_valid : buf.num_rows;
    // sample index (datasets.py:65-70)
    int64_t idx = 0, pick, final_idx;
    GoalDraws v, a;
    root_picks<kInj, false>(dr, s, w[0], w[1], npick, buf.num_rows, &idx, &pick, &v.pick, &a.pick);
    index_loads(buf, kInj && dr.idxs != nullptr, pick, &idx, &final_idx);
    const int64_t v_rand = cfg.value_cur_is_one ? 0 : rand_goal_of(buf, v.pick);
    const int64_t a_rand = cfg.actor_cur_is_one ? 0 : rand_goal_of(buf, a.pick);
    const int64_t next = idx + 1 < buf.num_rows ? idx + 1 : buf.num_rows - 1;
    goal_side_draws<kInj>(dr, cfg, s, w[1], w[2], w[3], w[4], v_log_q, a_log_q, v, a);
    const int64_t vg = sample_goal(idx, final_idx, v, v_rand, cfg.value_p_curgoal,
                                   cfg.value_traj_thresh, cfg.value_geom_sample, cfg.value_cur_is_one);
    const int64_t ag = sample_goal(idx, final_idx, a, a_rand, cfg.actor_p_curgoal,
                                   cfg.actor_traj_thresh, cfg.actor_geom_sample, cfg.actor_cur_is_one);
    if (own) {
      sel[0][b] = idx;
      sel[1][b] = next;
      sel[2][b] = vg;
      sel[3][b] = ag;
      store_gc_scalars(idxs_out, vgoal_out, agoal_out, masks, rewards, cfg.gc_negative, s, idx, vg, ag);
      store_draw_record(rec, s, pick, v, a);
    }
  }
  __syncthreads();
  copy_tile<0>(cols, num_cols, sel, base, n_here, flat4);
}

// ---------------------------------------------------------------- look-ahead
// One sample's selectors and scalars, as GCDataset.sample draws them with the
// Philox words w0..w4 (the same arithmetic as gc_sample_kernel's Philox path).
struct GcPick {
  int64_t idx, next, vg, ag;
  double mask, reward;
};

__device__ inline GcPick gc_chain(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg, const u32x4& w0,
                                  const u32x4& w1, const u32x4& w2, const u32x4& w3, const u32x4& w4,
                                  double v_log_q, double a_log_q) {
  const int64_t npick = buf.valid_idxs ? buf.num_valid : buf.num_rows;
  const int64_t pick = (int64_t)bounded64(w0.x, w0.y, (uint64_t)npick);
  GoalDraws v, a;
  v.pick = (int64_t)bounded64(w0.z, w0.w, (uint64_t)npick);
  a.pick = (int64_t)bounded64(w1.x, w1.y, (uint64_t)npick);
  int64_t idx = 0, final_idx;
  index_loads(buf, false, pick, &idx, &final_idx);
  const int64_t v_rand = cfg.value_cur_is_one ? 0 : rand_goal_of(buf, v.pick);
  const int64_t a_rand = cfg.actor_cur_is_one ? 0 : rand_goal_of(buf, a.pick);
  goal_side_draws<false>(ogbx_gc_draws{}, cfg, 0, w1, w2, w3, w4, v_log_q, a_log_q, v, a);
  GcPick p;
  p.idx = idx;
  p.next = idx + 1 < buf.num_rows ? idx + 1 : buf.num_rows - 1;
  p.vg = sample_goal(idx, final_idx, v, v_rand, cfg.value_p_curgoal, cfg.value_traj_thresh, cfg.value_geom_sample,
                     cfg.value_cur_is_one);
  p.ag = sample_goal(idx, final_idx, a, a_rand, cfg.actor_p_curgoal, cfg.actor_traj_thresh, cfg.actor_geom_sample,
                     cfg.actor_cur_is_one);
  const double succ = idx == p.vg ? 1.0 : 0.0;
  p.mask = 1.0 - succ;
  p.reward = succ - (cfg.gc_negative ? 1.0 : 0.0);
  return p;
}

// The first wave's chain of sample s under call (lo, hi): lanes 0..4 each run
// one Philox call, every lane then runs the chain on the broadcast words (a
// chain on one active lane issues about twice as slowly).
__device__ inline GcPick gc_wave_chain(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg, int64_t s, uint32_t lo,
                                       uint32_t hi, uint32_t k0, uint32_t k1, double v_log_q, double a_log_q) {
  const uint64_t su = (uint64_t)s;
  const uint32_t q = (uint32_t)(threadIdx.x & 63) % 5u;
  const u32x4 w = philox4x32_10({(uint32_t)su, lo, q, (uint32_t)(su >> 32) ^ hi}, k0, k1);
  u32x4 ws[5];
#pragma unroll
  for (int c = 0; c < 5; ++c)
    ws[c] = u32x4{(uint32_t)__builtin_amdgcn_readlane((int)w.x, c), (uint32_t)__builtin_amdgcn_readlane((int)w.y, c),
                  (uint32_t)__builtin_amdgcn_readlane((int)w.z, c), (uint32_t)__builtin_amdgcn_readlane((int)w.w, c)};
  return gc_chain(buf, cfg, ws[0], ws[1], ws[2], ws[3], ws[4], v_log_q, a_log_q);
}

// GCDataset.sample with look-ahead (one sample per workgroup, Philox draws):
// the selectors of this call come from ahead_in (stored by the previous
// call's launch; NULL: computed here first), and while waves 1..3 gather the
// rows, the first wave computes the NEXT call's selectors (call next_lo/hi)
// into ahead_out.  The draw chain of a call is thereby off its own critical
// path.  Words per sample (kGcAheadWords): idx, next, value goal, actor goal,
// mask, reward.  kHit (ahead_in valid) and the miss form (ahead_in ignored)
// are separate kernels: one kernel holding both paths spilled kernel
// arguments to VGPR lanes in a preamble every wave ran (HGC: 60 SGPR
// spills), and the hit path then measured 8.3 us against 6.4 us alone.
constexpr int kGcAheadWords = OGBX_GC_AHEAD_WORDS;
constexpr int64_t kGcAheadMaxSamples = 1024;

template <bool kHit, class Cols = GcColumns>
__global__ void __launch_bounds__(256) gc_ahead_kernel(
    ogbx_gc_buffer buf, ogbx_gc_config cfg, Cols cols, int32_t num_cols, uint32_t k0, uint32_t k1,
    uint32_t call_lo, uint32_t call_hi, uint32_t next_lo, uint32_t next_hi, double v_log_q, double a_log_q,
    const int64_t* __restrict__ ahead_in, int64_t* __restrict__ ahead_out, int64_t* idxs_out, int64_t* vgoal_out,
    int64_t* agoal_out, double* masks, double* rewards, bool flat4) {
  __shared__ int64_t sel[4][kGcMaxTile];
  const int64_t s = xcd_tile();
  const int t = (int)threadIdx.x;
  auto publish = [&](const GcPick& p) {
    sel[0][0] = p.idx;
    sel[1][0] = p.next;
    sel[2][0] = p.vg;
    sel[3][0] = p.ag;
    if (idxs_out) idxs_out[s] = p.idx;
    if (vgoal_out) vgoal_out[s] = p.vg;
    if (agoal_out) agoal_out[s] = p.ag;
    masks[s] = p.mask;
    rewards[s] = p.reward;
  };
  if constexpr (kHit) {
    // Hit: no block barrier.  The first wave runs the next call's chain from
    // the kernel's first instruction and writes this call's scalar outputs
    // from the record after it (a gathering wave that stored them would wait
    // for their write acknowledgements at its first row use: vmcnt counts
    // stores); each gathering wave reads the record's selectors into its own
    // LDS column (sel[.][wave]: written and read by the same wave, whose LDS
    // operations complete in order), so the gather waits for one record load
    // and never for the chain.
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    if (wave == 0) {
      const int64_t v = lane < 6 ? ahead_in[s * kGcAheadWords + lane] : 0;
      if (ahead_out) {
        const GcPick p = gc_wave_chain(buf, cfg, s, next_lo, next_hi, k0, k1, v_log_q, a_log_q);
        if (t == 0) {
          longlong2* o = reinterpret_cast<longlong2*>(ahead_out + s * kGcAheadWords);
          o[0] = make_longlong2(p.idx, p.next);
          o[1] = make_longlong2(p.vg, p.ag);
          o[2] = make_longlong2(__double_as_longlong(p.mask), __double_as_longlong(p.reward));
        }
      }
      if (lane == 0 && idxs_out) idxs_out[s] = v;
      if (lane == 2 && vgoal_out) vgoal_out[s] = v;
      if (lane == 3 && agoal_out) agoal_out[s] = v;
      if (lane == 4) masks[s] = __longlong_as_double(v);
      if (lane == 5) rewards[s] = __longlong_as_double(v);
      return;
    }
    if (lane < 4) sel[lane][wave] = ahead_in[s * kGcAheadWords + lane];
    __builtin_amdgcn_wave_barrier();
    copy_tile<0>(cols, num_cols, reinterpret_cast<const int64_t(*)[kGcMaxTile]>(&sel[0][wave]), s, 1, flat4, 1);
    return;
  }
  if (t < 64) {
    const GcPick p = gc_wave_chain(buf, cfg, s, call_lo, call_hi, k0, k1, v_log_q, a_log_q);
    if (t == 0) publish(p);
  }
  __syncthreads();
  if (ahead_out && t < 64) {
    const GcPick p = gc_wave_chain(buf, cfg, s, next_lo, next_hi, k0, k1, v_log_q, a_log_q);
    if (t == 0) {
      longlong2* o = reinterpret_cast<longlong2*>(ahead_out + s * kGcAheadWords);
      o[0] = make_longlong2(p.idx, p.next);
      o[1] = make_longlong2(p.vg, p.ag);
      o[2] = make_longlong2(__double_as_longlong(p.mask), __double_as_longlong(p.reward));
    }
  } else {
    copy_tile<0>(cols, num_cols, sel, s, 1, flat4, ahead_out ? 1 : 0);
  }
}

// high_next (compute_high_next_idxs) and kHgcSel: gc_select.h

// HGCDataset.sample (datasets.py:496-643): same tile structure as
// gc_sample_kernel with ten row selectors and the hierarchical scalars.
template <bool kInj>
__global__ void __launch_bounds__(256) hgc_sample_kernel(
    ogbx_gc_buffer buf, ogbx_gc_config cfg, ogbx_hgc_config hc, GcColumns cols, int32_t num_cols,
    int64_t total, int tile, ogbx_hgc_draws dr, uint32_t k0, uint32_t k1, uint32_t call_lo,
    uint32_t call_hi, double v_log_q, double a_log_q, double l_log_q, ogbx_hgc_outputs o,
    ogbx_hgc_draw_record rec, bool flat4) {
  __shared__ int64_t sel[kHgcSel][kGcMaxTile];
  __shared__ uint4 wb[(!kInj && kGcSpread) ? 7 : 1][kGcMaxTile];
  const int64_t base = xcd_tile() * tile;
  const int n_here = (int)((total - base) < tile ? (total - base) : tile);
  if (!kInj && kGcSpread) {
    tile_philox(wb, hc.has_low_value_goals ? 7 : 5, n_here, base, call_lo, call_hi, k0, k1);
    __syncthreads();
  }
  if (threadIdx.x < 64 && n_here > 0) {  // the whole first wave: see gc_sample_kernel
    const int b = (int)threadIdx.x % n_here;
    const bool own = (int)threadIdx.x < n_here;
    const int64_t s = base + b;
    const uint64_t su = (uint64_t)s;
    const uint32_t c0 = (uint32_t)su, c3 = (uint32_t)(su >> 32) ^ call_hi;
    u32x4 w0, w1, w2, w3, w4;
    if (!kInj && kGcSpread) {
      w0 = tile_word(wb, 0, b), w1 = tile_word(wb, 1, b), w2 = tile_word(wb, 2, b), w3 = tile_word(wb, 3, b),
      w4 = tile_word(wb, 4, b);
    } else {
      w0 = philox4x32_10({c0, call_lo, 0u, c3}, k0, k1);
      w1 = philox4x32_10({c0, call_lo, 1u, c3}, k0, k1);
      w2 = philox4x32_10({c0, call_lo, 2u, c3}, k0, k1);
      w3 = philox4x32_10({c0, call_lo, 3u, c3}, k0, k1);
      w4 = philox4x32_10({c0, call_lo, 4u, c3}, k0, k1);
    }
    const int64_t npick = buf.valid_idxs ? buf.num_valid : buf.num_rows;
    const ogbx_gc_draws& g = dr.gc;
    int64_t idx = 0, pick, fin;
    GoalDraws v, a, l;
    root_picks<kInj, false>(g, s, w0, w1, npick, buf.num_rows, &idx, &pick, &v.pick, &a.pick);
    u32x4 w5{}, w6{};
    int64_t l_rand = 0;
    if (hc.has_low_value_goals) {
      if (!kInj && kGcSpread) {
        w5 = tile_word(wb, 5, b);
        w6 = tile_word(wb, 6, b);
      } else {
        w5 = philox4x32_10({c0, call_lo, 5u, c3}, k0, k1);
        w6 = philox4x32_10({c0, call_lo, 6u, c3}, k0, k1);
      }
      l.pick = (kInj && dr.l_pick) ? dr.l_pick[s] : (int64_t)bounded64(w5.x, w5.y, (uint64_t)npick);
    }
    index_loads(buf, kInj && g.idxs != nullptr, pick, &idx, &fin);
    const int64_t v_rand = cfg.value_cur_is_one ? 0 : rand_goal_of(buf, v.pick);
    const int64_t a_rand = cfg.actor_cur_is_one ? 0 : rand_goal_of(buf, a.pick);
    if (hc.has_low_value_goals && !cfg.value_cur_is_one) l_rand = rand_goal_of(buf, l.pick);
    const int64_t next = idx + 1 < buf.num_rows ? idx + 1 : buf.num_rows - 1;
    // written out, not goal_side_draws: the helper moves this kernel's code (gc_device.h)
    const double uvg = u01_from(w1.z, w1.w), uag = u01_from(w2.x, w2.y);
    v.geom = (kInj && g.v_geom) ? g.v_geom[s] : (cfg.value_geom_sample ? geometric_from(uvg, v_log_q) : 0);
    a.geom = (kInj && g.a_geom) ? g.a_geom[s] : (cfg.actor_geom_sample ? geometric_from(uag, a_log_q) : 0);
    v.dist = (kInj && g.v_dist) ? g.v_dist[s] : uvg;
    a.dist = (kInj && g.a_dist) ? g.a_dist[s] : uag;
    v.u_traj = (kInj && g.v_u_traj) ? g.v_u_traj[s] : u01_from(w2.z, w2.w);
    v.u_cur = (kInj && g.v_u_cur) ? g.v_u_cur[s] : u01_from(w3.x, w3.y);
    a.u_traj = (kInj && g.a_u_traj) ? g.a_u_traj[s] : u01_from(w3.z, w3.w);
    a.u_cur = (kInj && g.a_u_cur) ? g.a_u_cur[s] : u01_from(w4.x, w4.y);
    const int64_t hvg = sample_goal(idx, fin, v, v_rand, cfg.value_p_curgoal, cfg.value_traj_thresh,
                                    cfg.value_geom_sample, cfg.value_cur_is_one);
    const int64_t hag = sample_goal(idx, fin, a, a_rand, cfg.actor_p_curgoal, cfg.actor_traj_thresh,
                                    cfg.actor_geom_sample, cfg.actor_cur_is_one);
    int64_t lvg = idx;
    if (hc.has_low_value_goals) {
      l.geom = (kInj && dr.l_geom) ? dr.l_geom[s] : geometric_from(u01_from(w5.z, w5.w), l_log_q);
      l.dist = 0.0;
      l.u_traj = (kInj && dr.l_u_traj) ? dr.l_u_traj[s] : u01_from(w6.x, w6.y);
      l.u_cur = (kInj && dr.l_u_cur) ? dr.l_u_cur[s] : u01_from(w6.z, w6.w);
      lvg = sample_goal(idx, fin, l, l_rand, cfg.value_p_curgoal, cfg.value_traj_thresh, 1,
                        cfg.value_cur_is_one);
      if (rec.l_pick && own) {
        rec.l_pick[s] = l.pick;
        rec.l_geom[s] = l.geom;
        rec.l_u_traj[s] = l.u_traj;
        rec.l_u_cur[s] = l.u_cur;
      }
    }
    int64_t hv_next, hv_steps, lv_next, lv_steps, ha_next, ha_steps, la_next, la_steps;
    high_next(idx, fin, hvg, hc.value_subgoal_steps, &hv_next, &hv_steps);
    high_next(idx, fin, hvg, hc.low_subgoal_steps, &lv_next, &lv_steps);
    high_next(idx, fin, hag, hc.actor_subgoal_steps, &ha_next, &ha_steps);
    const int64_t la_goal = idx + hc.actor_subgoal_steps < fin ? idx + hc.actor_subgoal_steps : fin;
    high_next(idx, fin, hag, hc.low_subgoal_steps, &la_next, &la_steps);
    if (own) {
    const int t = b;
    sel[0][t] = idx;
    sel[1][t] = next;
    sel[2][t] = hvg;
    sel[3][t] = hag;
    sel[4][t] = hv_next;
    sel[5][t] = lv_next;
    sel[6][t] = lvg;
    sel[7][t] = ha_next;
    sel[8][t] = la_goal;
    sel[9][t] = la_next;
    if (o.idxs) o.idxs[s] = idx;
    if (o.high_value_goal_idxs) o.high_value_goal_idxs[s] = hvg;
    if (o.high_actor_goal_idxs) o.high_actor_goal_idxs[s] = hag;
    if (o.low_value_goal_idxs) o.low_value_goal_idxs[s] = lvg;
    const double neg = cfg.gc_negative ? 1.0 : 0.0;
    o.high_value_offsets[s] = hvg - idx;
    o.high_value_subgoal_steps[s] = hv_steps;
    o.high_value_masks[s] = hc.hv_mask_table[hv_steps];
    o.high_value_rewards[s] = hc.hv_reward_table[hv_steps];
    o.low_value_subgoal_steps[s] = lv_steps;
    if (hc.has_low_value_goals) {
      const double ls = idx == lvg ? 1.0 : 0.0;
      o.low_value_masks[s] = 1.0 - ls;
      o.low_value_rewards[s] = ls - neg;
    } else {
      o.low_value_masks[s] = hc.lv_mask_table[lv_steps];
      o.low_value_rewards[s] = hc.lv_reward_table[lv_steps];
    }
    const double succ = idx == hvg ? 1.0 : 0.0;
    o.masks[s] = 1.0 - succ;
    o.rewards[s] = succ - neg;
    store_draw_record(rec.gc, s, pick, v, a);
    }  // own
  }
  __syncthreads();
  copy_tile<0>(cols, num_cols, sel, base, n_here, flat4);
}

// HGC look-ahead: one sample's ten selectors and nine scalar outputs (the
// order of ogbx_hgc_outputs from high_value_offsets on), as hgc_sample_kernel's
// Philox path computes them.
struct HgcPick {
  int64_t sel[kHgcSel];
  int64_t w[9];  // offsets, hv steps, hv mask, hv reward, lv steps, lv mask, lv reward, mask, reward (f64 as bits)
};

// The HGC reward tables held in the first wave's registers: lane t holds
// entries t and t + 64 of the value / low tables (loaded when the chain
// starts, so they arrive while it runs), and the chain's lookups are lane
// reads instead of global loads that wait for the subgoal step counts.  Valid when both tables have at most 128 entries (subgoal
// steps <= 127).  The mask tables are held the same way (the caller's tables,
// not 1 - (s < K) recomputed, so a C-ABI host's own tables give the same
// result as the direct ogbx_hgc_sample).
struct HgcTables {
  double hv0, hv1, lv0, lv1, hm0, hm1, lm0, lm1;
  bool regs;
};

__device__ __forceinline__ HgcTables hgc_tables_load(const ogbx_hgc_config& hc) {
  HgcTables tb{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, hc.value_subgoal_steps < 128 && hc.low_subgoal_steps < 128};
  const int t = (int)(threadIdx.x & 63);
  // clamped indices, every lane, no branch (a region around the loads made
  // the compiler wait for them at its end); entries past K are never looked
  // up, and with K >= 128 the lookups read the tables in memory instead
  const int64_t kv = hc.value_subgoal_steps, kl = hc.low_subgoal_steps;
  tb.hv0 = hc.hv_reward_table[min((int64_t)t, kv)];
  tb.hv1 = hc.hv_reward_table[min((int64_t)t + 64, kv)];
  tb.lv0 = hc.lv_reward_table[min((int64_t)t, kl)];
  tb.lv1 = hc.lv_reward_table[min((int64_t)t + 64, kl)];
  tb.hm0 = hc.hv_mask_table[min((int64_t)t, kv)];
  tb.hm1 = hc.hv_mask_table[min((int64_t)t + 64, kv)];
  tb.lm0 = hc.lv_mask_table[min((int64_t)t, kl)];
  tb.lm1 = hc.lv_mask_table[min((int64_t)t + 64, kl)];
  return tb;
}

// entry s (wave-uniform) of a register-held table
__device__ __forceinline__ double table_lane(double v0, double v1, int64_t s) {
  const int i = __builtin_amdgcn_readfirstlane((int)s);
  const double v = i < 64 ? v0 : v1;
  const int l = i & 63;
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

__device__ inline HgcPick hgc_chain(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg, const ogbx_hgc_config& hc,
                                    const u32x4* wv, double v_log_q, double a_log_q, double l_log_q,
                                    const HgcTables& tb) {
  const u32x4 w0 = wv[0], w1 = wv[1], w2 = wv[2], w3 = wv[3], w4 = wv[4];
  const int64_t npick = buf.valid_idxs ? buf.num_valid : buf.num_rows;
  const int64_t pick = (int64_t)bounded64(w0.x, w0.y, (uint64_t)npick);
  GoalDraws v, a, l;
  v.pick = (int64_t)bounded64(w0.z, w0.w, (uint64_t)npick);
  a.pick = (int64_t)bounded64(w1.x, w1.y, (uint64_t)npick);
  u32x4 w5{}, w6{};
  int64_t l_rand = 0;
  if (hc.has_low_value_goals) {
    w5 = wv[5];
    w6 = wv[6];
    l.pick = (int64_t)bounded64(w5.x, w5.y, (uint64_t)npick);
  }
  int64_t idx = 0, fin;
  index_loads(buf, false, pick, &idx, &fin);
  const int64_t v_rand = cfg.value_cur_is_one ? 0 : rand_goal_of(buf, v.pick);
  const int64_t a_rand = cfg.actor_cur_is_one ? 0 : rand_goal_of(buf, a.pick);
  if (hc.has_low_value_goals && !cfg.value_cur_is_one) l_rand = rand_goal_of(buf, l.pick);
  const int64_t next = idx + 1 < buf.num_rows ? idx + 1 : buf.num_rows - 1;
  goal_side_draws<false>(ogbx_gc_draws{}, cfg, 0, w1, w2, w3, w4, v_log_q, a_log_q, v, a);
  const int64_t hvg = sample_goal(idx, fin, v, v_rand, cfg.value_p_curgoal, cfg.value_traj_thresh,
                                  cfg.value_geom_sample, cfg.value_cur_is_one);
  const int64_t hag = sample_goal(idx, fin, a, a_rand, cfg.actor_p_curgoal, cfg.actor_traj_thresh,
                                  cfg.actor_geom_sample, cfg.actor_cur_is_one);
  int64_t lvg = idx;
  if (hc.has_low_value_goals) {
    l.geom = geometric_from(u01_from(w5.z, w5.w), l_log_q);
    l.dist = 0.0;
    l.u_traj = u01_from(w6.x, w6.y);
    l.u_cur = u01_from(w6.z, w6.w);
    lvg = sample_goal(idx, fin, l, l_rand, cfg.value_p_curgoal, cfg.value_traj_thresh, 1, cfg.value_cur_is_one);
  }
  int64_t hv_next, hv_steps, lv_next, lv_steps, ha_next, ha_steps, la_next, la_steps;
  high_next(idx, fin, hvg, hc.value_subgoal_steps, &hv_next, &hv_steps);
  high_next(idx, fin, hvg, hc.low_subgoal_steps, &lv_next, &lv_steps);
  high_next(idx, fin, hag, hc.actor_subgoal_steps, &ha_next, &ha_steps);
  const int64_t la_goal = idx + hc.actor_subgoal_steps < fin ? idx + hc.actor_subgoal_steps : fin;
  high_next(idx, fin, hag, hc.low_subgoal_steps, &la_next, &la_steps);
  HgcPick p;
  p.sel[0] = idx;
  p.sel[1] = next;
  p.sel[2] = hvg;
  p.sel[3] = hag;
  p.sel[4] = hv_next;
  p.sel[5] = lv_next;
  p.sel[6] = lvg;
  p.sel[7] = ha_next;
  p.sel[8] = la_goal;
  p.sel[9] = la_next;
  const double neg = cfg.gc_negative ? 1.0 : 0.0;
  p.w[0] = hvg - idx;
  p.w[1] = hv_steps;
  if (tb.regs) {
    p.w[2] = __double_as_longlong(table_lane(tb.hm0, tb.hm1, hv_steps));
    p.w[3] = __double_as_longlong(table_lane(tb.hv0, tb.hv1, hv_steps));
  } else {
    p.w[2] = __double_as_longlong(hc.hv_mask_table[hv_steps]);
    p.w[3] = __double_as_longlong(hc.hv_reward_table[hv_steps]);
  }
  p.w[4] = lv_steps;
  if (hc.has_low_value_goals) {
    const double ls = idx == lvg ? 1.0 : 0.0;
    p.w[5] = __double_as_longlong(1.0 - ls);
    p.w[6] = __double_as_longlong(ls - neg);
  } else if (tb.regs) {
    p.w[5] = __double_as_longlong(table_lane(tb.lm0, tb.lm1, lv_steps));
    p.w[6] = __double_as_longlong(table_lane(tb.lv0, tb.lv1, lv_steps));
  } else {
    p.w[5] = __double_as_longlong(hc.lv_mask_table[lv_steps]);
    p.w[6] = __double_as_longlong(hc.lv_reward_table[lv_steps]);
  }
  const double succ = idx == hvg ? 1.0 : 0.0;
  p.w[7] = __double_as_longlong(1.0 - succ);
  p.w[8] = __double_as_longlong(succ - neg);
  return p;
}

__device__ inline HgcPick hgc_wave_chain(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg,
                                         const ogbx_hgc_config& hc, int64_t s, uint32_t lo, uint32_t hi, uint32_t k0,
                                         uint32_t k1, double v_log_q, double a_log_q, double l_log_q) {
  // the reward tables: issued first, they arrive while the Philox calls and
  // the goal chain run (their lookups come last)
  const HgcTables tb = hgc_tables_load(hc);
  const uint64_t su = (uint64_t)s;
  const uint32_t calls = hc.has_low_value_goals ? 7u : 5u;
  const uint32_t q = (uint32_t)(threadIdx.x & 63) % calls;
  const u32x4 w = philox4x32_10({(uint32_t)su, lo, q, (uint32_t)(su >> 32) ^ hi}, k0, k1);
  u32x4 ws[7];
#pragma unroll
  for (int c = 0; c < 7; ++c)
    ws[c] = u32x4{(uint32_t)__builtin_amdgcn_readlane((int)w.x, c), (uint32_t)__builtin_amdgcn_readlane((int)w.y, c),
                  (uint32_t)__builtin_amdgcn_readlane((int)w.z, c), (uint32_t)__builtin_amdgcn_readlane((int)w.w, c)};
  return hgc_chain(buf, cfg, hc, ws, v_log_q, a_log_q, l_log_q, tb);
}

constexpr int kHgcAheadWords = OGBX_HGC_AHEAD_WORDS;
static_assert(kHgcAheadWords >= kHgcSel + 9, "HGC look-ahead record: 10 selectors + 9 scalars");

// HGCDataset.sample with look-ahead (gc_ahead_kernel's scheme).
template <bool kHit, class Cols = GcColumns>
__global__ void __launch_bounds__(256) hgc_ahead_kernel(
    ogbx_gc_buffer buf, ogbx_gc_config cfg, ogbx_hgc_config hc, Cols cols, int32_t num_cols, uint32_t k0,
    uint32_t k1, uint32_t call_lo, uint32_t call_hi, uint32_t next_lo, uint32_t next_hi, double v_log_q,
    double a_log_q, double l_log_q, const int64_t* __restrict__ ahead_in, int64_t* __restrict__ ahead_out,
    ogbx_hgc_outputs o, bool flat4) {
  __shared__ int64_t sel[kHgcSel][kGcMaxTile];
  const int64_t s = xcd_tile();
  const int t = (int)threadIdx.x;
  // scalar word j (0..8) of a record -> its output (static j: no pointer array)
  auto put_scalar = [&](int j, int64_t v) {
    switch (j) {
      case 0: o.high_value_offsets[s] = v; break;
      case 1: o.high_value_subgoal_steps[s] = v; break;
      case 2: o.high_value_masks[s] = __longlong_as_double(v); break;
      case 3: o.high_value_rewards[s] = __longlong_as_double(v); break;
      case 4: o.low_value_subgoal_steps[s] = v; break;
      case 5: o.low_value_masks[s] = __longlong_as_double(v); break;
      case 6: o.low_value_rewards[s] = __longlong_as_double(v); break;
      case 7: o.masks[s] = __longlong_as_double(v); break;
      default: o.rewards[s] = __longlong_as_double(v); break;
    }
  };
  auto put_index = [&](int k, int64_t v) {
    if (k == 0 && o.idxs) o.idxs[s] = v;
    if (k == 2 && o.high_value_goal_idxs) o.high_value_goal_idxs[s] = v;
    if (k == 3 && o.high_actor_goal_idxs) o.high_actor_goal_idxs[s] = v;
    if (k == 6 && o.low_value_goal_idxs) o.low_value_goal_idxs[s] = v;
  };
  if constexpr (kHit) {
    // Hit: no block barrier (gc_ahead_kernel's scheme)
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    if (wave == 0) {
      const int64_t v = lane < kHgcSel + 9 ? ahead_in[s * kHgcAheadWords + lane] : 0;
      if (ahead_out) {
        const HgcPick p = hgc_wave_chain(buf, cfg, hc, s, next_lo, next_hi, k0, k1, v_log_q, a_log_q, l_log_q);
        if (t == 0) {
          int64_t* r = ahead_out + s * kHgcAheadWords;
#pragma unroll
          for (int k = 0; k < kHgcSel; ++k) r[k] = p.sel[k];
#pragma unroll
          for (int j = 0; j < 9; ++j) r[kHgcSel + j] = p.w[j];
        }
      }
      if (lane < kHgcSel)
        put_index(lane, v);
      else if (lane < kHgcSel + 9)
        put_scalar(lane - kHgcSel, v);
      return;
    }
    if (lane < kHgcSel) sel[lane][wave] = ahead_in[s * kHgcAheadWords + lane];
    __builtin_amdgcn_wave_barrier();
    copy_tile<0, true>(cols, num_cols, reinterpret_cast<const int64_t(*)[kGcMaxTile]>(&sel[0][wave]), s, 1, flat4, 1);
    return;
  }
  if (t < 64) {
    const HgcPick p = hgc_wave_chain(buf, cfg, hc, s, call_lo, call_hi, k0, k1, v_log_q, a_log_q, l_log_q);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < kHgcSel; ++k) {
        sel[k][0] = p.sel[k];
        put_index(k, p.sel[k]);
      }
#pragma unroll
      for (int j = 0; j < 9; ++j) put_scalar(j, p.w[j]);
    }
  }
  __syncthreads();
  if (ahead_out && t < 64) {
    const HgcPick p = hgc_wave_chain(buf, cfg, hc, s, next_lo, next_hi, k0, k1, v_log_q, a_log_q, l_log_q);
    if (t == 0) {
      int64_t* r = ahead_out + s * kHgcAheadWords;
#pragma unroll
      for (int k = 0; k < kHgcSel; ++k) r[k] = p.sel[k];
#pragma unroll
      for (int j = 0; j < 9; ++j) r[kHgcSel + j] = p.w[j];
    }
  } else {
    copy_tile<0>(cols, num_cols, sel, s, 1, flat4, ahead_out ? 1 : 0);
  }
}

__global__ void traj_end_kernel(const int64_t* __restrict__ term, int64_t nterm, int64_t nrows,
                                int64_t* __restrict__ out) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  // searchsorted(term, r, side='left'): first position with term[pos] >= r
  int64_t lo = 0, hi = nterm;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (term[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  out[r] = lo < nterm ? term[lo] : term[nterm - 1];
}

struct PositiveF32 {
  const float* x;
  __device__ bool operator()(const int64_t& i) const { return x[i] > 0.0f; }
};

}  // namespace ogbx

using namespace ogbx;

// The look-ahead kernels run one sample per workgroup and read one selector
// buffer while they write the other.
static ogbx_status check_ahead(int64_t total, const int64_t* ahead_in, const int64_t* ahead_out, const char* who) {
  OGBX_CHECK(total <= kGcAheadMaxSamples, OGBX_EINVAL,
             named(who, "at most 1024 samples per call (one per workgroup)"));
  OGBX_CHECK(ahead_in != ahead_out || ahead_in == nullptr, OGBX_EINVAL,
             named(who, "ahead_in and ahead_out must differ"));
  return OGBX_OK;
}

// GC per-sample scalar outputs (the index outputs may be NULL).
struct GcScalars {
  int64_t *idxs = nullptr, *vg = nullptr, *ag = nullptr;
  double *masks = nullptr, *rewards = nullptr;
};

// ------------------------------------------------------------------ launches
// The only launch site of each kernel: the one-shot entry points and the
// sampler plan both come through here.  flat4 = flat4_columns() of the table.
static ogbx_status launch_gc_sample(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg, const GcParams& pr,
                                    const GcColumns& cc, int32_t num_cols, bool flat4, int64_t total,
                                    uint64_t call, const ogbx_gc_draws& dr, const ogbx_gc_draw_record& rec,
                                    const GcScalars& o, hipStream_t s) {
  int64_t tile, blocks;
  sample_grid(total, &tile, &blocks);
  const auto kern = any_draw(dr) ? gc_sample_kernel<true> : gc_sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, s, buf, cfg, cc, num_cols, total, (int)tile, dr,
                     pr.k0, pr.k1, (uint32_t)call, (uint32_t)(call >> 32), pr.v_log_q, pr.a_log_q, o.idxs, o.vg,
                     o.ag, o.masks, o.rewards, rec, tile <= 4 && flat4);
  OGBX_LAUNCHED("gc_sample_kernel");
  return OGBX_OK;
}

static ogbx_status launch_hgc_sample(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg,
                                     const ogbx_hgc_config& hcfg, const GcParams& pr, const GcColumns& cc,
                                     int32_t num_cols, bool flat4, int64_t total, uint64_t call,
                                     const ogbx_hgc_draws& dr, const ogbx_hgc_draw_record& rec,
                                     const ogbx_hgc_outputs& o, hipStream_t s) {
  int64_t tile, blocks;
  sample_grid(total, &tile, &blocks);
  const bool inj = any_draw(dr.gc) || dr.l_pick || dr.l_geom || dr.l_u_traj || dr.l_u_cur;
  const auto kern = inj ? hgc_sample_kernel<true> : hgc_sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, s, buf, cfg, hcfg, cc, num_cols, total, (int)tile,
                     dr, pr.k0, pr.k1, (uint32_t)call, (uint32_t)(call >> 32), pr.v_log_q, pr.a_log_q, pr.l_log_q,
                     o, rec, tile <= 4 && flat4);
  OGBX_LAUNCHED("hgc_sample_kernel");
  return OGBX_OK;
}

// Cols: GcColumns, or a plan's GcColumnsSmall image of at most 16 columns.
// One workgroup per sample; `call + 1`'s selectors go to ahead_out.
template <class Cols>
static ogbx_status launch_gc_ahead(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg, const GcParams& pr,
                                   const Cols& cols, int32_t num_cols, bool flat4, int64_t total, uint64_t call,
                                   const int64_t* ahead_in, int64_t* ahead_out, const GcScalars& o,
                                   hipStream_t s) {
  const uint64_t next = call + 1;
  const auto kern = ahead_in ? gc_ahead_kernel<true, Cols> : gc_ahead_kernel<false, Cols>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)total), dim3(256), 0, s, buf, cfg, cols, num_cols, pr.k0, pr.k1,
                     (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)next, (uint32_t)(next >> 32), pr.v_log_q,
                     pr.a_log_q, ahead_in, ahead_out, o.idxs, o.vg, o.ag, o.masks, o.rewards, flat4);
  OGBX_LAUNCHED("gc_ahead_kernel");
  return OGBX_OK;
}

template <class Cols>
static ogbx_status launch_hgc_ahead(const ogbx_gc_buffer& buf, const ogbx_gc_config& cfg,
                                    const ogbx_hgc_config& hcfg, const GcParams& pr, const Cols& cols,
                                    int32_t num_cols, bool flat4, int64_t total, uint64_t call,
                                    const int64_t* ahead_in, int64_t* ahead_out, const ogbx_hgc_outputs& o,
                                    hipStream_t s) {
  const uint64_t next = call + 1;
  const auto kern = ahead_in ? hgc_ahead_kernel<true, Cols> : hgc_ahead_kernel<false, Cols>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)total), dim3(256), 0, s, buf, cfg, hcfg, cols, num_cols, pr.k0, pr.k1,
                     (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)next, (uint32_t)(next >> 32), pr.v_log_q,
                     pr.a_log_q, pr.l_log_q, ahead_in, ahead_out, o, flat4);
  OGBX_LAUNCHED("hgc_ahead_kernel");
  return OGBX_OK;
}

extern "C" {

ogbx_status ogbx_gc_sample(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                           const ogbx_gc_column* cols, int32_t num_cols, int64_t batch,
                           int64_t num_batches, const ogbx_gc_draws* draws, uint64_t seed,
                           uint64_t call_index, int64_t* idxs_out, int64_t* value_goal_out,
                           int64_t* actor_goal_out, double* masks, double* rewards,
                           const ogbx_gc_draw_record* record, void* stream) {
  const char* who = "ogbx_gc_sample";
  OGBX_CHECK(buf && cfg && masks && rewards, OGBX_EINVAL, named(who, "null argument"));
  GcColumns cc{};
  bool flat4;
  GC_TRY(check_columns(cols, num_cols, batch, num_batches, 3, who, &cc, &flat4));
  GC_TRY(check_buffer(buf));
  return launch_gc_sample(*buf, *cfg, gc_params(seed, *cfg, nullptr), cc, num_cols, flat4,
                          batch * num_batches, call_index, draws ? *draws : ogbx_gc_draws{},
                          record ? *record : ogbx_gc_draw_record{},
                          {idxs_out, value_goal_out, actor_goal_out, masks, rewards}, (hipStream_t)stream);
}

ogbx_status ogbx_gc_sample_ahead(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                                 const ogbx_gc_column* cols, int32_t num_cols, int64_t batch,
                                 int64_t num_batches, uint64_t seed, uint64_t call_index,
                                 const int64_t* ahead_in, int64_t* ahead_out, int64_t* idxs_out,
                                 int64_t* value_goal_out, int64_t* actor_goal_out, double* masks,
                                 double* rewards, void* stream) {
  const char* who = "ogbx_gc_sample_ahead";
  OGBX_CHECK(buf && cfg && masks && rewards, OGBX_EINVAL, named(who, "null argument"));
  GcColumns cc{};
  bool flat4;
  GC_TRY(check_columns(cols, num_cols, batch, num_batches, 3, who, &cc, &flat4));
  GC_TRY(check_ahead(batch * num_batches, ahead_in, ahead_out, who));
  GC_TRY(check_buffer(buf));
  return launch_gc_ahead(*buf, *cfg, gc_params(seed, *cfg, nullptr), cc, num_cols, flat4,
                         batch * num_batches, call_index, ahead_in, ahead_out,
                         {idxs_out, value_goal_out, actor_goal_out, masks, rewards}, (hipStream_t)stream);
}

ogbx_status ogbx_hgc_sample(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                            const ogbx_hgc_config* hcfg, const ogbx_gc_column* cols,
                            int32_t num_cols, int64_t batch, int64_t num_batches,
                            const ogbx_hgc_draws* draws, uint64_t seed, uint64_t call_index,
                            const ogbx_hgc_outputs* out, const ogbx_hgc_draw_record* record,
                            void* stream) {
  const char* who = "ogbx_hgc_sample";
  OGBX_CHECK(buf && cfg && hcfg && out, OGBX_EINVAL, named(who, "null argument"));
  GcColumns cc{};
  bool flat4;
  GC_TRY(check_hgc_outputs(out, who));
  GC_TRY(check_hgc_config(hcfg, who, 0, "negative subgoal steps"));
  GC_TRY(check_columns(cols, num_cols, batch, num_batches, kHgcSel - 1, who, &cc, &flat4));
  GC_TRY(check_buffer(buf));
  return launch_hgc_sample(*buf, *cfg, *hcfg, gc_params(seed, *cfg, hcfg), cc, num_cols,
                           flat4, batch * num_batches, call_index,
                           draws ? *draws : ogbx_hgc_draws{}, record ? *record : ogbx_hgc_draw_record{}, *out,
                           (hipStream_t)stream);
}

ogbx_status ogbx_hgc_sample_ahead(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                                  const ogbx_hgc_config* hcfg, const ogbx_gc_column* cols, int32_t num_cols,
                                  int64_t batch, int64_t num_batches, uint64_t seed, uint64_t call_index,
                                  const int64_t* ahead_in, int64_t* ahead_out, const ogbx_hgc_outputs* out,
                                  void* stream) {
  const char* who = "ogbx_hgc_sample_ahead";
  OGBX_CHECK(buf && cfg && hcfg && out, OGBX_EINVAL, named(who, "null argument"));
  GcColumns cc{};
  bool flat4;
  GC_TRY(check_hgc_outputs(out, who));
  GC_TRY(check_hgc_config(hcfg, who, 0, "negative subgoal steps"));
  GC_TRY(check_columns(cols, num_cols, batch, num_batches, kHgcSel - 1, who, &cc, &flat4));
  GC_TRY(check_ahead(batch * num_batches, ahead_in, ahead_out, who));
  GC_TRY(check_buffer(buf));
  return launch_hgc_ahead(*buf, *cfg, *hcfg, gc_params(seed, *cfg, hcfg), cc, num_cols,
                          flat4, batch * num_batches, call_index, ahead_in, ahead_out, *out,
                          (hipStream_t)stream);
}

}  // extern "C"

// ---------------------------------------------------------------- sampler plans
// A plan owns everything a steady stream of GCDataset / HGCDataset.sample
// calls repeats: the validated buffer and config, the Philox key, the
// geometric log terms, up to OGBX_GC_PLAN_SLOTS prepared output batches (the
// column descriptors as one kernel-argument image), and the look-ahead state:
// one pair of selector buffers per stream (allocated on the stream's first
// call, never shared across streams) and the (stream, samples, call) the
// last launch stored selectors for.  A call is then one lookup and one launch.
namespace {
constexpr int kPlanStreams = 8;

struct PlanBatch {
  bool set = false;
  GcColumns cc{};
  int32_t ncols = 0;
  int64_t total = 0;  // batch * num_batches
  GcScalars out{};
  ogbx_hgc_outputs hout{};
  bool flat4 = false;
  bool small = false;  // ncols <= kGcSmallCols: launch with cs
  GcColumnsSmall cs{};
};

struct PlanPair {
  void* stream = nullptr;
  int64_t* buf[2] = {nullptr, nullptr};
};
}  // namespace

struct ogbx_gc_plan_s {
  ogbx_gc_buffer buf;
  ogbx_gc_config cfg;
  ogbx_hgc_config hcfg;
  bool hgc = false, lookahead = true;
  int device = 0;
  GcParams pr;
  PlanBatch slots[OGBX_GC_PLAN_SLOTS];
  PlanPair pairs[kPlanStreams];
  int npairs = 0;
  // the selectors in pairs[key_pair].buf[key_which] belong to (key_total, key_call)
  bool key_valid = false;
  int key_pair = 0, key_which = 0;
  int64_t key_total = 0;
  uint64_t key_call = 0;
  int64_t hits = 0;
  // guards pairs / npairs / key_* / hits: ctypes releases the GIL, so two
  // host threads may call ogbx_gc_plan_sample on one plan (uncontended: ~20 ns)
  std::mutex mu;
};

extern "C" {

ogbx_status ogbx_gc_plan_create(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                                const ogbx_hgc_config* hcfg, uint64_t seed, int32_t lookahead,
                                ogbx_gc_plan_t* plan) {
  const char* who = "ogbx_gc_plan_create";
  OGBX_CHECK(buf && cfg && plan, OGBX_EINVAL, named(who, "null argument"));
  GC_TRY(check_buffer(buf));
  if (hcfg) GC_TRY(check_hgc_config(hcfg, who, 0, "negative subgoal steps"));
  auto* p = new (std::nothrow) ogbx_gc_plan_s();
  OGBX_CHECK(p, OGBX_ENOMEM, "ogbx_gc_plan_create: out of host memory");
  p->buf = *buf;
  p->cfg = *cfg;
  p->hgc = hcfg != nullptr;
  if (hcfg) p->hcfg = *hcfg;
  p->lookahead = lookahead != 0;
  // the plan's device is the buffer's, not whichever device is current: the
  // look-ahead selector pairs are allocated there on a stream's first call
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, buf->traj_end) == hipSuccess && attr.type == hipMemoryTypeDevice)
    p->device = attr.device;
  else if (hipGetDevice(&p->device) != hipSuccess)
    p->device = 0;
  p->pr = gc_params(seed, *cfg, hcfg);
  *plan = p;
  return OGBX_OK;
}

ogbx_status ogbx_gc_plan_set_batch(ogbx_gc_plan_t p, int32_t slot, const ogbx_gc_column* cols, int32_t num_cols,
                                   int64_t batch, int64_t num_batches, int64_t* idxs_out, int64_t* value_goal_out,
                                   int64_t* actor_goal_out, double* masks, double* rewards,
                                   const ogbx_hgc_outputs* hgc_out) {
  const char* who = "ogbx_gc_plan_set_batch";
  OGBX_CHECK(p, OGBX_EINVAL, "null plan");
  OGBX_CHECK(slot >= 0 && slot < OGBX_GC_PLAN_SLOTS, OGBX_EINVAL, named(who, "slot out of range"));
  PlanBatch b;
  GC_TRY(check_columns(cols, num_cols, batch, num_batches, p->hgc ? kHgcSel - 1 : 3, who, &b.cc, &b.flat4));
  if (p->hgc)
    GC_TRY(check_hgc_outputs(hgc_out, who));
  else
    OGBX_CHECK(masks && rewards, OGBX_EINVAL, named(who, "null masks / rewards"));
  b.ncols = num_cols;
  b.total = batch * num_batches;
  b.out = {idxs_out, value_goal_out, actor_goal_out, masks, rewards};
  if (hgc_out) b.hout = *hgc_out;
  b.small = num_cols <= kGcSmallCols;
  for (int i = 0; i < kGcSmallCols && i < num_cols; ++i) b.cs.c[i] = b.cc.c[i];
  b.set = true;
  std::lock_guard<std::mutex> guard(p->mu);
  p->slots[slot] = b;
  return OGBX_OK;
}

ogbx_status ogbx_gc_plan_sample(ogbx_gc_plan_t p, int32_t slot, uint64_t call_index, void* stream) {
  OGBX_CHECK(p, OGBX_EINVAL, "null plan");
  std::lock_guard<std::mutex> guard(p->mu);
  OGBX_CHECK(slot >= 0 && slot < OGBX_GC_PLAN_SLOTS && p->slots[slot].set, OGBX_EINVAL,
             "ogbx_gc_plan_sample: no batch in this slot");
  const PlanBatch& b = p->slots[slot];
  const int64_t total = b.total;
  hipStream_t s = (hipStream_t)stream;
  if (!p->lookahead || total > kGcAheadMaxSamples) {
    p->key_valid = false;
    if (p->hgc)
      return launch_hgc_sample(p->buf, p->cfg, p->hcfg, p->pr, b.cc, b.ncols, b.flat4, total, call_index,
                               ogbx_hgc_draws{}, ogbx_hgc_draw_record{}, b.hout, s);
    return launch_gc_sample(p->buf, p->cfg, p->pr, b.cc, b.ncols, b.flat4, total, call_index, ogbx_gc_draws{},
                            ogbx_gc_draw_record{}, b.out, s);
  }
  // this stream's buffer pair (allocated on its first call; with every pair
  // taken, the call runs without look-ahead: nothing stored, nothing read)
  int pi = -1;
  for (int i = 0; i < p->npairs; ++i)
    if (p->pairs[i].stream == stream) pi = i;
  if (pi < 0 && p->npairs < kPlanStreams) {
    const size_t words = (size_t)kGcAheadMaxSamples * (p->hgc ? kHgcAheadWords : kGcAheadWords);
    int cur = 0;
    OGBX_HIP(hipGetDevice(&cur));
    if (cur != p->device) OGBX_HIP(hipSetDevice(p->device));
    PlanPair pr;
    pr.stream = stream;
    hipError_t e0 = hipMalloc(&pr.buf[0], words * sizeof(int64_t));
    hipError_t e1 = e0 == hipSuccess ? hipMalloc(&pr.buf[1], words * sizeof(int64_t)) : e0;
    if (cur != p->device) (void)hipSetDevice(cur);
    if (e0 != hipSuccess || e1 != hipSuccess) {
      if (pr.buf[0]) (void)hipFree(pr.buf[0]);
      return hip_fail(e0 != hipSuccess ? e0 : e1, "hipMalloc (look-ahead buffers)");
    }
    pi = p->npairs++;
    p->pairs[pi] = pr;
  }
  const int64_t* in = nullptr;
  int64_t* out = nullptr;
  int which = 0;
  if (pi >= 0) {
    const bool hit = p->key_valid && p->key_pair == pi && p->key_total == total && p->key_call == call_index;
    if (hit) {
      in = p->pairs[pi].buf[p->key_which];
      which = 1 - p->key_which;
      ++p->hits;
    }
    out = p->pairs[pi].buf[which];
  }
  auto launch = [&](const auto& cols) {
    if (p->hgc)
      return launch_hgc_ahead(p->buf, p->cfg, p->hcfg, p->pr, cols, b.ncols, b.flat4, total, call_index, in, out,
                              b.hout, s);
    return launch_gc_ahead(p->buf, p->cfg, p->pr, cols, b.ncols, b.flat4, total, call_index, in, out, b.out, s);
  };
  GC_TRY(b.small ? launch(b.cs) : launch(b.cc));
  p->key_valid = pi >= 0;
  p->key_pair = pi;
  p->key_which = which;
  p->key_total = total;
  p->key_call = call_index + 1;
  return OGBX_OK;
}

int64_t ogbx_gc_plan_hits(ogbx_gc_plan_t p) {
  if (!p) return -1;
  std::lock_guard<std::mutex> guard(p->mu);
  return p->hits;
}

ogbx_status ogbx_gc_plan_destroy(ogbx_gc_plan_t p) {
  if (!p) return OGBX_OK;
  hipError_t err = hipSuccess;
  for (int i = 0; i < p->npairs; ++i)
    for (int k = 0; k < 2; ++k)
      if (p->pairs[i].buf[k]) {
        const hipError_t e = hipFree(p->pairs[i].buf[k]);  // waits for in-flight launches
        if (err == hipSuccess) err = e;
      }
  delete p;
  if (err != hipSuccess) return hip_fail(err, "hipFree (look-ahead buffers)");
  return OGBX_OK;
}

}  // extern "C"

extern "C" {

ogbx_status ogbx_gc_traj_end(const int64_t* terminal_locs, int64_t num_terminals,
                             int64_t num_rows, int64_t* traj_end, void* stream) {
  OGBX_CHECK(terminal_locs && traj_end && num_terminals > 0 && num_rows > 0, OGBX_EINVAL,
             "ogbx_gc_traj_end: bad argument");
  hipLaunchKernelGGL(traj_end_kernel, dim3((uint32_t)((num_rows + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, terminal_locs, num_terminals, num_rows, traj_end);
  OGBX_LAUNCHED("traj_end_kernel");
  return OGBX_OK;
}

ogbx_status ogbx_nonzero_f32(const float* x, int64_t n, int64_t* out, int64_t* count,
                             void* stream) {
  OGBX_CHECK(x && out && count && n >= 0, OGBX_EINVAL, "ogbx_nonzero_f32: bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipcub::CountingInputIterator<int64_t> it(0);
  PositiveF32 pred{x};
  size_t tmp_bytes = 0;
  OGBX_HIP(hipcub::DeviceSelect::If(nullptr, tmp_bytes, it, out, count, n, pred, s));
  void* tmp = nullptr;
  OGBX_HIP(hipMallocAsync(&tmp, tmp_bytes > 0 ? tmp_bytes : 1, s));
  hipError_t e = hipcub::DeviceSelect::If(tmp, tmp_bytes, it, out, count, n, pred, s);
  hipError_t e2 = hipFreeAsync(tmp, s);
  if (e != hipSuccess) return hip_fail(e, "hipcub::DeviceSelect::If");
  if (e2 != hipSuccess) return hip_fail(e2, "hipFreeAsync");
  return OGBX_OK;
}

}  // extern "C"
