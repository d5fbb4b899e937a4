// gc_device.h -- what the fused sample kernels of gcsample.hip and trl.hip
// share: the per-sample draw chain (index loads, goal relabel), the tile
// helpers (Philox words, XCD-major numbering, row copies) and the host-side
// argument checks and launch parameters of the ogbx_gc_* / ogbx_hgc_* /
// ogbx_trl_* entry points.  The samplers of replay.hip, online.hip,
// online_hgc.hip and online_trl.hip take the tile helpers, the goal draws and
// their record (goal_side_draws, store_draw_record) and the gather-column check
// (check_gather_columns) from here too, and with them the first wave's
// prologue (sample_words, root_picks), store_gc_scalars,
// sample_grid and the hierarchical host checks (check_hgc_config,
// check_hgc_outputs).  trl_device.h holds what the two TRL kernels share beyond
// that; on_device / all_on_device and clamp_row are common.h's.  Internal to
// libogbx.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "common.h"

namespace ogbx {

constexpr int kGcMaxTile = 64;
constexpr int kGcMaxCols = 32;

template <int N>
struct GcColumnsN {
  ogbx_gc_column c[N];
};
using GcColumns = GcColumnsN<kGcMaxCols>;
// A sampler plan's batches of at most 16 columns (GC 9, HGC 15) launch with
// this half-size table: the host's launch cost grows with the kernel
// arguments (a 1,376-byte argument 2.5 -> 3.4 us per launch on ROCm 7,
// profiles/r06_launch_host.txt), and a steady sample(1024) call is host-bound.
constexpr int kGcSmallCols = 16;
using GcColumnsSmall = GcColumnsN<kGcSmallCols>;

__device__ inline uint64_t bounded64(uint32_t hi, uint32_t lo, uint64_t n) {
  const uint64_t u = ((uint64_t)hi << 32) | lo;
  return __umul64hi(u, n);
}

struct GoalDraws {
  int64_t pick;
  int64_t geom;
  double dist, u_traj, u_cur;
};

// GCDataset.sample_goals for one sample (datasets.py:296-327).
// rand_goal = valid_idxs[d.pick] (or d.pick), loaded by the caller together
// with the sample's other index loads.
__device__ inline int64_t sample_goal(int64_t idx, int64_t final_idx, const GoalDraws& d,
                                      int64_t rand_goal, double p_cur, double thresh, int geom,
                                      int cur_is_one) {
  if (cur_is_one) return idx;
  int64_t traj;
  if (geom) {
    const int64_t s = idx + d.geom;
    traj = s < final_idx ? s : final_idx;
  } else {
    const int64_t lo = idx + 1 < final_idx ? idx + 1 : final_idx;
    traj = (int64_t)rint((double)lo * d.dist + (double)final_idx * (1.0 - d.dist));
  }
  int64_t goal = d.u_traj < thresh ? traj : rand_goal;
  goal = d.u_cur < p_cur ? idx : goal;
  return goal;
}

// The sample's dependent index loads, issued back to back so that they share
// one HBM round trip: idx = valid_idxs[pick], its trajectory end, and the
// random goals valid_idxs[goal pick] (datasets.py:65-70, 307-309).  Every
// condition is wave-uniform (pointer presence), so no load address waits on
// another load; for explicit idxs (pick < 0) the end needs idx first.
// Periodic buffer (ogbx_gc_buffer.period > 0): pick p lies in period
// q = p / period_picks at offset r, so idx = q period + r and its trajectory
// end is q period + period_end -- no index load at all.  The IEEE quotient is
// off by at most one near an integer; the remainder test corrects it.
__device__ inline int64_t periodic_row(const ogbx_gc_buffer& buf, int64_t pick, int64_t* q_out) {
  // the quotient estimate by the reciprocal (a function of the kernel
  // arguments alone, so it is computed off the sample's chain): within one of
  // floor(pick / period_picks) like the IEEE quotient, and the remainder test
  // below makes q exact either way
  const double inv_pp = 1.0 / (double)buf.period_picks;
  int64_t q = (int64_t)((double)pick * inv_pp);
  int64_t r = pick - q * buf.period_picks;
  if (r < 0) {
    --q;
    r += buf.period_picks;
  } else if (r >= buf.period_picks) {
    ++q;
    r -= buf.period_picks;
  }
  *q_out = q;
  return q * buf.period + r;
}

__device__ inline void index_loads(const ogbx_gc_buffer& buf, bool explicit_idxs, int64_t pick,
                                   int64_t* idx, int64_t* fin) {
  const int64_t* __restrict__ vi = buf.valid_idxs;
  if (!explicit_idxs && buf.period > 0) {
    int64_t q;
    *idx = periodic_row(buf, pick, &q);
    *fin = q * buf.period + buf.period_end;
  } else if (explicit_idxs) {
    *fin = buf.traj_end[*idx];
  } else if (buf.valid_pairs) {
    const longlong2 p = reinterpret_cast<const longlong2*>(buf.valid_pairs)[pick];
    *idx = p.x;
    *fin = p.y;
  } else if (vi && buf.valid_traj_end) {
    *idx = vi[pick];
    *fin = buf.valid_traj_end[pick];
  } else if (vi) {
    *idx = vi[pick];
    *fin = buf.traj_end[*idx];
  } else {
    *idx = pick;
    *fin = buf.traj_end[pick];
  }
}

__device__ inline int64_t rand_goal_of(const ogbx_gc_buffer& buf, int64_t pick) {
  if (buf.period > 0) {
    int64_t q;
    return periodic_row(buf, pick, &q);
  }
  if (buf.valid_pairs) return buf.valid_pairs[2 * pick];
  return buf.valid_idxs ? buf.valid_idxs[pick] : pick;
}

// Source row pitch of a column in units of T (src_stride 0 = dense rows).
template <typename T>
__device__ __forceinline__ int64_t src_pitch(const ogbx_gc_column& col) {
  return (col.src_stride ? (int64_t)col.src_stride : col.row_bytes) / (int64_t)sizeof(T);
}

__device__ inline int64_t geometric_from(double u, double log_q) {
  // legacy RandomState.geometric inversion: ceil(log(1-u) / log(1-p))
  double g = ceil(log(1.0 - u) / log_q);
  return g < 1.0 ? 1 : (int64_t)g;
}

// The eight draws of the value and actor goals besides the picks, in the slot
// layout every sampler shares (words w1.zw .. w4.xy of sample s); an injected
// draw replaces its Philox value in the kInj instances.  The picks stay with
// the kernels: they load with the index loads, and the ring clamps them.
// A kernel calls this only where its gfx950 code is the written-out block's,
// instruction for instruction (profiles/buffer_refactor_isa.txt):
// hgc_sample_kernel (gcsample.hip) keeps the block written out -- through the
// helper both of its instances came out 5 and 7 instructions longer with
// another SGPR assignment.
template <bool kInj>
__device__ __forceinline__ void goal_side_draws(const ogbx_gc_draws& dr, const ogbx_gc_config& cfg, int64_t s,
                                                const u32x4& w1, const u32x4& w2, const u32x4& w3, const u32x4& w4,
                                                double v_log_q, double a_log_q, GoalDraws& v, GoalDraws& a) {
  const double uvg = u01_from(w1.z, w1.w), uag = u01_from(w2.x, w2.y);
  v.geom = (kInj && dr.v_geom) ? dr.v_geom[s] : (cfg.value_geom_sample ? geometric_from(uvg, v_log_q) : 0);
  a.geom = (kInj && dr.a_geom) ? dr.a_geom[s] : (cfg.actor_geom_sample ? geometric_from(uag, a_log_q) : 0);
  v.dist = (kInj && dr.v_dist) ? dr.v_dist[s] : uvg;
  a.dist = (kInj && dr.a_dist) ? dr.a_dist[s] : uag;
  v.u_traj = (kInj && dr.v_u_traj) ? dr.v_u_traj[s] : u01_from(w2.z, w2.w);
  v.u_cur = (kInj && dr.v_u_cur) ? dr.v_u_cur[s] : u01_from(w3.x, w3.y);
  a.u_traj = (kInj && dr.a_u_traj) ? dr.a_u_traj[s] : u01_from(w3.z, w3.w);
  a.u_cur = (kInj && dr.a_u_cur) ? dr.a_u_cur[s] : u01_from(w4.x, w4.y);
}

// The draws sample s used, to the record of a recording call (rec.pick NULL:
// none).  pick is -1 where the call gave the row itself.
__device__ __forceinline__ void store_draw_record(const ogbx_gc_draw_record& rec, int64_t s, int64_t pick,
                                                  const GoalDraws& v, const GoalDraws& a) {
  if (rec.pick) {
    rec.pick[s] = pick;
    rec.v_pick[s] = v.pick;
    rec.v_geom[s] = v.geom;
    rec.v_dist[s] = v.dist;
    rec.v_u_traj[s] = v.u_traj;
    rec.v_u_cur[s] = v.u_cur;
    rec.a_pick[s] = a.pick;
    rec.a_geom[s] = a.geom;
    rec.a_dist[s] = a.dist;
    rec.a_u_traj[s] = a.u_traj;
    rec.a_u_cur[s] = a.u_cur;
  }
}

// Threads [t0, blockDim.x) copy (t0 = 64: the first wave is busy elsewhere).
template <typename T>
__device__ inline void copy_rows(const ogbx_gc_column& col, const int64_t* sel, int64_t base,
                                 int tile, int t0) {
  const int64_t units = col.row_bytes / (int64_t)sizeof(T);
  const int64_t pitch = src_pitch<T>(col);
  const T* __restrict__ src = (const T*)col.src;
  T* __restrict__ dst = (T*)col.dst;
  const int64_t total = units * tile;
  const int step = blockDim.x - t0, tid = threadIdx.x - t0;
  int64_t b = tid / units, k = tid % units;
  const int64_t sb = step / units, sk = step % units;
  for (int64_t f = tid; f < total; f += step) {
    dst[(base + b) * units + k] = src[sel[b] * pitch + k];
    k += sk;
    b += sb;
    if (k >= units) {
      k -= units;
      b += 1;
    }
  }
}

// Copy every column row of a tile.  For small tiles (latency-bound launches)
// whose columns are all 4-byte granular with rows of <= 128 words, each
// (column, sample) row is one job for one wave: the job's column descriptor
// and row index are wave-uniform (scalar loads, one LDS broadcast), lanes
// cover the row's words, and each wave issues the loads of up to kJ jobs
// before any store, so all column rows of the tile share one HBM round trip.
// Otherwise each column is copied with its widest aligned unit.
// Waves [wave0, blockDim.x / 64) copy (wave0 = 1: the first wave computes the
// next call's selectors meanwhile, gc_ahead_kernel).
// kNt: non-temporal stores on the small-tile path (the HGC hit kernel: its 3.6
// MB of rows per launch leave less to the end-of-kernel write-back, 6.44 ->
// 6.34 us; GC's 1.3 MB measured 4.34 -> 4.38 us and keeps plain stores)
template <int kSel, bool kNt = false, class Cols = GcColumns>
__device__ inline void copy_tile(const Cols& cols, int num_cols, const int64_t (*sel)[kGcMaxTile], int64_t base,
                                 int n_here, bool flat4, int wave0 = 0) {
  if ((int)(threadIdx.x >> 6) < wave0) return;
  if (flat4) {
    constexpr int kJ = 8, kSlots = 2;
    const int nw = (int)(blockDim.x >> 6) - wave0;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) - wave0;
    const int lane = (int)(threadIdx.x & 63);
    const int jobs = num_cols * n_here;
    for (int j0 = wave; j0 < jobs; j0 += nw * kJ) {
      uint32_t v[kJ][kSlots];
      uint32_t* d[kJ][kSlots];
#pragma unroll
      for (int u = 0; u < kJ; ++u) {
        const int j = j0 + u * nw;
#pragma unroll
        for (int q = 0; q < kSlots; ++q) d[u][q] = nullptr;
        if (j < jobs) {
          const int c = j / n_here, b = j - c * n_here;
          const ogbx_gc_column& col = cols.c[c];
          const int units = (int)(col.row_bytes >> 2);
          const uint32_t* src = (const uint32_t*)col.src + sel[col.select][b] * src_pitch<uint32_t>(col);
          uint32_t* dst = (uint32_t*)col.dst + (base + b) * units;
#pragma unroll
          for (int q = 0; q < kSlots; ++q) {
            const int k = lane + 64 * q;
            if (k < units) {
              v[u][q] = src[k];
              d[u][q] = dst + k;
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kJ; ++u)
#pragma unroll
        for (int q = 0; q < kSlots; ++q)
          if (d[u][q]) {
            if constexpr (kNt)
              __builtin_nontemporal_store(v[u][q], d[u][q]);
            else
              *d[u][q] = v[u][q];
          }
    }
    return;
  }
  for (int c = 0; c < num_cols; ++c) {
    const ogbx_gc_column& col = cols.c[c];
    const int64_t* srow = sel[col.select];
    const uintptr_t align = (uintptr_t)col.src | (uintptr_t)col.dst | (uintptr_t)col.src_stride;
    const int t0 = 64 * wave0;
    if (col.row_bytes % 16 == 0 && align % 16 == 0)
      copy_rows<uint4>(col, srow, base, n_here, t0);
    else if (col.row_bytes % 8 == 0 && align % 8 == 0)
      copy_rows<uint2>(col, srow, base, n_here, t0);
    else if (col.row_bytes % 4 == 0 && align % 4 == 0)
      copy_rows<uint32_t>(col, srow, base, n_here, t0);
    else
      copy_rows<uint8_t>(col, srow, base, n_here, t0);
  }
}

// The tile's Philox words, one call per lane: sample b of the tile, call q
// (q < calls) -> wb[q][b].  A B = 1024 launch has two samples per workgroup,
// so in-lane calls would run kCalls dependent-free chains on two lanes; spread
// over 2 * kCalls lanes each lane runs one.  Same counters and keys as the
// in-lane form, so the words are identical.
constexpr bool kGcSpread = true;
// Every lane of a wave that has a call computes one (lanes past the last call
// repeat one and store nothing): gfx950 issues a dependent integer chain about
// twice as slowly with <= 16 active lanes, and a B = 1,024 tile
// has 5-7 calls.
__device__ inline void tile_philox(uint4 (*wb)[kGcMaxTile], int calls, int n_here, int64_t base,
                                   uint32_t call_lo, uint32_t call_hi, uint32_t k0, uint32_t k1) {
  const int tot = calls * n_here, span = (tot + 63) & ~63;
  for (int t = threadIdx.x; t < span; t += blockDim.x) {
    const int tt = t < tot ? t : t % tot;
    const int b = tt / calls, q = tt - b * calls;
    const uint64_t su = (uint64_t)(base + b);
    const u32x4 w = philox4x32_10({(uint32_t)su, call_lo, (uint32_t)q, (uint32_t)(su >> 32) ^ call_hi}, k0, k1);
    if (t < tot) wb[q][b] = make_uint4(w.x, w.y, w.z, w.w);
  }
}
// Tile of this workgroup: consecutive workgroup ids go round-robin to the 8
// XCDs, each with its own L2, so tiles are numbered XCD-major -- the
// workgroups of one XCD own a contiguous run of samples and the partial
// 128-B lines where one sample's output rows meet the next are merged in
// that XCD's L2 instead of being written back twice.
__device__ inline int64_t xcd_tile() {
  const int64_t b = blockIdx.x, nb = gridDim.x;
  const int64_t per = nb >> 3, rem = nb & 7, x = b & 7;
  return x * per + (x < rem ? x : rem) + (b >> 3);
}

__device__ inline u32x4 tile_word(const uint4 (*wb)[kGcMaxTile], int q, int b) {
  const uint4 v = wb[q][b];
  return u32x4{v.x, v.y, v.z, v.w};
}

// ------- the first wave's prologue, over a dataset and over the ring; a kernel takes
// a helper only where its gfx950 code stays (profiles/sampler_device_refactor_isa.txt)
// Philox words 0 .. 4 of sample s, the lane's sample b of the tile: the tile's
// words from LDS (tile_philox), else (kInLane) computed in the lane.
template <bool kInLane>
__device__ __forceinline__ void sample_words(const uint4 (*wb)[kGcMaxTile], int b, int64_t s, uint32_t call_lo,
                                             uint32_t call_hi, uint32_t k0, uint32_t k1, u32x4* w) {
  const uint64_t su = (uint64_t)s;
  const uint32_t c0 = (uint32_t)su, c3 = (uint32_t)(su >> 32) ^ call_hi;
  if constexpr (kInLane) {
    w[0] = philox4x32_10({c0, call_lo, 0u, c3}, k0, k1);
    w[1] = philox4x32_10({c0, call_lo, 1u, c3}, k0, k1);
    w[2] = philox4x32_10({c0, call_lo, 2u, c3}, k0, k1);
    w[3] = philox4x32_10({c0, call_lo, 3u, c3}, k0, k1);
    w[4] = philox4x32_10({c0, call_lo, 4u, c3}, k0, k1);
  } else {
    w[0] = tile_word(wb, 0, b), w[1] = tile_word(wb, 1, b), w[2] = tile_word(wb, 2, b), w[3] = tile_word(wb, 3, b),
    w[4] = tile_word(wb, 4, b);
  }
}

// The picks of the sample, its value goal and its actor goal out of npick
// (words w0.xy, w0.zw, w1.xy), an injected pick in place of its Philox value;
// kClamp (the ring) moves injected picks into [0, npick).  *pick stays -1 where
// the call gave the row itself (dr.idxs).
template <bool kInj, bool kClamp>
__device__ __forceinline__ void root_picks(const ogbx_gc_draws& dr, int64_t s, const u32x4& w0, const u32x4& w1,
                                           int64_t npick, int64_t nrows, int64_t* idx, int64_t* pick,
                                           int64_t* v_pick, int64_t* a_pick) {
  auto given = [s](const int64_t* p, int64_t n) { return kClamp ? clamp_row(p[s], n) : p[s]; };
  *pick = -1;
  if (kInj && dr.idxs) {
    *idx = given(dr.idxs, nrows);
  } else {
    *pick = (kInj && dr.pick) ? given(dr.pick, npick) : (int64_t)bounded64(w0.x, w0.y, (uint64_t)npick);
    if (kClamp) *idx = *pick;  // over the ring the pick is the row (a pick table maps it next)
  }
  *v_pick = (kInj && dr.v_pick) ? given(dr.v_pick, npick) : (int64_t)bounded64(w0.z, w0.w, (uint64_t)npick);
  *a_pick = (kInj && dr.a_pick) ? given(dr.a_pick, npick) : (int64_t)bounded64(w1.x, w1.y, (uint64_t)npick);
}

// The per-sample scalars of a GC batch (the index outputs may be NULL).
__device__ __forceinline__ void store_gc_scalars(int64_t* idxs_out, int64_t* vgoal_out, int64_t* agoal_out,
                                                 double* masks, double* rewards, int gc_negative, int64_t s,
                                                 int64_t idx, int64_t vg, int64_t ag) {
  if (idxs_out) idxs_out[s] = idx;
  if (vgoal_out) vgoal_out[s] = vg;
  if (agoal_out) agoal_out[s] = ag;
  const double succ = idx == vg ? 1.0 : 0.0;
  masks[s] = 1.0 - succ;
  rewards[s] = succ - (gc_negative ? 1.0 : 0.0);
}

// ---------------------------------------------------------------- host side
// Every column 4-byte granular and aligned with rows of <= 128 words (the
// per-wave job copy of copy_tile).
static bool flat4_columns(const ogbx_gc_column* cols, int num_cols) {
  bool flat4 = true;
  for (int i = 0; i < num_cols; ++i) {
    const ogbx_gc_column& c = cols[i];
    flat4 = flat4 && c.row_bytes % 4 == 0 && c.row_bytes <= 512 &&
            ((uintptr_t)c.src | (uintptr_t)c.dst | (uintptr_t)c.src_stride) % 4 == 0;
  }
  return flat4;
}

// True when any draw is injected (parity replays); the Philox-only kernels
// carry no per-draw pointer tests, so their index loads issue back to back.
static bool any_draw(const ogbx_gc_draws& d) {
  return d.idxs || d.pick || d.v_pick || d.v_geom || d.v_dist || d.v_u_traj || d.v_u_cur ||
         d.a_pick || d.a_geom || d.a_dist || d.a_u_traj || d.a_u_cur;
}

// period == 0, or a whole number of periods covering the buffer with the
// picks and the trajectory end inside one period.
static bool periodic_ok(const ogbx_gc_buffer& b) {
  if (b.period == 0) return true;
  const int64_t npick = b.valid_idxs ? b.num_valid : b.num_rows;
  return b.period > 0 && b.period_picks > 0 && b.period_picks <= b.period && b.period_end >= 0 &&
         b.period_end < b.period && b.num_rows % b.period == 0 &&
         npick == (b.num_rows / b.period) * b.period_picks;
}

// ------------------------------------------------------------ argument checks
// Every check of the GC / HGC entry points lives here, once; an entry point
// runs its checks before its first HIP call.  `who` is the entry point's name.
static std::string named(const char* who, const char* what) { return std::string(who) + ": " + what; }

static ogbx_status check_buffer(const ogbx_gc_buffer* buf) {
  OGBX_CHECK(buf->num_rows > 0 && buf->traj_end, OGBX_EINVAL, "empty trajectory buffer");
  OGBX_CHECK(buf->valid_idxs == nullptr || buf->num_valid > 0, OGBX_EINVAL,
             "no valid transitions in the dataset");
  OGBX_CHECK(periodic_ok(*buf), OGBX_EINVAL, "ogbx_gc_buffer: inconsistent period fields");
  return OGBX_OK;
}

// The descriptors of a gather-column table of num_cols entries (the count is
// the entry point's to check), column by column: bit k of `selects` allows
// select code k.  Copies the table to *cc (the kernel argument; NULL: not
// here) and tells whether copy_tile may take its per-wave job copy (*flat4).
// The entry points word their rejects in two ways, each pinned by its tests:
//   kSplitNull (replay and ring): "null column pointer" on its own and first,
//     then "bad column descriptor", then the stride;
//   otherwise (ogbx_gc_* / ogbx_hgc_* / ogbx_trl_*): the stride first, then a
//     null pointer folded into "bad column descriptor".
template <bool kSplitNull, class Cols>
static ogbx_status check_gather_columns(const ogbx_gc_column* cols, int32_t num_cols, uint32_t selects,
                                        const char* who, Cols* cc, bool* flat4) {
  for (int i = 0; i < num_cols; ++i) {
    const ogbx_gc_column& c = cols[i];
    const bool ptrs = c.src && c.dst;
    const bool desc = c.row_bytes > 0 && c.select >= 0 && c.select < 32 && ((selects >> c.select) & 1u);
    if (kSplitNull) {
      OGBX_CHECK(ptrs, OGBX_EINVAL, named(who, "null column pointer"));
      OGBX_CHECK(desc, OGBX_EINVAL, named(who, "bad column descriptor"));
    }
    OGBX_CHECK(c.src_stride == 0 || c.src_stride >= c.row_bytes, OGBX_EINVAL, named(who, "src_stride below row_bytes"));
    OGBX_CHECK(ptrs && desc, OGBX_EINVAL, named(who, "bad column descriptor"));
    if (cc) cc->c[i] = c;
  }
  *flat4 = flat4_columns(cols, num_cols);
  return OGBX_OK;
}

// The hierarchical checks ogbx_hgc_* and ogbx_online_hgc_sample share.  The
// bound on the subgoal steps and its wording are the entry point's: >= 0 and
// "negative subgoal steps" over a dataset, >= 1 over the ring.
static ogbx_status check_hgc_config(const ogbx_hgc_config* hcfg, const char* who, int64_t min_steps,
                                    const char* steps_words) {
  OGBX_CHECK(hcfg->hv_mask_table && hcfg->hv_reward_table && hcfg->lv_mask_table && hcfg->lv_reward_table,
             OGBX_EINVAL, named(who, "missing reward/mask tables"));
  OGBX_CHECK(hcfg->value_subgoal_steps >= min_steps && hcfg->low_subgoal_steps >= min_steps &&
                 hcfg->actor_subgoal_steps >= min_steps,
             OGBX_EINVAL, named(who, steps_words));
  OGBX_CHECK(!hcfg->has_low_value_goals || (hcfg->low_discount > 0.0 && hcfg->low_discount < 1.0), OGBX_EINVAL,
             named(who, "low_discount must be in (0, 1)"));
  return OGBX_OK;
}

static ogbx_status check_hgc_outputs(const ogbx_hgc_outputs* out, const char* who) {
  OGBX_CHECK(out && out->high_value_offsets && out->high_value_subgoal_steps && out->high_value_masks &&
                 out->high_value_rewards && out->low_value_subgoal_steps && out->low_value_masks &&
                 out->low_value_rewards && out->masks && out->rewards,
             OGBX_EINVAL, named(who, "missing scalar output"));
  return OGBX_OK;
}

// Bits 0 .. max_select: the select codes of the dataset samplers.
constexpr uint32_t selects_up_to(int max_select) { return (2u << max_select) - 1u; }

// The batch shape and the column descriptors (select in [0, max_select]),
// copied into the kernel-argument table *cc.
static ogbx_status check_columns(const ogbx_gc_column* cols, int32_t num_cols, int64_t batch, int64_t num_batches,
                                 int max_select, const char* who, GcColumns* cc, bool* flat4) {
  OGBX_CHECK(num_cols >= 0 && num_cols <= kGcMaxCols, OGBX_EINVAL, named(who, "at most 32 columns"));
  OGBX_CHECK(batch > 0 && num_batches > 0, OGBX_EINVAL, "batch and num_batches must be > 0");
  return check_gather_columns<false>(cols, num_cols, selects_up_to(max_select), who, cc, flat4);
}

// ------------------------------------------------- derived launch parameters
// tile: one sample per workgroup up to 1024 samples (B = 1024: 1,024
// workgroups of 256 threads; measured against 2 and 4 samples per workgroup
// and 64- to 1024-thread workgroups), then up to 64 per workgroup
static int64_t gc_tile(int64_t total) { return std::clamp<int64_t>(total / 1024, 1, kGcMaxTile); }

// Samples per workgroup and workgroups of a launch; false when the grid passes
// the launch limit (the ring and replay entry points refuse that).
static bool sample_grid(int64_t total, int64_t* tile, int64_t* blocks) {
  *tile = gc_tile(total);
  *blocks = (total + *tile - 1) / *tile;
  return *blocks <= 0x7fffffffll;
}

// What a (seed, config) fixes for every call: the Philox key and the
// log(1 - p) terms of the geometric draws (p = 1 - discount).
struct GcParams {
  uint32_t k0 = 0, k1 = 0;
  double v_log_q = 0, a_log_q = 0, l_log_q = 0;
};

static GcParams gc_params(uint64_t seed, const ogbx_gc_config& cfg, const ogbx_hgc_config* hcfg) {
  GcParams pr;
  seed_key(seed, hcfg ? kTagHgcSample : kTagGcSample, &pr.k0, &pr.k1);
  pr.v_log_q = std::log(1.0 - (1.0 - cfg.value_discount));
  pr.a_log_q = std::log(1.0 - (1.0 - cfg.actor_discount));
  pr.l_log_q = (hcfg && hcfg->has_low_value_goals) ? std::log(1.0 - (1.0 - hcfg->low_discount)) : 0.0;
  return pr;
}

}  // namespace ogbx
