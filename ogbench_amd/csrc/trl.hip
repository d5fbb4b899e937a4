// trl.hip -- TRL batches of GCDataset on gfx950 (include/ogbx_trl.h): the
// GC sample chain plus the value midpoint, a row drawn uniformly between the
// sample and its value goal, and the gathers of every column in one launch.
//
// Reference (hliuson/ogbench impls/utils/datasets.py):
//   GCDataset.__post_init__, TRL pick table   198-204
//   GCDataset.sample, TRL branch              254-292
//
// trl_sample_kernel is organised as gc_sample_kernel (gcsample.hip) and built
// from the same device code (gc_device.h; trl_device.h holds what it shares with
// the ring's online_trl_sample_kernel alone): tiles of at most 64 samples
// numbered XCD-major, the first wave runs the draw chain into LDS selectors,
// then the whole workgroup copies rows.  The fifth selector, the midpoint, is
// arithmetic on idx and the value goal -- mid = idx + mulhi(u64, goal - idx)
// with the two Philox words of slot 4 that the GC chain leaves unused -- so it
// adds no dependent load: midpoint rows are fetched in the same round trip as
// goal rows.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../../include/ogbx_trl.h"
#include "common.h"
#include "gc_device.h"
#include "trl_device.h"

namespace ogbx {

constexpr int kTrlSel = OGBX_TRL_SELECT_MIDPOINT + 1;

template <bool kInj>
__global__ void __launch_bounds__(256) trl_sample_kernel(
    ogbx_gc_buffer buf, ogbx_gc_config cfg, GcColumns cols, int32_t num_cols, int64_t total, int tile,
    ogbx_gc_draws dr, const int64_t* __restrict__ mid_in, uint32_t k0, uint32_t k1, uint32_t call_lo,
    uint32_t call_hi, double v_log_q, double a_log_q, ogbx_trl_outputs o, ogbx_gc_draw_record rec,
    int64_t* __restrict__ mid_rec, bool flat4) {
  __shared__ int64_t sel[kTrlSel][kGcMaxTile];
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
    // the GC chain, word for word as gc_sample_kernel draws it
    const int64_t npick = buf.valid_idxs ? buf.num_valid : buf.num_rows;
    int64_t idx = 0, pick, final_idx;
    GoalDraws v, a;
    root_picks<kInj, false>(dr, s, w[0], w[1], npick, buf.num_rows, &idx, &pick, &v.pick, &a.pick);
    // an injected midpoint row: loaded with the index loads, not after them
    const int64_t mid_given = (kInj && mid_in) ? mid_in[s] : 0;
    index_loads(buf, kInj && dr.idxs != nullptr, pick, &idx, &final_idx);
    const int64_t v_rand = cfg.value_cur_is_one ? 0 : rand_goal_of(buf, v.pick);
    const int64_t a_rand = cfg.actor_cur_is_one ? 0 : rand_goal_of(buf, a.pick);
    const int64_t next = idx + 1 < buf.num_rows ? idx + 1 : buf.num_rows - 1;
    goal_side_draws<kInj>(dr, cfg, s, w[1], w[2], w[3], w[4], v_log_q, a_log_q, v, a);
    const int64_t vg = sample_goal(idx, final_idx, v, v_rand, cfg.value_p_curgoal,
                                   cfg.value_traj_thresh, cfg.value_geom_sample, cfg.value_cur_is_one);
    const int64_t ag = sample_goal(idx, final_idx, a, a_rand, cfg.actor_p_curgoal,
                                   cfg.actor_traj_thresh, cfg.actor_geom_sample, cfg.actor_cur_is_one);
    // value midpoint: randint(idx, vg) (datasets.py:259), words z, w of slot 4.
    // No row lies in [idx, vg) when vg <= idx: counted, and mid = idx keeps
    // the gathers inside the buffer.
    const int64_t span = vg - idx;
    const bool bad = span <= 0;
    int64_t mid = idx;
    if (!bad) {
      if (kInj && mid_in)
        mid = mid_given < 0 ? 0 : (mid_given >= buf.num_rows ? buf.num_rows - 1 : mid_given);
      else
        mid = idx + (int64_t)bounded64(w[4].z, w[4].w, (uint64_t)span);
    }
    count_bad_samples(o.bad_count, bad, own);
    if (own) {
      sel[0][b] = idx;
      sel[1][b] = next;
      sel[2][b] = vg;
      sel[3][b] = ag;
      sel[4][b] = mid;
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

struct NotTrajEnd {
  const int64_t* traj_end;
  __device__ bool operator()(const int64_t& r) const { return traj_end[r] != r; }
};

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_trl_api_version(void) { return OGBX_TRL_API_VERSION; }

ogbx_status ogbx_trl_sample(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                            const ogbx_gc_column* cols, int32_t num_cols, int64_t batch,
                            int64_t num_batches, const ogbx_gc_draws* draws, const int64_t* midpoint,
                            uint64_t seed, uint64_t call_index, const ogbx_trl_outputs* out,
                            const ogbx_gc_draw_record* record, int64_t* midpoint_record, void* stream) {
  const char* who = "ogbx_trl_sample";
  OGBX_CHECK(buf && cfg && out && (cols || num_cols == 0), OGBX_EINVAL, named(who, "null argument"));
  GcColumns cc{};
  bool flat4;
  GC_TRY(check_columns(cols, num_cols, batch, num_batches, OGBX_TRL_SELECT_MIDPOINT, who, &cc, &flat4));
  GC_TRY(check_buffer(buf));
  const ogbx_gc_draws dr = draws ? *draws : ogbx_gc_draws{};
  const ogbx_gc_draw_record rec = record ? *record : ogbx_gc_draw_record{};
  GC_TRY(check_draw_record_complete(rec, who));

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  OGBX_CHECK(all_on_device(dev, {buf->traj_end, buf->valid_idxs, buf->valid_traj_end, buf->valid_pairs}) &&
                 trl_pointers_on_device(dev, dr, rec, *out, midpoint, midpoint_record, cols, num_cols),
             OGBX_EINVAL, named(who, "every pointer must be device memory of the current device"));

  const GcParams pr = gc_params(seed, *cfg, nullptr);  // the GC stream tag: same words as ogbx_gc_sample
  const int64_t total = batch * num_batches;
  int64_t tile, blocks;
  sample_grid(total, &tile, &blocks);
  const auto kern = (any_draw(dr) || midpoint) ? trl_sample_kernel<true> : trl_sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, *buf, *cfg, cc, num_cols,
                     total, (int)tile, dr, midpoint, pr.k0, pr.k1, (uint32_t)call_index,
                     (uint32_t)(call_index >> 32), pr.v_log_q, pr.a_log_q, *out, rec, midpoint_record, tile <= 4 && flat4);
  OGBX_LAUNCHED("trl_sample_kernel");
  return OGBX_OK;
}

ogbx_status ogbx_trl_valid_idxs(const int64_t* traj_end, int64_t num_rows, int64_t* out, int64_t* count,
                                void* stream) {
  OGBX_CHECK(traj_end && out && count && num_rows > 0, OGBX_EINVAL, "ogbx_trl_valid_idxs: bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipcub::CountingInputIterator<int64_t> it(0);
  NotTrajEnd pred{traj_end};
  size_t tmp_bytes = 0;
  OGBX_HIP(hipcub::DeviceSelect::If(nullptr, tmp_bytes, it, out, count, num_rows, pred, s));
  void* tmp = nullptr;
  OGBX_HIP(hipMallocAsync(&tmp, tmp_bytes > 0 ? tmp_bytes : 1, s));
  hipError_t e = hipcub::DeviceSelect::If(tmp, tmp_bytes, it, out, count, num_rows, pred, s);
  hipError_t e2 = hipFreeAsync(tmp, s);
  if (e != hipSuccess) return hip_fail(e, "hipcub::DeviceSelect::If");
  if (e2 != hipSuccess) return hip_fail(e2, "hipFreeAsync");
  return OGBX_OK;
}

}  // extern "C"
