// trl_device.h -- what the TRL sample kernels over a dataset (trl.hip) and over
// the episode ring (online_trl.hip) share after the GC chain of gc_device.h:
// the count of samples without a value midpoint, the draw-record check and the
// pointer list of ogbx_trl_sample / ogbx_online_trl_sample.  Internal to libogbx.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/ogbx_trl.h"
#include "common.h"
#include "gc_device.h"

namespace ogbx {

// bad_count += the wave's lanes with a bad sample of their own.  Every lane of
// the first wave calls it: one atomic per tile at most.
__device__ __forceinline__ void count_bad_samples(int64_t* bad_count, bool bad, bool own) {
  if (bad_count) {
    const unsigned long long m = __ballot(bad && own);
    if (m != 0ull && threadIdx.x == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(bad_count), (unsigned long long)__popcll(m));
  }
}

// ---------------------------------------------------------------- host side
// A draw record is all eleven arrays or none (rec.pick NULL).
static ogbx_status check_draw_record_complete(const ogbx_gc_draw_record& rec, const char* who) {
  OGBX_CHECK(!rec.pick || (rec.v_pick && rec.v_geom && rec.v_dist && rec.v_u_traj && rec.v_u_cur && rec.a_pick &&
                           rec.a_geom && rec.a_dist && rec.a_u_traj && rec.a_u_cur),
             OGBX_EINVAL, named(who, "incomplete draw record"));
  return OGBX_OK;
}

// The optional pointers of a TRL call (NULL: absent) and both ends of every
// gather column are device memory of `dev`.
static bool trl_pointers_on_device(int dev, const ogbx_gc_draws& dr, const ogbx_gc_draw_record& rec,
                                   const ogbx_trl_outputs& o, const int64_t* midpoint,
                                   const int64_t* midpoint_record, const ogbx_gc_column* cols, int32_t num_cols) {
  bool ok = all_on_device(
      dev, {midpoint, midpoint_record, dr.idxs, dr.pick, dr.v_pick, dr.v_geom, dr.v_dist, dr.v_u_traj, dr.v_u_cur,
            dr.a_pick, dr.a_geom, dr.a_dist, dr.a_u_traj, dr.a_u_cur, rec.pick, rec.v_pick, rec.v_geom, rec.v_dist,
            rec.v_u_traj, rec.v_u_cur, rec.a_pick, rec.a_geom, rec.a_dist, rec.a_u_traj, rec.a_u_cur, o.idxs,
            o.value_goal_idxs, o.actor_goal_idxs, o.value_midpoint_idxs, o.value_offsets, o.value_midpoint_offsets,
            o.masks, o.rewards, o.bad_count});
  for (int i = 0; i < num_cols && ok; ++i) ok = all_on_device(dev, {cols[i].src, cols[i].dst});
  return ok;
}

}  // namespace ogbx
