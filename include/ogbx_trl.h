/* ogbx_trl.h -- TRL batches of GCDataset: the value midpoint, a row drawn
 * between each sample and its value goal, and the keys built around it
 * (hliuson/ogbench impls/utils/datasets.py:198-204, 254-292; consumed by
 * impls/agents/trl.py:44-68).
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_trl_api_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h.
 *
 * Scope: the direct path only.  There is no look-ahead / sampler-plan form
 * (ogbx_gc_plan_*) of the TRL sample; every call is one ogbx_trl_sample.
 */
#ifndef OGBX_TRL_H_
#define OGBX_TRL_H_

#include "ogbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_TRL_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_trl_api_version(void);

/* Row selector of the value midpoint (ogbx_gc_column.select; 0..3 are those of
 * ogbx_gc_sample: 0 idx, 1 min(idx+1, R-1), 2 value goal, 3 actor goal). */
#define OGBX_TRL_SELECT_MIDPOINT 4

/* Philox words.  The sample chain uses the GC stream tag and slots 0..4 of the
 * counter {sample_lo, call_lo, slot, sample_hi ^ call_hi} exactly as
 * ogbx_gc_sample does (slot 4: words x, y = the actor goal's u_cur), so idxs,
 * both goals, masks and rewards equal ogbx_gc_sample's for the same buffer,
 * config, seed and call.  The midpoint takes words z, w of slot 4, which the
 * GC chain leaves unused:
 *   mid = idx + mulhi64((z << 32) | w, value_goal - idx)     in [idx, goal)
 * (np.random.randint(idxs, value_goal_idxs), datasets.py:259).  No further
 * Philox call, no existing stream moves; the crop offsets of a visual batch
 * stay in OGBX_VISUAL_CROP_SLOT (ogbx_visual.h). */

/* Per-sample outputs, device arrays of batch * num_batches elements; every
 * pointer may be NULL (that output is not written). */
typedef struct {
  int64_t* idxs;
  int64_t* value_goal_idxs;
  int64_t* actor_goal_idxs;
  int64_t* value_midpoint_idxs;
  int64_t* value_offsets;          /* value goal - idx                         */
  int64_t* value_midpoint_offsets; /* midpoint - idx                           */
  double* masks;
  double* rewards;
  /* One int64, zeroed by the caller.  The kernel adds the number of samples
   * whose value goal is <= idx (no row lies between them): possible only with
   * explicit idxs that name a trajectory's last row, or with injected draws.
   * Such a sample gets mid = idx; its offsets are as computed. */
  int64_t* bad_count;
} ogbx_trl_outputs;

/* GCDataset.sample with the TRL branch (datasets.py:213-294) in ONE launch.
 *
 * buf, cfg, cols, batch, num_batches, draws, seed, call_index, record, stream:
 *   as ogbx_gc_sample.  buf describes the TRL pick table -- every row that is
 *   not the last of its trajectory (ogbx_trl_valid_idxs) -- in any of its
 *   forms (valid_pairs, valid_idxs + valid_traj_end, the periodic closed
 *   form); cfg needs value_p_curgoal = 0 and a value_traj_thresh of 1 (no
 *   random value goals), else the value goal may not lie past idx.
 * cols: up to 32 columns, select 0..3 as ogbx_gc_sample and
 *   OGBX_TRL_SELECT_MIDPOINT.
 * midpoint: NULL (draw it, see above), or device int64 [batch * num_batches]
 *   holding the midpoint ROW of each sample, the raw result of the reference's
 *   randint(idxs, value_goal_idxs); a row outside [0, R) is clamped into the
 *   buffer.
 * midpoint_record: NULL, or device int64 array that receives the midpoint rows
 *   used.
 * Returns OGBX_EINVAL (message in ogbx_last_error()) before any launch for a
 * NULL buf / cfg / out, num_cols > 32, a selector outside 0..4, non-positive
 * sizes, or a pointer that is not device memory of the current device. */
ogbx_status ogbx_trl_sample(const ogbx_gc_buffer* buf, const ogbx_gc_config* cfg,
                            const ogbx_gc_column* cols, int32_t num_cols, int64_t batch,
                            int64_t num_batches, const ogbx_gc_draws* draws, const int64_t* midpoint,
                            uint64_t seed, uint64_t call_index, const ogbx_trl_outputs* out,
                            const ogbx_gc_draw_record* record, int64_t* midpoint_record, void* stream);

/* The TRL pick table: the rows r of [0, num_rows) with traj_end[r] != r, in
 * order, to out (device int64 [num_rows]) and their number to *count (device
 * int64).  traj_end: ogbx_gc_traj_end's output. */
ogbx_status ogbx_trl_valid_idxs(const int64_t* traj_end, int64_t num_rows, int64_t* out, int64_t* count,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_TRL_H_ */
