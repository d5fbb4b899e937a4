/* ogbx_online_hgc.h -- hierarchical hindsight sampling over the on-device
 * episode ring of ogbx_online.h: HGCDataset.sample (hliuson/ogbench
 * impls/utils/datasets.py:478-643) over the live rows in one launch.
 *
 * An extension of include/ogbx.h and include/ogbx_online.h exported by the
 * same libogbx.so.  It has its own version (ogbx_online_hgc_api_version());
 * OGBX_ABI_VERSION, OGBX_STREAM_VERSION and OGBX_ONLINE_API_VERSION cover
 * their own headers and are unchanged.  Conventions (status codes,
 * ogbx_last_error(), streams, device pointers) are those of ogbx.h; the ring,
 * its snapshot and its flat indices u = e * L + k are those of ogbx_online.h;
 * the configs, draws, draw record, scalar outputs and column selectors are
 * those of ogbx_hgc_sample (ogbx.h).
 */
#ifndef OGBX_ONLINE_HGC_H_
#define OGBX_ONLINE_HGC_H_

#include "ogbx.h"
#include "ogbx_online.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_ONLINE_HGC_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_online_hgc_api_version(void);

/* HGCDataset.sample over the ring's snapshot in ONE launch of
 * online_hgc_sample_kernel.  Needs ring->steps >= 1.
 * Per sample: the flat pick and its episode's end fin exactly as
 * ogbx_online_gc_sample takes them (the end step clamped into
 * [row's step, S - 1]); the high value goal, with hcfg->has_low_value_goals
 * the low value goal (geometric with low_discount), and the high actor goal by
 * sample_goals (datasets.py:296-327) on the flat indices; the four
 * compute_high_next_idxs results (value / low steps against the high value
 * goal, actor / low steps against the high actor goal) and
 * low actor goal = min(idx + actor_subgoal_steps, fin).
 *   cols    select in ogbx_hgc_sample's numbering: 0 the sample's row, 2 high
 *           value goal, 3 high actor goal, 4 high value next, 5 low value
 *           next, 6 low value goal, 7 high actor next, 8 low actor goal, 9 low
 *           actor next; 1, the next row, is refused: the ring stores its own
 *           next_observations.  src is the ring's column [T * N, ...]; every
 *           selector is mapped to its physical row ((S - L + k) % T) * N + e.
 *           Up to 32 columns; up to 16 launch with a half-size argument table.
 *   total   samples.
 *   draws   optional injected draws; draws->gc.idxs are explicit flat rows.
 *           Explicit rows, injected picks and the three goals are clamped into
 *           [0, L * N).
 *   out     the scalars of ogbx_hgc_sample; the four index outputs (flat
 *           indices) may be NULL.  offsets, step counts, masks and rewards as
 *           ogbx_hgc_sample: the four tables of hcfg are indexed by the clipped
 *           step count, which lies in [0, K] because fin >= idx; with low
 *           value goals low_value_masks / low_value_rewards are
 *           1 - (idx == low goal) / (idx == low goal) - gc_negative.
 *   record  optional draw record.
 * Every physical row lies below T * N and every table read in bounds whatever
 * the episode tables and the injected draws hold.  Nothing is read back.
 * The draw.  No Philox tag or slot of its own: the key and the slot layout are
 * ogbx_hgc_sample's over a buffer of L * N rows without valid_idxs (five
 * words, seven with low value goals), so at one (seed, call) both return the
 * same batch.
 * Returns OGBX_EINVAL (message in ogbx_last_error()) before any device work
 * for a NULL ring / cfg / hcfg / out / episode table / reward or mask table /
 * column pointer, a ring outside its ranges, steps < 1, total <= 0, num_cols
 * outside 0..32, select outside {0, 2..9}, row_bytes <= 0, src_stride below
 * row_bytes, a subgoal step count < 1, low_discount outside (0, 1) with low
 * value goals, or a missing mandatory scalar output (high_value_offsets ..
 * rewards).  Pointers are not probed for residency (as ogbx_gc_sample). */
ogbx_status ogbx_online_hgc_sample(const ogbx_online_ring* ring, const ogbx_gc_config* cfg,
                                   const ogbx_hgc_config* hcfg, const ogbx_gc_column* cols, int32_t num_cols,
                                   int64_t total, const ogbx_hgc_draws* draws, const ogbx_hgc_outputs* out,
                                   const ogbx_hgc_draw_record* record, uint64_t seed, uint64_t call_index,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_ONLINE_HGC_H_ */
