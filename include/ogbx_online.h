/* ogbx_online.h -- hindsight goal sampling over an on-device episode ring:
 * what a batched env produced, one row per env and step, kept time-major with
 * incremental episode tables, and GCDataset.sample (hliuson/ogbench
 * impls/utils/datasets.py:213-327) over the live rows in one launch.
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_online_api_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h; the insert columns are those of ogbx_replay.h.
 *
 * The ring.  num_envs = N lanes, horizon = T time slots; every insert takes
 * exactly one row from every env.  The row of env e at logical step t lives
 * at physical row (t % T) * N + e of every column (dense [T * N, ...]).  The
 * caller counts the steps S inserted so far (ogbx_online_ring.steps) and
 * passes it to every call: nothing is read back.  L = min(S, T) steps are
 * live, S - L .. S - 1.
 *
 * The snapshot of a ring is the dataset of its live rows unrolled env-major:
 * flat index u = e * L + k holds env e at step S - L + k, and terminals[u] = 1
 * on the last row of every closed episode and on every env's newest row (an
 * open episode ends "now").  An episode whose head was overwritten starts at
 * its oldest live row.  ogbx_online_gc_sample returns what the reference's
 * GCDataset.sample returns over that snapshot; every index it takes or
 * reports (idxs, goal picks, index outputs) is a flat index u.
 *
 * Episode tables, O(1) per inserted row and never rewritten afterwards:
 *   ep_seq  int32 [T, N]  the ordinal of the env's episode the row belongs to
 *   cur_seq int32 [N]     the ordinal of the env's open episode (= the number
 *                         of episodes it closed)
 *   ep_end  int64 [T, N]  ep_end[(seq % T) * N + e]: the logical step at which
 *                         episode seq of env e closed
 * An env has at most T live episodes, so live ordinals are distinct mod T;
 * episode seq + T can close only after T further rows of that env, by when
 * every row of episode seq was overwritten.  A row of the open episode
 * (ep_seq == cur_seq[e]) ends at step S - 1, any other at its table entry.
 * All three are zeroed by the caller before the first insert.
 */
#ifndef OGBX_ONLINE_H_
#define OGBX_ONLINE_H_

#include "ogbx.h"
#include "ogbx_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_ONLINE_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_online_api_version(void);

typedef struct {
  int64_t num_envs; /* N, 1 .. 2^31 - 1                                      */
  int64_t horizon;  /* T, 1 .. 2^31 - 1; N * T rows per column, below 2^46    */
  int64_t steps;    /* S >= 0: steps inserted so far                          */
  int32_t* ep_seq;  /* [T, N]                                                 */
  int32_t* cur_seq; /* [N]                                                    */
  int64_t* ep_end;  /* [T, N]                                                 */
} ogbx_online_ring;

/* Insert step S = ring->steps (one row per env, num_envs rows) in ONE launch
 * of online_insert_kernel; the caller then counts S + 1.
 *   cols        ogbx_replay_insert_column (ogbx_replay.h): dst is the ring's
 *               column [T * N, row_elems], src (and alt) [N, row_elems]; the
 *               casts, the 1 - value op and alt / alt_select are those of
 *               ogbx_replay_insert.  Row e goes to row (S % T) * N + e.
 *   done        device uint8 [N]: nonzero closes env e's episode at step S
 *               (ep_end[(cur_seq[e] % T) * N + e] = S, cur_seq[e] += 1);
 *               every env's ep_seq[(S % T) * N + e] = cur_seq[e] before that.
 *   alt_select  optional device uint8 [N] (may be `done`); required when any
 *               column has alt.
 * num_cols may be 0 (tables only).  Returns OGBX_EINVAL (message in
 * ogbx_last_error()) before any device work for a NULL ring / table / done /
 * column pointer, num_envs or horizon outside their ranges, steps < 0,
 * num_cols outside 0..OGBX_REPLAY_MAX_COLS, row_elems <= 0 or above 2^19, an
 * unknown dtype or op, or a column with alt but no alt_select.  Pointers are
 * not probed for residency (as ogbx_gc_sample). */
ogbx_status ogbx_online_insert(const ogbx_online_ring* ring, const ogbx_replay_insert_column* cols,
                               int32_t num_cols, const uint8_t* done, const uint8_t* alt_select, void* stream);

/* Zero cur_seq on the stream; the caller restarts its step count at 0.  Rows
 * and the other tables stay: no live row refers to them. */
ogbx_status ogbx_online_clear(const ogbx_online_ring* ring, void* stream);

/* The output batch of one sample call. */
typedef struct {
  const ogbx_gc_column* cols; /* select 0: the sample's row, 2: its value
                                 goal's, 3: its actor goal's (ogbx.h's
                                 numbering; 1, the next row, is refused: the
                                 ring stores its own next_observations)      */
  int32_t num_cols;           /* 0 .. OGBX_REPLAY_MAX_COLS                   */
  int32_t pad_;
  int64_t total;              /* samples                                     */
  int64_t* idxs_out;          /* optional [total], flat indices              */
  int64_t* value_goal_out;    /* optional [total]                            */
  int64_t* actor_goal_out;    /* optional [total]                            */
  double* masks;              /* [total]: 1 - (idx == value goal)            */
  double* rewards;            /* [total]: (idx == value goal) - gc_negative  */
} ogbx_online_batch;

/* GCDataset.sample over the ring's snapshot in ONE launch of
 * online_gc_sample_kernel.  Needs ring->steps >= 1.
 * Per sample: the flat pick u = e * L + k (split with a reciprocal of L that
 * the remainder corrects), the row's ep_seq and its episode's end
 * fin = e * L + (end step - (S - L)), both goals by sample_goals
 * (datasets.py:296-327) on the flat indices, and every selector mapped to its
 * physical row ((S - L + k) % T) * N + e.  The end step is clamped into
 * [row's step, S - 1] and every flat index into [0, L * N), so every physical
 * row lies below T * N whatever the tables and the injected draws hold.
 *   draws   optional injected draws (ogbx.h); draws->idxs are explicit flat
 *           rows, clamped into [0, L * N).
 *   record  optional draw record (ogbx.h).
 * The draw.  No Philox tag or slot of its own: the key and the slot layout are
 * ogbx_gc_sample's over a buffer of L * N rows without valid_idxs, so at one
 * (seed, call) both return the same batch.
 * Returns OGBX_EINVAL before any device work for a NULL ring / cfg / batch /
 * table / masks / rewards / column pointer, a ring outside its ranges,
 * steps < 1, total <= 0, num_cols outside 0..OGBX_REPLAY_MAX_COLS or a bad
 * column descriptor (row_bytes <= 0, select outside {0, 2, 3}, src_stride
 * below row_bytes). */
ogbx_status ogbx_online_gc_sample(const ogbx_online_ring* ring, const ogbx_gc_config* cfg,
                                  const ogbx_online_batch* batch, const ogbx_gc_draws* draws,
                                  const ogbx_gc_draw_record* record, uint64_t seed, uint64_t call_index,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_ONLINE_H_ */
