/* ogbx_online_trl.h -- TRL batches over the on-device episode ring: what
 * GCDataset.sample returns with a TRL agent name (hliuson/ogbench
 * impls/utils/datasets.py:198-204, 254-276) over the snapshot of a ring of
 * include/ogbx_online.h -- picks only among the rows that are not the last of
 * their trajectory, and the value-midpoint keys of include/ogbx_trl.h.
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_online_trl_api_version()); no other version moves.
 * Conventions (status codes, ogbx_last_error(), streams, device pointers) are
 * those of ogbx.h; the ring is ogbx_online.h's, the outputs, the midpoint
 * selector and the Philox words are ogbx_trl.h's.
 *
 * The pick table.  Over the snapshot (ogbx_online.h: flat index u = e * L + k,
 * L = min(S, T) live steps, t0 = S - L) the terminal rows of env e are the
 * last rows of the episodes it closed before its newest row, and the newest
 * row itself.  With seq0[e] = ep_seq at step t0 and seqn[e] = ep_seq at step
 * S - 1 (ordinals differ in uint32, as the insert counts them) env e closed
 * m = seqn - seq0 episodes before its newest row and holds
 *   V[e] = L - 1 - m
 * pickable rows.  P, int64 [N + 1], is the exclusive prefix sum of V; P[N] is
 * the size of the pick table (the reference's len(valid_idxs)).  The table is
 * never materialised.  Pick j in [0, P[N]) is selected in closed form:
 *   1. the env e with P[e] <= j < P[e + 1]             (a search over P)
 *   2. the rank r = j - P[e] among the env's pickable rows
 *   3. the smallest i in [0, m) with
 *        G(i) = ep_end[((seq0 + i) % T) * N + e] - t0 - i  >  r,
 *      i = m if there is none: i terminal rows lie before the pick, and
 *      k = r + i.  G(i) counts the pickable rows before the terminal of the
 *      env's i-th live closed episode; it does not decrease in i.
 * The search of step 3 is over the env's live closed episodes, at most
 * log2(L) + 1 dependent loads.  The episode of the picked row is ordinal
 * seq0 + i, so its end needs no load of the row's ep_seq.
 */
#ifndef OGBX_ONLINE_TRL_H_
#define OGBX_ONLINE_TRL_H_

#include <stddef.h>

#include "ogbx.h"
#include "ogbx_online.h"
#include "ogbx_trl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_ONLINE_TRL_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_online_trl_api_version(void);

/* Envs that one workgroup of the table scan covers (a scan over more envs
 * carries its running sum from workgroup to workgroup). */
#define OGBX_ONLINE_TRL_TABLE_TILE 2048

/* Bytes of temporary device storage ogbx_online_trl_table needs for a ring of
 * num_envs envs, to *bytes (at least 1).  The caller allocates it once. */
ogbx_status ogbx_online_trl_table_bytes(int64_t num_envs, size_t* bytes);

/* Write the exclusive prefix sum of V (above) for the ring's current `steps`
 * to P, device int64 [num_envs + 1]: one device-wide scan on the stream whose
 * input is computed from the two ep_seq rows of steps S - L and S - 1 (both
 * contiguous in e).  V is clamped into [0, L - 1] whatever the rows hold.
 *   temp, temp_bytes  device storage of at least ogbx_online_trl_table_bytes
 *                     bytes, owned by the caller; nothing is allocated or read
 *                     back by the call.
 * Needs ring->steps >= 1.  Call it again after every insert or clear before
 * the next ogbx_online_trl_sample.  Returns OGBX_EINVAL before any device work
 * for a NULL ring / table / P / temp, a ring outside its ranges, steps < 1 or
 * temp_bytes below the need. */
ogbx_status ogbx_online_trl_table(const ogbx_online_ring* ring, int64_t* P, void* temp, size_t temp_bytes,
                                  void* stream);

/* GCDataset.sample with the TRL branch over the ring's snapshot in ONE launch
 * of online_trl_sample_kernel.  Needs ring->steps >= 1 and P built by
 * ogbx_online_trl_table for these `steps`.
 *
 * Per sample: the pick and the actor side's random goal go through the select
 * above (two independent chains, issued interleaved); the value side draws no
 * random goal (cfg forbids it) and skips its select.  The episode end, both
 * goals and the midpoint follow as in ogbx_online_gc_sample / ogbx_trl_sample
 * on flat indices, and every selector is mapped to its physical row.
 *   cols      up to 32 columns over the ring's columns ([T * N, ...]); select
 *             0 the sample's row, 1 flat min(u + 1, L * N - 1), 2 / 3 the value
 *             / actor goal, OGBX_TRL_SELECT_MIDPOINT the midpoint.
 *   total     samples.
 *   draws     optional injected draws (ogbx.h): pick / a_pick index the pick
 *             table, draws->idxs are explicit flat rows.
 *   midpoint  NULL, or device int64 [total]: the midpoint's raw flat row.
 *   out       ogbx_trl_outputs (ogbx_trl.h); every index is a flat index.
 *             bad_count counts the samples whose value goal is <= idx, and
 *             every sample when P[N] == 0; such a sample gets mid = idx.
 *   record, midpoint_record   as ogbx_trl_sample.
 * The draw.  The key, the slot layout and the midpoint words are exactly
 * ogbx_trl_sample's over a pick table of P[N] entries (GC stream tag, slots
 * 0..4, midpoint from words z, w of slot 4), P[N] read on the device: at one
 * (seed, call) the batch equals the offline TRL sampler's over the snapshot.
 * Memory safety.  A pick is clamped into [0, max(P[N], 1)), the env into
 * [0, N), k into [0, L - 1] and every flat index into [0, L * N); every table
 * index is reduced mod T, so every physical row lies below T * N whatever P,
 * the tables and the injected values hold.
 * Returns OGBX_EINVAL before any device work for a NULL ring / cfg / out / P /
 * table / column pointer, a ring outside its ranges, steps < 1, total <= 0,
 * num_cols outside 0..32, a bad column descriptor (row_bytes <= 0, select
 * outside 0..4, src_stride below row_bytes), an incomplete draw record, a
 * pointer that is not device memory of the current device, or a cfg with
 * value_p_curgoal != 0 or a value trajectory threshold below 1. */
ogbx_status ogbx_online_trl_sample(const ogbx_online_ring* ring, const int64_t* P, const ogbx_gc_config* cfg,
                                   const ogbx_gc_column* cols, int32_t num_cols, int64_t total,
                                   const ogbx_gc_draws* draws, const int64_t* midpoint, uint64_t seed,
                                   uint64_t call_index, const ogbx_trl_outputs* out,
                                   const ogbx_gc_draw_record* record, int64_t* midpoint_record, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_ONLINE_TRL_H_ */
