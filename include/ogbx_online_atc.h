/* ogbx_online_atc.h -- ATC batches over the on-device episode ring: what
 * ATCDataset.sample(B, k) (hliuson/ogbench impls/utils/datasets.py:369-464)
 * returns over the snapshot of a ring of include/ogbx_online.h -- anchor /
 * positive observation pairs (o_t, o_{t+k}) of one episode, frame stacked and
 * randomly cropped -- with every live row a candidate (the ring has no
 * `valids`) and `next_observations` never read.
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_online_atc_api_version()); no other version moves.
 * Conventions (status codes, ogbx_last_error(), streams, device pointers) are
 * those of ogbx.h; the ring is ogbx_online.h's, the column, the outputs and
 * the Philox words are ogbx_atc.h's, the frame stack over the ring is
 * ogbx_online_visual.h's.
 *
 * The anchor table.  Over the snapshot (ogbx_online.h: flat index
 * u = e * L + o, L = min(S, T) live steps, t0 = S - L) valid(k) holds the rows
 * whose offset + k stays inside their episode.  Per env e, with seq0 and seqn
 * the ep_seq at steps t0 and S - 1 (ordinals differ in uint32, as the insert
 * counts them):
 *   c = clamp(seqn - seq0, 0, L - 1)   episodes closed before the newest row
 *   the env has c + 1 live segments i = 0..c; segment i < c ends at offset
 *     E_i = ep_end[((seq0 + i) % T) * N + e] - t0,  segment c at L - 1;
 *     b_0 = 0, b_{i+1} = E_i + 1, len_i = E_i - b_i + 1, E_i clamped into
 *     [b_i, L - 1] whatever the table holds
 *   w_i = max(len_i - k, 0)            anchors of segment i: b_i .. E_i - k
 *   W_i = sum of w_j over j < i,  A[e] = W_c + w_c
 * P, int64 [N + 1], is the exclusive prefix sum of A; P[N] is the size of
 * valid(k).  The table of rows is never materialised.  Pick j in [0, P[N]):
 *   1. the env e with P[e] <= j < P[e + 1]            (a search over P)
 *   2. the rank r = j - P[e]
 *   3. the largest i in [0, c] with W_i <= r          (a search over W)
 *   4. the anchor offset o = b_i + (r - W_i); the positive is o + k, in the
 *      same segment.
 * The picks in order are the reference's valid_idxs over the snapshot.
 */
#ifndef OGBX_ONLINE_ATC_H_
#define OGBX_ONLINE_ATC_H_

#include <stddef.h>

#include "ogbx.h"
#include "ogbx_atc.h"
#include "ogbx_online.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_ONLINE_ATC_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_online_atc_api_version(void);

/* Envs that one workgroup of the table scan covers (a scan over more envs
 * carries its running sum from workgroup to workgroup). */
#define OGBX_ONLINE_ATC_TABLE_TILE 2048

/* Bytes of temporary device storage ogbx_online_atc_table needs for a ring of
 * num_envs envs (the per-env counts A and the scan's own storage), to *bytes
 * (at least 1).  The caller allocates it once. */
ogbx_status ogbx_online_atc_table_bytes(int64_t num_envs, size_t* bytes);

/* Build W and P (above) for the ring's current `steps` and this k: one launch
 * of online_atc_count_kernel (one wave per env over its live segments) and
 * one device-wide exclusive scan, on the stream.
 *   W   device int32 [T, N], indexed like ep_end by (ordinal % T) * N + e: W_i
 *       of the env's live segments (c + 1 <= T of them, distinct mod T); the
 *       other entries are left as they are.
 *   P   device int64 [N + 1].
 *   temp, temp_bytes  device storage of at least ogbx_online_atc_table_bytes
 *       bytes, 8-byte aligned, owned by the caller; nothing is allocated or
 *       read back by the call.
 * Needs ring->steps >= 1.  Call it again after every insert, clear or change
 * of k before the next ogbx_online_atc_sample.  Returns OGBX_EINVAL before any
 * device work for a NULL ring / table / W / P / temp, a ring outside its
 * ranges, steps < 1, k < 0 or temp_bytes below the need. */
ogbx_status ogbx_online_atc_table(const ogbx_online_ring* ring, int64_t k, int32_t* W, int64_t* P, void* temp,
                                  size_t temp_bytes, void* stream);

/* ATCDataset.sample over the ring's snapshot in ONE launch of
 * online_atc_sample_kernel: one workgroup per (sample, side), side = anchor or
 * positive, both workgroups of a sample on one XCD (ogbx_atc_sample's layout).
 * Needs ring->steps >= 1 and W, P built by ogbx_online_atc_table for these
 * `steps` and this k.
 *
 * The anchor of sample s, in this order of precedence:
 *   idxs[s]            when idxs is non-NULL (device int64 [total]), a flat row;
 *   else pick[s]       when pick is non-NULL (device int64 [total], positions
 *                      into valid(k)), through the select above;
 *   else the Philox pick, through the select above.
 *   col          ogbx_atc_column (ogbx_atc.h): src is the ring's observations
 *                column ([T * N, height, width, px_bytes], unstacked).  Channel
 *                block j of a side at offset o of env e is the frame at offset
 *                max(o - (F-1-j), o0), o0 the earliest of o - (F-1) .. o that
 *                is live and of o's episode (ogbx_online_visual.h).
 *   frame_stack, padding, crop_from, draw_crop   as ogbx_atc_sample.
 *   out          ogbx_atc_outputs (ogbx_atc.h); every index is a flat index.
 *                bad_count counts the explicit rows whose index leaves the
 *                snapshot or whose idx + k leaves their episode, and every
 *                sample drawn (by pick or Philox) when P[N] == 0.
 * The draw.  The key and the slots are exactly ogbx_atc_sample's over a table
 * of P[N] entries, P[N] read on the device (the ATC stream tag; the pick from
 * slot 0, words x, y: mulhi64(., max(P[N], 1)); the crop from
 * OGBX_VISUAL_CROP_SLOT): at one (seed, call) the batch equals the offline
 * sampler's over the snapshot, and no existing stream moves.
 * Memory safety.  A pick is clamped into [0, max(P[N], 1)), the env into
 * [0, N), every offset, stack row and positive into [0, L - 1] and every flat
 * index into [0, L * N); every table index is reduced mod T, so every physical
 * row lies below T * N whatever W, P, the tables and the injected values hold.
 * Returns OGBX_EINVAL (message in ogbx_last_error()) before any device work
 * for a NULL ring / table / W / P / col / column pointer, a ring outside its
 * ranges, steps < 1, non-positive sizes, k < 0, frame_stack outside
 * 1..OGBX_VISUAL_MAX_STACK, a negative padding, a crop_from output without
 * crop offsets, an image too large or too wide to stage, too many samples for
 * one launch, or a pointer that is not device memory of the current device. */
ogbx_status ogbx_online_atc_sample(const ogbx_online_ring* ring, int64_t k, const int32_t* W, const int64_t* P,
                                   const ogbx_atc_column* col, int64_t total, int32_t frame_stack, int32_t padding,
                                   const int64_t* idxs, const int64_t* pick, const int64_t* crop_from,
                                   int32_t draw_crop, uint64_t seed, uint64_t call_index,
                                   const ogbx_atc_outputs* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_ONLINE_ATC_H_ */
