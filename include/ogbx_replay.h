/* ogbx_replay.h -- an on-device replay buffer: batched ring inserts of the
 * transitions a vectorized env produced, and uniform sampling over the rows
 * held so far (hliuson/ogbench impls/utils/datasets.py:86-146, ReplayBuffer;
 * used by data_gen_scripts/main_sac.py:66-137).
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_replay_api_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h.
 *
 * The header.  `pointer` (the next slot written) and `size` (the rows that
 * sample draws from) live on the device, in OGBX_REPLAY_HEADER_WORDS int64
 * words owned by the caller and zeroed before the first call:
 *   header[2 p + 0] = pointer, header[2 p + 1] = size      p = 0, 1
 * Two copies, because an insert's workgroups read the old pointer while one
 * of them writes the new one: an insert called with `parity` p reads copy p
 * and writes copy 1 - p.  The caller flips its parity after every insert (and
 * only then) and passes the current parity to the next insert or sample.  No
 * entry point reads anything back to the host.
 *
 * The ring, as N sequential add_transition calls in row order give it
 * (datasets.py:134-142): with M rows kept of the n offered,
 *   the j-th kept row lands at slot (pointer + j) % max_size
 *   pointer' = (pointer + M) % max_size
 *   size'    = max(size, min(pointer + M, max_size - 1))
 * The last line is the reference's: it takes size = max(pointer, size) after
 * the modulo, so size stops at max_size - 1 and the buffer's last row is
 * never drawn.  (Exactly: size' = max(size, the largest pointer value the M
 * adds visit), which is the line above in every state the ring reaches by
 * itself, size >= pointer; M = 0 changes nothing.)
 * The header must hold pointer < max_size (a buffer filled to
 * max_size by the caller cannot take inserts; the reference raises there).
 */
#ifndef OGBX_REPLAY_H_
#define OGBX_REPLAY_H_

#include "ogbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_REPLAY_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_replay_api_version(void);

#define OGBX_REPLAY_MAX_COLS 16
#define OGBX_REPLAY_HEADER_WORDS 4

/* Element types of an insert column's source and destination. */
typedef enum {
  OGBX_REPLAY_BOOL = 0, /* source only: one byte, nonzero = 1                 */
  OGBX_REPLAY_U8 = 1,
  OGBX_REPLAY_I32 = 2,
  OGBX_REPLAY_I64 = 3,
  OGBX_REPLAY_F32 = 4,
  OGBX_REPLAY_F64 = 5
} ogbx_replay_dtype;

typedef enum {
  OGBX_REPLAY_OP_NONE = 0,
  OGBX_REPLAY_OP_ONE_MINUS = 1 /* dst = 1 - value, in the destination type,
                                  after the cast                               */
} ogbx_replay_op;

/* One column of an insert.  dst is the buffer's column, dense
 * [max_size, row_elems] of dst_dtype; src is dense [n, row_elems] of
 * src_dtype.  alt (optional, same type and shape as src): row i is read from
 * alt instead of src where the call's alt_select[i] is nonzero.
 * Values are converted as a NumPy assignment converts them, for in-range
 * values: integer -> float and float64 -> float32 round to nearest even,
 * float -> integer truncates toward zero, integer -> narrower integer wraps.
 * With equal types (or BOOL -> U8) and no op, rows move as bytes, in the
 * widest unit (16 / 8 / 4 / 1 bytes) the row size and the pointers allow. */
typedef struct {
  void* dst;
  const void* src;
  const void* alt;
  int64_t row_elems;
  int32_t src_dtype; /* ogbx_replay_dtype                                   */
  int32_t dst_dtype; /* ogbx_replay_dtype but BOOL                           */
  int32_t op;        /* ogbx_replay_op                                       */
  int32_t pad_;
} ogbx_replay_insert_column;

/* Insert n rows (one per env) of num_cols columns in ONE launch of
 * replay_insert_kernel.
 *   keep        optional device uint8 [n]: only rows with a nonzero byte are
 *               inserted, in row order (a row's slot is its rank among them);
 *               NULL keeps every row.  All zero leaves the header's values
 *               unchanged (they are still copied to the other parity).
 *   alt_select  optional device uint8 [n], see ogbx_replay_insert_column.alt;
 *               required when any column has alt.
 * Returns OGBX_EINVAL (message in ogbx_last_error()) before any device work
 * for a NULL header / cols / column pointer, n <= 0, max_size <= 0,
 * n > max_size (two rows of one launch would race for one slot),
 * row_elems <= 0 or above 2^19 (a row of more than 4 MiB), num_cols outside
 * 1..OGBX_REPLAY_MAX_COLS, parity outside
 * {0, 1}, an unknown dtype or op, a column with alt but no alt_select, or a
 * pointer that is not device memory of the current device. */
ogbx_status ogbx_replay_insert(int64_t* header, int32_t parity, int64_t max_size,
                               const ogbx_replay_insert_column* cols, int32_t num_cols, int64_t n,
                               const uint8_t* keep, const uint8_t* alt_select, void* stream);

/* Reset pointer and size to 0 (both parities), on the stream. */
ogbx_status ogbx_replay_clear(int64_t* header, void* stream);

/* Dataset.sample / get_subset over rows [0, size) (datasets.py:65-83) in ONE
 * launch of replay_sample_kernel; size is read from header copy `parity`.
 *   cols        ogbx_gc_column descriptors (ogbx.h): select 0 gathers row
 *               idx, select 1 row next = max(min(idx + 1, size - 1), 0), the
 *               compact layout's next observation (clamped at the CURRENT
 *               size - 1, not at max_size - 1).
 *   idxs        optional device int64 [total]: explicit rows, clamped into
 *               [0, max_size); NULL draws them.
 * The draw.  No Philox tag or slot of its own: key
 *   (lo32(seed), hi32(seed) ^ 0x47430001), the GC sampler's; counter
 *   {sample_lo, call_lo, 0, sample_hi ^ call_hi}; idx = mulhi64((x << 32) | y,
 *   size) -- the index draw of ogbx_gc_sample over a buffer of `size` rows
 *   without valid_idxs, so at one (seed, call) both return the same rows.
 *   idxs_out    optional device int64 [total]: the rows used.
 *   empty_count optional device int64, zeroed by the caller once: when
 *               size == 0 every drawn sample reads row 0 (and next row 0) and
 *               the kernel adds `total` to it (with explicit idxs too, whose
 *               rows are read as given).  Nothing is read out of bounds.
 * Returns OGBX_EINVAL before any device work for a NULL header / cols /
 * column pointer, total <= 0, max_size <= 0, num_cols outside
 * 1..OGBX_REPLAY_MAX_COLS, a bad column descriptor (row_bytes <= 0, select
 * outside {0, 1}, src_stride below row_bytes), parity outside {0, 1}, or a
 * pointer that is not device memory of the current device. */
ogbx_status ogbx_replay_sample(const int64_t* header, int32_t parity, int64_t max_size,
                               const ogbx_gc_column* cols, int32_t num_cols, int64_t total,
                               const int64_t* idxs, uint64_t seed, uint64_t call_index, int64_t* idxs_out,
                               int64_t* empty_count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_REPLAY_H_ */
