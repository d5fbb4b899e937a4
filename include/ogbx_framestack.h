/* ogbx_framestack.h -- frame stacks of batched env observations, composed on
 * the device: FrameStackWrapper of impls/utils/env_utils.py:48-76
 * (hliuson/ogbench) for every env of a batch in one launch per step.
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_framestack_abi_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h.
 *
 * Layout.  An observation is n envs x `pixels` P x `elem_bytes` E, E being the
 * last axis in bytes (powderworld [N,H,W,6] u8: P = H*W, E = 6; point maze
 * [N,2] f64: P = 1, E = 16; ant [N,29] f64: P = 1, E = 232).  A stack is
 * n x P x k x E bytes, k = num_stack, slot k-1 the newest frame: the
 * concatenate(frames, axis=-1) of the reference.
 *
 * There is no handle: the calls are stateless, asynchronous on `stream`,
 * allocate nothing and read nothing back.
 *
 * Alignment.  The stacks (`stack`, `prev`, `next`, `final_stack`) must start
 * on a 16-byte boundary (any torch allocation does); an env's row inside them
 * may start anywhere.  `obs` and `final_obs` may start at any byte.
 */
#ifndef OGBX_FRAMESTACK_H_
#define OGBX_FRAMESTACK_H_

#include "ogbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_FRAMESTACK_ABI_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_framestack_abi_version(void);

typedef struct {
  int64_t n;          /* envs, >= 0 (0: nothing is launched) */
  int64_t pixels;     /* P >= 1: product of the axes between the env axis and the last */
  int64_t elem_bytes; /* E >= 1: bytes of the last axis of one frame */
  int32_t num_stack;  /* k >= 1 */
  int32_t pad;
} ogbx_framestack_shape;

/* FrameStackWrapper.reset (and its goal tiling): for every env, or only those
 * with mask[e] != 0 when `mask` (device u8 [n]) is non-NULL, all k slots of
 * stack[e] become obs[e].  Rows of the other envs are untouched.
 * OGBX_EINVAL as for ogbx_framestack_push. */
ogbx_status ogbx_framestack_fill(const ogbx_framestack_shape* shape, const void* obs, const uint8_t* mask,
                                 void* stack, void* stream);

/* FrameStackWrapper.step, out of place: `prev` is read, `next` is written, the
 * caller alternates two buffers.  done = terminated | truncated, each a
 * nullable device u8 [n].
 *   env not done (or both masks NULL):
 *     next[e,p] = prev[e,p,1:] || obs[e,p]
 *   env done:
 *     next[e,p] = k copies of obs[e,p] (with same-step auto-reset obs is the
 *       new episode's first observation)
 *     final_stack[e,p] = prev[e,p,1:] || final_obs[e,p] when final_stack is
 *       non-NULL: what the reference's step returned before its reset
 * Every row of `next` is written; final_stack rows of envs that are not done
 * are not written (as final_obs of ogbx_maze_step).
 *
 * OGBX_EINVAL (message in ogbx_last_error()) before any device work: a NULL
 * shape, obs, prev or next (fill: shape, obs or stack); n < 0, pixels < 1,
 * elem_bytes < 1 or num_stack < 1; byte counts that do not fit int64;
 * final_stack without final_obs, or final_stack with both masks NULL; a stack
 * that does not start on a 16-byte boundary; an output range that overlaps an
 * input range or the other output; then, with a device, a pointer that is not
 * memory of the current device.  n == 0 returns OGBX_OK without a launch. */
ogbx_status ogbx_framestack_push(const ogbx_framestack_shape* shape, const void* obs, const void* prev,
                                 const uint8_t* terminated, const uint8_t* truncated, const void* final_obs,
                                 void* next, void* final_stack, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_FRAMESTACK_H_ */
