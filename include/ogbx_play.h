/* ogbx_play.h -- powderworld play-data collection on the device: the
 * data-collection mode of the powderworld envs and the open-loop action plan
 * of the play policy (hliuson/ogbench ogbench/powderworld/powderworld_env.py
 * :284-427 with mode='data_collection', ogbench/powderworld/behaviors.py,
 * data_gen_scripts/generate_powderworld.py:49-81).
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_play_api_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h.
 */
#ifndef OGBX_PLAY_H_
#define OGBX_PLAY_H_

#include "ogbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_PLAY_API_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_play_api_version(void);

/* ---------------------------------------------------------------- data mode
 * A handle learns its mode at ogbx_powder_create from the `pad` word of
 * ogbx_powder_opts (layout unchanged): 0 = task mode, as ever;
 * OGBX_POWDER_MODE_DATA = data collection.  Any other value is OGBX_EINVAL.
 *
 * A data-mode handle has no task and no goal: its success tolerances are 0, so
 * the goal-match count of a step (>= 0) is never below them.  ogbx_powder_step
 * then reports reward 0, terminated 0 and success 0 for every env and step,
 * and truncated from the TimeLimit; the three-stage action protocol, the
 * forward and the paint are those of task mode.  ctrl keeps task index 1 (a
 * valid index: no kernel forms a pointer from a task of 0); medium/hard goal
 * ids are zeroed by the reset.  ogbx_powder_describe reports tol = 0.
 * ogbx_powder_reset on a data-mode handle, ogbx_play_powder_reset on a
 * task-mode handle and ogbx_powder_step(auto_reset != 0) on a data-mode handle
 * are OGBX_EINVAL: collection runs lock-step rounds. */
#define OGBX_POWDER_MODE_DATA 1

/* PowderworldEnv.reset in data-collection mode for every env (or the envs with
 * mask[e] != 0; mask: device uint8 [N] or NULL): an empty world with a wall
 * border, stage 0, elapsed 0, episode + 1; medium/hard: zero momentum and
 * velocity, a fresh render cache, and phase 0 of the step schedule after an
 * unmasked reset.  No draw is made; `seed` keys the Philox streams of later
 * steps (the replacement of invalid actions, the medium/hard rand fields), as
 * the seed of ogbx_powder_reset does.  obs: device uint8 [N, H, W, 6], the
 * render of the new world with an empty action frame (rows of masked-out envs
 * are not written). */
ogbx_status ogbx_play_powder_reset(ogbx_powder_t env, const uint8_t* mask, uint8_t* obs, uint64_t seed,
                                   void* stream);

/* ---------------------------------------------------------------- action plan
 * The play policy is open loop (Behavior.select_action ignores ob and info),
 * so ogbx_play_plan writes the actions of a whole episode of every env in ONE
 * launch, before any world is stepped: actions int32 [T, N], step major, the
 * layout ogbx_powder_step(k_steps = K) reads.  One lane per env; every
 * behaviour's sequence is a closed form of its step index (no table).
 *
 * The episode of one env (generate_powderworld.py:49-81), `pop` being the next
 * draw:
 *   choose: u = pop; kind = #{k : cdf[k] <= u}, at most 2 (0 Fill, 1 Line,
 *           2 Square: np.random.choice(agents, p=probs)); then the reset draws
 *     Fill    elem, flip_x, flip_y, flip_xy             size * size entries
 *             entry i: x = i % size, y = i / size; flip_x: x = size-1-x;
 *             flip_y: y = size-1-y; flip_xy: swap
 *     Line    elem, target in [0, size), flip_dir, flip_xy      size entries
 *             entry i: x = i, y = target; flip_dir: y = size-1-y; flip_xy: swap
 *     Square  elem, length in [1, size-1], x1 and y1 in [0, size-length),
 *             reverse bit of side 0..3, then j3 in [0,3], j2 in [0,2], j1 in
 *             [0,1]: perm = (0,1,2,3); swap perm[3], perm[j3]; swap perm[2],
 *             perm[j2]; swap perm[1], perm[j1] (np.random.shuffle of a 4-list)
 *             4 (length + 1) entries; entry s: side perm[s / (length+1)], offset
 *             o = s % (length+1), o = length - o if the side is reversed;
 *             side 0 (x1, y1+o), 1 (x1+length, y1+o), 2 (x1+o, y1),
 *             3 (x1+o, y1+length)
 *   step t, stage t % 3:
 *     stage 0 (a decision): u = pop; u < p_random: the held semantic action is
 *       elem, x, y = three pops (sample_semantic_action) and the behaviour does
 *       not advance; else it is the behaviour's element and next entry, and
 *       the behaviour is done after its last entry.  actions[t] = elem index;
 *       a done behaviour is replaced now (choose, above).
 *     stage 1: actions[t] = held x.   stage 2: actions[t] = held y.
 *
 * Philox words.  The key is (lo32(seed), hi32(seed) ^ 0x504C0001), a stream tag
 * of the plan's own; the counter is {lo32(g), episode, pop index, hi32(g)} with
 * g = env_base + e and pop index 0, 1, 2, ... in the order above.  Of the four
 * words of a pop:
 *   uniform (choose, decision)   u01(x, y) = ((x << 32 | y) >> 11) * 2^-53
 *   integer in [lo, lo + n)      lo + mulhi32(x, n)
 * No existing tag or slot moves.  An env's plan is a function of (seed, g,
 * episode) alone: it does not depend on N or on which envs share a wavefront,
 * and a shard with env_base = b reproduces rows b.. of the one-device plan. */
typedef struct {
  int32_t size;      /* world_size / brush_size (brush_size == grid_size), 2..64 */
  int32_t num_elems; /* 1..64 */
  int32_t xy_size;   /* _xy_action_size, 1..256 */
  int32_t pad;
  double p_random;   /* p_random_action, in [0, 1] */
  double cdf[3];     /* normalised cumulative behaviour weights, nondecreasing,
                        cdf[2] == 1 ((1, 3, 3) / 7 in the reference) */
  int64_t env_base;  /* global index of env 0 */
  int64_t episode;   /* Philox counter word 1 (low 32 bits) */
} ogbx_play_config;

/* Injected draws (parity mode), NULL for Philox.  tape: device float64 [N,
 * tape_len], per env the values the reference drew, in the order above;
 * integers as exact doubles (elements as their index); a uniform as itself.
 * Every pop takes the env's next value (an integer is clamped into its range).
 * short_count: one device int64, zeroed by the caller; the kernel adds 1 for
 * every env whose tape ran out.  Such an env pops 0 from then on; nothing is
 * read past its row. */
typedef struct {
  const double* tape;
  int64_t tape_len;
  int64_t* short_count;
} ogbx_play_tape;

/* Optional outputs; every pointer may be NULL.
 * decisions: one word per decision (stage-0 step) d = t / 3:
 *   bit 0     1 = random semantic action, 0 = the behaviour's entry
 *   bits 1-2  kind of the env's behaviour at the decision (0, 1, 2)
 *   bit 3     1 = that behaviour was chosen since the previous decision
 *             (at the episode's start or as a replacement)
 *   bits 8..  the behaviour's step counter before the decision (the index of
 *             the entry used, when bit 0 is 0) */
typedef struct {
  int32_t* used;      /* [N] pops consumed (with a tape: values of its row used) */
  int32_t* decisions; /* [(T + 2) / 3, N] */
  uint8_t* terminals; /* [T] t == T - 1 */
} ogbx_play_outputs;

/* Returns OGBX_EINVAL (message in ogbx_last_error()) before any device work
 * for a NULL cfg / actions, n_envs <= 0, T <= 0, p_random outside [0, 1], sizes
 * outside the ranges above, a bad cdf, env_base < 0, a tape with tape_len <= 0
 * or without short_count, or a pointer that is not device memory of the current
 * device. */
ogbx_status ogbx_play_plan(const ogbx_play_config* cfg, int64_t n_envs, int32_t T, int32_t* actions,
                           const ogbx_play_tape* tape, const ogbx_play_outputs* out, uint64_t seed,
                           void* stream);

/* Batched PowderworldEnv.sample_semantic_action (:446-451): out int32 [N, 3] =
 * (elem index, x, y).  Philox: the plan's key; counter {lo32(g), lo32(call),
 * 0x80000000, hi32(g)} (a slot no pop index reaches: T < 2^31 / 3); elem =
 * mulhi32(x, num_elems), x = mulhi32(y, xy_size), y = mulhi32(z, xy_size). */
ogbx_status ogbx_play_sample_semantic(int32_t num_elems, int32_t xy_size, int64_t n_envs, int64_t env_base,
                                      uint64_t seed, uint64_t call_index, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_PLAY_H_ */
