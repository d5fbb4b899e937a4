/* ogbx_collect.h -- fused point-maze data collection on the device: the
 * episode loop of data_gen_scripts/generate_locomaze.py:142-184 (hliuson/ogbench)
 * for the point agent and its four dataset kinds, k steps of every env per
 * launch, rows written straight into the trajectory-major dataset.
 *
 * An extension of include/ogbx.h exported by the same libogbx.so.  It has its
 * own version (ogbx_collect_abi_version()); OGBX_ABI_VERSION and
 * OGBX_STREAM_VERSION cover ogbx.h alone and are unchanged.  Conventions
 * (status codes, ogbx_last_error(), streams, device pointers) are those of
 * ogbx.h.
 */
#ifndef OGBX_COLLECT_H_
#define OGBX_COLLECT_H_

#include "ogbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OGBX_COLLECT_ABI_VERSION 1
/* Version of this header the loaded library was built from. */
int32_t ogbx_collect_abi_version(void);

/* Dataset kinds (generate_locomaze.py:30-34).  PATH and STITCH differ only in
 * how the caller draws the episode's goal cell; the kernel runs them alike. */
#define OGBX_COLLECT_PATH 0
#define OGBX_COLLECT_NAVIGATE 1
#define OGBX_COLLECT_STITCH 2
#define OGBX_COLLECT_EXPLORE 3

/* One step of one env, t being the episode step (the envs of a handle run in
 * lock step from their reset: elapsed == t for every env, which the caller
 * guarantees by passing t0 = the steps taken since the reset):
 *   rows     observations[row] = qpos[row] = (float)qpos, row = row_offset +
 *            e * row_stride + t
 *   dir      PATH / NAVIGATE / STITCH: (subgoal - xy) / (|subgoal - xy| + 1e-6),
 *            the BFS subgoal of ogbx_maze_oracle_subgoal;
 *            EXPLORE: d / (|d| + 1e-6), d the standard-normal pair of period
 *            t / explore_period.  |v| = sqrt(fma(vy, vy, vx * vx)).
 *   action   a = clip(dir + z, -1, 1) in float64, z the step's N(0, noise)
 *            pair; actions[row] = (float)a
 *   step     ogbx_maze_step with the float64 action a (success timing,
 *            physics and teleports of the handle, the teleport out-portal from
 *            the step's own Philox stream), no auto-reset;
 *            terminals[row] = elapsed + 1 >= max_episode_steps
 *   NAVIGATE on success: goal = ij_to_xy(goal_cells[pick]) (+ r * unit / 4 per
 *            axis under add_noise_to_goal, as ogbx_maze_set_goal); it steers
 *            step t + 1
 * After the launch qpos, goal and elapsed of the handle are those after the
 * chunk's last step: ogbx_maze_step, ogbx_maze_expert_action or another chunk
 * continue from there.
 *
 * Philox words.  The key is (lo32(seed), hi32(seed) ^ 0x4D5A0005), a stream tag
 * of the collector's own; g = env_base + e.  Counters {c0, c1, c2, c3}:
 *   action normal      {lo32(g), t,                  0x61, hi32(g)}
 *       u1 = 1 - u01(x, y), u2 = u01(z, w), r = sqrt(-2 ln u1), a = 2 pi u2,
 *       z = (0.0 + noise * (r cos a), 0.0 + noise * (r sin a))
 *   goal pick          {lo32(g), t,                  0x62, hi32(g)}
 *       pick = mulhi32(x, n_goal_cells)
 *   goal noise         {lo32(g), t,                  0x63, hi32(g)}
 *       r = (-1 + 2 u01(x, y), -1 + 2 u01(z, w))
 *   explore direction  {lo32(g), t / explore_period, 0x64, hi32(g)}
 *       d = (r cos a, r sin a) with u1, u2, r, a as above
 * u01(hi, lo) = ((hi << 32 | lo) >> 11) * 2^-53.  A draw is a function of
 * (seed, g, t) alone: it does not depend on the chunk length, the launch
 * geometry or which envs share a wavefront.  No existing tag or slot moves. */
typedef struct {
  int32_t mode;            /* OGBX_COLLECT_* */
  int32_t explore_period;  /* steps per explore direction, > 0 (10 in the reference) */
  double noise;            /* standard deviation of the action noise, >= 0 */
  const int32_t* goal_cells; /* device int32 [n_goal_cells, 2] (i, j): the cells NAVIGATE
                                resamples from; unused by the other kinds */
  int32_t n_goal_cells;
  int32_t pad;
} ogbx_collect_config;

/* Injected draws (parity mode): every pointer may be NULL (then Philox).  The
 * tape is indexed by position, not consumed: an event at step t reads entry t.
 * N is the handle's batch size. */
typedef struct {
  const double* normal;     /* device f64 [steps, N, 2]: the finished N(0, noise) sample */
  const int32_t* goal_pick; /* device i32 [steps, N], clamped into [0, n_goal_cells) */
  const double* goal_noise; /* device f64 [steps, N, 2]: uniform(-1, 1) */
  const double* dir;        /* device f64 [ceil(steps / explore_period), N, 2]: raw standard normals */
  int64_t steps;            /* episode steps the tape covers; >= t0 + k_steps */
} ogbx_collect_tape;

typedef struct {
  float* observations;   /* device f32 [rows, 2] */
  float* actions;        /* device f32 [rows, 2] */
  uint8_t* terminals;    /* device u8  [rows] */
  float* qpos;           /* device f32 [rows, 2] */
  int64_t row_stride;    /* rows between consecutive envs: the episode length T */
  int64_t row_offset;    /* row of env 0 at t = 0 */
  /* optional diagnostics, step major for the chunk (K = k_steps); may be NULL */
  double* qpos64;        /* device f64 [K, N, 2]: the state before each step */
  double* goal64;        /* device f64 [K, N, 2]: the goal before each step */
  uint8_t* success;      /* device u8  [K, N] */
} ogbx_collect_outputs;

/* Advance every env of a point handle by k_steps steps of its episode, steps
 * t0 .. t0 + k_steps - 1, in one launch.  Asynchronous on `stream`; makes no
 * allocation.  `seed` keys the draws above (the teleport draw keeps the seed of
 * the handle's reset).
 * OGBX_EINVAL (message in ogbx_last_error()) before any device work: a NULL
 * handle, cfg or out; a handle that is not a point handle or was created with
 * terminate_at_goal != 0; a NULL dataset column; k_steps <= 0 or t0 < 0; a chunk
 * past the time limit (t0 + k_steps > max_episode_steps) or past row_stride or
 * past tape->steps; a negative row_offset; an unknown mode; explore_period <= 0;
 * noise < 0 or not finite; NAVIGATE without goal cells.  OGBX_ESTATE before the
 * handle's first reset. */
ogbx_status ogbx_maze_collect(ogbx_maze_t env, const ogbx_collect_config* cfg, const ogbx_collect_tape* tape,
                              int32_t t0, int32_t k_steps, uint64_t seed, const ogbx_collect_outputs* out,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OGBX_COLLECT_H_ */
