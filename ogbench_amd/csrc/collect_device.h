// collect_device.h -- maze_collect_kernel: the episode loop of
// data_gen_scripts/generate_locomaze.py:142-184 (hliuson/ogbench) for the point
// agent, k steps of every env in one launch (include/ogbx_collect.h).  Included
// by locomaze.hip after the helpers it reuses: subgoal_of and the arithmetic of
// expert_action_kernel, point_step_as, goal_within / goal_reached and the
// teleport block of maze_step_kernel, the arithmetic of set_goal_kernel.  A
// fused step therefore computes bit for bit what the launches expert_action ->
// step (float64 action) -> set_goal compute.
//
// One lane per env, 64 envs per wave; qpos, goal and elapsed stay in registers
// across the chunk, and every step writes its dataset row in its final
// trajectory-major place (row_offset + e * row_stride + t): no staging tensor.
// A step's dependent physics chain is microseconds long, so the scattered
// 8-byte row stores are written directly.
//
// Philox streams: key seed_key(seed, kTagMazeCollect); counter
//   {lo32(g), c1, domain, hi32(g)},  g = env_base + e
//   domain kCollectNormal  c1 = t           the step's N(0, noise) pair (Box-Muller)
//   domain kCollectPick    c1 = t           word x -> goal cell index
//   domain kCollectGNoise  c1 = t           words (x, y), (z, w) -> goal noise
//   domain kCollectDir     c1 = t / period  the period's standard-normal pair
// t is the episode step.  Nothing depends on the chunk length, the launch
// geometry or which envs share a wave.  The teleport draw is the step's own
// (key of the handle's reset seed ^ kTagMazeTeleport, counter slot 0x100 + el).
#pragma once

#include "../../include/ogbx_collect.h"

namespace ogbx {

constexpr uint32_t kTagMazeCollect = 0x4D5A0005u;
constexpr uint32_t kCollectNormal = 0x61u, kCollectPick = 0x62u, kCollectGNoise = 0x63u, kCollectDir = 0x64u;

struct CollectArgs {
  const MazeParams* Pp;
  const int16_t* bfs;
  MazeStepConsts C;
  MazeState S;
  int64_t n;
  ogbx_collect_config cfg;
  ogbx_collect_tape tape;  // pointers all NULL without a tape
  ogbx_collect_outputs out;
  int32_t t0, k_steps;
  uint32_t k0, k1;    // the collector's key
  uint32_t sk0, sk1;  // the step's key (teleports)
};

// The standard-normal pair of one Philox call (the Box-Muller form of
// expert_action_kernel): (r cos a, r sin a).
__device__ inline void collect_box_muller(const u32x4 w, double* c, double* s) {
  const double u1 = 1.0 - u01_from(w.x, w.y);  // (0, 1]
  const double u2 = u01_from(w.z, w.w);
  const double r = sqrt(-2.0 * log(u1));
  const double a = 6.283185307179586 * u2;
  *c = r * cos(a);
  *s = r * sin(a);
}

// kMode: OGBX_COLLECT_PATH (also STITCH), _NAVIGATE or _EXPLORE.
template <int kMode>
__global__ void __launch_bounds__(256) maze_collect_kernel(const CollectArgs A) {
  static_assert(kMode == OGBX_COLLECT_PATH || kMode == OGBX_COLLECT_NAVIGATE || kMode == OGBX_COLLECT_EXPLORE,
                "STITCH runs the PATH instantiation");
  const MazeParams& P = *A.Pp;
  OGBX_POINT_MODEL(pm, P);
  const MazeStepConsts& C = A.C;
  __shared__ uint16_t nb_s[kMaxCells];
  __shared__ uint8_t wall_s[kMaxCells];
  // one table entry per thread of the 256-thread block
  nb_s[threadIdx.x] = P.nbmask[threadIdx.x];
  wall_s[threadIdx.x] = P.wall[threadIdx.x];
  __syncthreads();
  const int64_t n = A.n;
  const int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t gi = (uint64_t)(i + C.env_base);
  const uint32_t g_lo = (uint32_t)gi, g_hi = (uint32_t)(gi >> 32);
  const double2 q = reinterpret_cast<const double2*>(A.S.qpos)[i];
  const double2 g = reinterpret_cast<const double2*>(A.S.goal)[i];
  int32_t el = A.S.elapsed[i];
  const uint32_t ep = A.S.episode[i];
  double x = q.x, y = q.y, gx = g.x, gy = g.y;
  const int64_t row0 = A.out.row_offset + i * A.out.row_stride;
  const double noise = A.cfg.noise;

  for (int32_t k = 0; k < A.k_steps; ++k) {
    const int32_t t = A.t0 + k;
    const int64_t row = row0 + t;
    const int64_t tn = (int64_t)t * n + i;  // this step's tape entry
    const int64_t kn = (int64_t)k * n + i;  // this step's diagnostics entry
    // 1. rows: the point agent's prev_qpos is its observation
    const float2 qf = make_float2((float)x, (float)y);
    reinterpret_cast<float2*>(A.out.observations)[row] = qf;
    reinterpret_cast<float2*>(A.out.qpos)[row] = qf;
    if (A.out.qpos64 != nullptr) reinterpret_cast<double2*>(A.out.qpos64)[kn] = make_double2(x, y);
    if (A.out.goal64 != nullptr) reinterpret_cast<double2*>(A.out.goal64)[kn] = make_double2(gx, gy);
    // 2. direction
    double vx, vy;
    if constexpr (kMode == OGBX_COLLECT_EXPLORE) {
      const int32_t period = t / A.cfg.explore_period;
      if (A.tape.dir != nullptr) {
        const double2 d = reinterpret_cast<const double2*>(A.tape.dir)[(int64_t)period * n + i];
        vx = d.x;
        vy = d.y;
      } else {
        collect_box_muller(philox4x32_10({g_lo, (uint32_t)period, kCollectDir, g_hi}, A.k0, A.k1), &vx, &vy);
      }
    } else {
      double sx, sy;
      subgoal_of(P, wall_s, A.bfs, x, y, gx, gy, &sx, &sy);
      vx = sx - x;
      vy = sy - y;
    }
    const double den = sqrt(fma(vy, vy, vx * vx)) + 1e-6;
    const double ux = vx / den, uy = vy / den;
    // 3. action
    double nx, ny;
    if (A.tape.normal != nullptr) {
      const double2 z = reinterpret_cast<const double2*>(A.tape.normal)[tn];
      nx = z.x;
      ny = z.y;
    } else {
      double c, s;
      collect_box_muller(philox4x32_10({g_lo, (uint32_t)t, kCollectNormal, g_hi}, A.k0, A.k1), &c, &s);
      nx = 0.0 + noise * c;
      ny = 0.0 + noise * s;
    }
    double ax = ux + nx, ay = uy + ny;
    ax = ax < -1.0 ? -1.0 : (ax > 1.0 ? 1.0 : ax);
    ay = ay < -1.0 ? -1.0 : (ay > 1.0 ? 1.0 : ay);
    reinterpret_cast<float2*>(A.out.actions)[row] = make_float2((float)ax, (float)ay);
    // 4. step (maze_step_kernel's float64 action path, no auto-reset)
    const double dx = 0.2 * ax, dy = 0.2 * ay;
    bool succ = false;
    if (C.success_pre) succ = goal_within(x, y, gx, gy, C.goal_s2max);
    x = x + dx;
    y = y + dy;
    point_step_as(pm, nb_s, C.H, C.W, &x, &y);
    if (!C.success_pre) succ = goal_within(x, y, gx, gy, C.goal_s2max);
    if (C.n_tp_in > 0) {
      for (int tp = 0; tp < C.n_tp_in; ++tp) {
        if (goal_reached(x, y, P.tp_in[tp][0], P.tp_in[tp][1], P.tp_radius * 1.5)) {
          u32x4 c = philox4x32_10({g_lo, ep, 0x100u + (uint32_t)el, g_hi}, A.sk0 ^ kTagMazeTeleport, A.sk1);
          int o_idx = (int)bounded_u32(c.x, (uint32_t)P.n_tp_out);
          x = P.tp_out[o_idx][0];
          y = P.tp_out[o_idx][1];
          break;
        }
      }
    }
    el += 1;
    A.out.terminals[row] = (uint8_t)(el >= C.max_steps);
    if (A.out.success != nullptr) A.out.success[kn] = (uint8_t)succ;
    // 5. navigate: a reached goal is replaced (set_goal_kernel's arithmetic)
    if constexpr (kMode == OGBX_COLLECT_NAVIGATE) {
      if (succ) {
        int32_t pick;
        if (A.tape.goal_pick != nullptr) {
          pick = A.tape.goal_pick[tn];
          pick = pick < 0 ? 0 : (pick > A.cfg.n_goal_cells - 1 ? A.cfg.n_goal_cells - 1 : pick);
        } else {
          const u32x4 w = philox4x32_10({g_lo, (uint32_t)t, kCollectPick, g_hi}, A.k0, A.k1);
          pick = (int32_t)bounded_u32(w.x, (uint32_t)A.cfg.n_goal_cells);
        }
        const int32_t ci = A.cfg.goal_cells[2 * pick], cj = A.cfg.goal_cells[2 * pick + 1];
        gx = cj * P.pm.unit - P.pm.off_x;
        gy = ci * P.pm.unit - P.pm.off_y;
        if (C.add_noise_to_goal) {
          double r0, r1;
          if (A.tape.goal_noise != nullptr) {
            const double2 r = reinterpret_cast<const double2*>(A.tape.goal_noise)[tn];
            r0 = r.x;
            r1 = r.y;
          } else {
            const u32x4 w = philox4x32_10({g_lo, (uint32_t)t, kCollectGNoise, g_hi}, A.k0, A.k1);
            r0 = -1.0 + 2.0 * u01_from(w.x, w.y);
            r1 = -1.0 + 2.0 * u01_from(w.z, w.w);
          }
          gx = gx + r0 * P.pm.unit / 4.0;
          gy = gy + r1 * P.pm.unit / 4.0;
        }
      }
    }
  }
  // 6. the env state continues from here
  reinterpret_cast<double2*>(A.S.qpos)[i] = make_double2(x, y);
  A.S.elapsed[i] = el;
  if constexpr (kMode == OGBX_COLLECT_NAVIGATE) reinterpret_cast<double2*>(A.S.goal)[i] = make_double2(gx, gy);
}

}  // namespace ogbx
