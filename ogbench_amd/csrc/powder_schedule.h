// powder_schedule.h -- which kernels one ogbx_powder_step call of a medium /
// hard env launches, as a pure function of the host's schedule state.  Plain
// C++17 (no HIP, no project headers) so that a CPU test can enumerate it
// (tests/test_powder_schedule_cpu.py).
//
// Results never depend on the plan: pwf_step_kernel without the skip list
// steps render-only envs itself, bit-identically (only slower), and any order
// is a permutation of the envs.  Only speed depends on it.
#pragma once
#include <cstdint>

// phase of a batch whose envs need not step together (a masked reset, a
// restored state)
constexpr int64_t kPwfPhaseUnknown = -1;

struct PwfSchedule {
  // steps since the last reset of every env (kPwfPhaseUnknown: unknown).  Envs
  // reset together step in phase, so the host can tell the steps on which every
  // in-phase env needs the full kernel (its forward step, or the synchronized
  // truncation + auto-reset) and not launch pwf_light_step_kernel, whose every
  // workgroup would exit.  A wrong guess is harmless (above), so out-of-phase
  // envs (an earlier success + auto-reset, a restored state) stay correct.
  int64_t phase = kPwfPhaseUnknown;
  // the last light launch sorted `order` for the step after it (by task
  // length if order_by_task, which means nothing otherwise); consumed by that
  // step when it is the in-phase full step the host expected.  A stale order
  // is still a permutation of the envs: only the schedule would differ.
  bool order_ready = false;
  bool order_by_task = false;
};

// The launches of one step, in their fixed order: light, order kernel, full.
struct PwfStepPlan {
  bool light;             // launch pwf_light_step_kernel (render-only envs)
  int32_t order_mode;     // its extra sorting workgroup: 0 none, 1 by last cost, 2 by task length
  bool sparse;            // full kernel: a chunk of envs per workgroup, else one env per workgroup (dense)
  bool pass_skip;         // dense launch: skip the envs the light kernel handled
  bool use_order;         // dense launch: workgroups in `order`, costliest first
  bool run_order_kernel;  // sort `order` in a launch of its own before the dense launch ...
  bool by_task;           // ... by task length (else by last measured cost)
};

// A reset of every env (all_envs) puts them in phase; a masked one does not.
inline void pwf_schedule_reset(PwfSchedule& s, bool all_envs) {
  s.phase = all_envs ? 0 : kPwfPhaseUnknown;
  s.order_ready = false;
}

// The plan of a step of k_steps env steps, and s advanced past it.
// light_enabled: the OGBX_PWF_LIGHT knob; n_fits_i32: `order` holds int32 envs.
inline PwfStepPlan pwf_plan_step(PwfSchedule& s, int32_t max_steps, int32_t auto_reset, int32_t k_steps,
                                 bool light_enabled, bool n_fits_i32) {
  const bool in_phase = s.phase >= 0;
  // episodes of T steps repeat when auto-reset truncates them; j: the in-phase
  // envs' elapsed steps before this step, jn: before the next
  const int64_t T = max_steps > 0 ? max_steps : 0;
  const bool wraps = auto_reset && T > 0;
  const int64_t j = wraps ? s.phase % T : s.phase;
  const int64_t jn = wraps ? (s.phase + 1) % T : s.phase + 1;
  // a full step: the forward of the third sub-action, or the synchronized
  // truncation + auto-reset (goal replay)
  const bool sync_reset = wraps && j + 1 >= T, sync_next = wraps && jn + 1 >= T;
  // every in-phase env runs the full kernel this step
  const bool all_full = in_phase && k_steps == 1 && (j % 3 == 2 || sync_reset);

  PwfStepPlan p{};
  p.light = light_enabled && k_steps == 1 && !all_full;
  // the order of the next step's full launch, if the next step is an in-phase
  // full step: sorted by a workgroup of this light launch
  if (p.light && in_phase && n_fits_i32 && (jn % 3 == 2 || sync_next)) p.order_mode = sync_next ? 2 : 1;
  // in phase, a render-only step leaves (nearly) no env to the full kernel
  p.sparse = p.light && in_phase;
  p.pass_skip = p.light && !p.sparse;
  // in-phase full step: workgroups longest first (the synchronized goal
  // replays by task length, forward steps by last measured cost), sorted here
  // unless the step before pre-sorted them by the same key
  p.use_order = all_full && n_fits_i32;
  p.by_task = p.use_order && sync_reset;
  p.run_order_kernel = p.use_order && !(s.order_ready && s.order_by_task == p.by_task);

  s.order_ready = p.order_mode != 0;
  if (p.light) s.order_by_task = p.order_mode == 2;
  if (in_phase) s.phase += k_steps;
  return p;
}
