// Driver of tests/test_powder_schedule_cpu.py: runs pwf_plan_step over the
// cases on stdin and prints every plan and the schedule state after it.
//
// A case is one line: phase max_steps auto_reset light_enabled n_fits_i32
// n_steps k_1 ... k_n.  Output: "case" on a line of its own, then per step
//   light order_mode sparse pass_skip use_order run_order_kernel by_task | phase order_ready order_by_task
#include <cstdio>
#include <vector>

#include "powder_schedule.h"

int main() {
  long long phase;
  int max_steps, auto_reset, light_enabled, n_fits, n_steps;
  while (std::scanf("%lld %d %d %d %d %d", &phase, &max_steps, &auto_reset, &light_enabled, &n_fits, &n_steps) == 6) {
    if (n_steps < 0 || n_steps > 4096) return 2;
    std::vector<int> ks((size_t)n_steps);
    for (int& k : ks)
      if (std::scanf("%d", &k) != 1) return 2;
    PwfSchedule s;
    pwf_schedule_reset(s, true);
    s.phase = phase;
    std::puts("case");
    for (int k : ks) {
      const PwfStepPlan p = pwf_plan_step(s, max_steps, auto_reset, k, light_enabled != 0, n_fits != 0);
      std::printf("%d %d %d %d %d %d %d | %lld %d %d\n", (int)p.light, (int)p.order_mode, (int)p.sparse,
                  (int)p.pass_skip, (int)p.use_order, (int)p.run_order_kernel, (int)p.by_task, (long long)s.phase,
                  (int)s.order_ready, (int)s.order_by_task);
    }
  }
  return 0;
}
