// pds_evaluate_stats_hover.hip -- the fused policy evaluation with flight metrics and observation sums (pds_evaluate.h, STATS) for one task:
// dispatcher + the PID control modes and the Kalman hold; control_mode PWM with every noise setting:
// pds_evaluate_stats_hover_pwm.hip, the latency ring: pds_evaluate_stats_hover_lat.hip.  The variants of pds_evaluate_hover.hip.
#include "pds_evaluate.h"

namespace pds {
bool launch_evaluate_stats_hover(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalStatsArgs &ea) {
  if (!rollout_supported(PDS_TASK_HOVER, f)) return false;
  if (f.hold) return eval_pid_hold_family<PDS_TASK_HOVER>(f, EvalStatsLaunch{grid, s, ea});
  if (f.lat) return launch_evaluate_stats_hover_lat(f, grid, s, ea);
  if (f.ctrl == 0) return launch_evaluate_stats_hover_pwm(f, grid, s, ea);
  return eval_pid_hold_family<PDS_TASK_HOVER>(f, EvalStatsLaunch{grid, s, ea});
}
}  // namespace pds
