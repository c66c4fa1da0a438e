// pds_evaluate_stats_takeoff.hip -- the fused policy evaluation with flight metrics and observation sums (pds_evaluate.h, STATS) for TakeOff: the
// variants of pds_evaluate_takeoff.hip -- every noise setting, the latency ring, the Kalman hold.
#include "pds_evaluate.h"

namespace pds {
bool launch_evaluate_stats_takeoff(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalStatsArgs &ea) {
  if (!rollout_supported(PDS_TASK_TAKEOFF, f)) return false;
  const EvalStatsLaunch l{grid, s, ea};
  if (f.hold) return eval_pid_hold_family<PDS_TASK_TAKEOFF>(f, l);
  if (f.lat) return eval_lat_family<PDS_TASK_TAKEOFF>(f, l);
  return eval_pwm_family<PDS_TASK_TAKEOFF>(f, l);
}
}  // namespace pds
