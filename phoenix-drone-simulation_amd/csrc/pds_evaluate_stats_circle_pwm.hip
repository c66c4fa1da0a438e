// pds_evaluate_stats_circle_pwm.hip -- the stats form (METRICS and STATS) of the kernels of pds_evaluate_circle_pwm.hip: control_mode PWM without
// latency ring / Kalman hold, all eight settings of domain randomisation x thrust noise x observation noise, with and without
// motor dynamics.
#include "pds_evaluate.h"

namespace pds {
bool launch_evaluate_stats_circle_pwm(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalStatsArgs &ea) { return eval_pwm_family<PDS_TASK_CIRCLE>(f, EvalStatsLaunch{grid, s, ea}); }
}  // namespace pds
