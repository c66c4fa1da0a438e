// pds_evaluate_stats_circle_lat.hip -- the stats form (METRICS and STATS) of the kernels of pds_evaluate_circle_lat.hip: the latency ring with
// control_mode PWM and with the PID modes, {lean, reference default} x {with, without motor dynamics}.
#include "pds_evaluate.h"

namespace pds {
bool launch_evaluate_stats_circle_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalStatsArgs &ea) { return eval_lat_family<PDS_TASK_CIRCLE>(f, EvalStatsLaunch{grid, s, ea}); }
}  // namespace pds
