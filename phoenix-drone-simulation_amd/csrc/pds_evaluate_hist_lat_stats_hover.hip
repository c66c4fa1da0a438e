// pds_evaluate_hist_lat_stats_hover.hip -- instantiates the stats form of the one-launch evaluation of observation-history
// policies (csrc/pds_evaluate_hist.h, STATS) on the latency ring with control_mode PWM for one task: {lean, reference-default noise} x
// {with, without motor dynamics} x 4 input widths.
#include "pds_evaluate_hist.h"

namespace pds {
bool launch_evaluate_hist_stats_hover_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka) {
  return hist_lat_task<PDS_TASK_HOVER, 0>(f, hn, EvalHistStatsLaunch{grid, s, ka});
}
}  // namespace pds
