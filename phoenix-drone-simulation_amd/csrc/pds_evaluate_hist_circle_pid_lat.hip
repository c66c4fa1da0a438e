// pds_evaluate_hist_circle_pid_lat.hip -- instantiates the one-launch evaluation of observation-history policies
// (csrc/pds_evaluate_hist.h) on the latency ring under the PID control modes for one task: {AttitudeRate, Attitude} x {lean,
// reference-default noise} x {with, without motor dynamics} x 4 input widths.
#include "pds_evaluate_hist.h"

namespace pds {
bool launch_evaluate_hist_circle_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka) {
  return hist_lat_pid<PDS_TASK_CIRCLE>(f, hn, EvalHistLaunch{grid, s, ka});
}
}  // namespace pds
