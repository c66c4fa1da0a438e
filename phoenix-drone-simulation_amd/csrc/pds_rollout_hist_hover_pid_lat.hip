// pds_rollout_hist_hover_pid_lat.hip -- instantiates the one-launch rollout for observation histories other than 2
// (csrc/pds_rollout_hist.h) on the latency ring under the PID control modes for one task: {AttitudeRate, Attitude} x {lean,
// reference-default noise} x {with, without motor dynamics} x 4 input widths.
#include "pds_rollout_hist.h"

namespace pds {
bool launch_rollout_hist_hover_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const RolloutHistArgs &ra) {
  return hist_lat_pid<PDS_TASK_HOVER>(f, hn, RolloutHistLaunch{grid, s, ra});
}
}  // namespace pds
