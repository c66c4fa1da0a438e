// pds_evaluate_hist_lat_record_circle.hip -- instantiates the record form of the one-launch evaluation of observation-history
// policies (csrc/pds_evaluate_hist.h, REC) on the latency ring with control_mode PWM for one task: {lean, reference-default noise} x
// {with, without motor dynamics} x 4 input widths.
#include "pds_evaluate_hist.h"

namespace pds {
bool launch_evaluate_hist_record_circle_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka) {
  return hist_lat_task<PDS_TASK_CIRCLE, 0>(f, hn, EvalHistRecordLaunch{grid, s, ka});
}
}  // namespace pds
