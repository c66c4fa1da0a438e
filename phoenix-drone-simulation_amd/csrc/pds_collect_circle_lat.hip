// pds_collect_circle_lat.hip -- the fused off-policy collection kernels (pds_collect.h) of one task with control_mode PWM on the
// latency ring: noise off or the reference's default, with and without motor dynamics.
#include "pds_collect.h"

namespace pds {
bool launch_collect_circle_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) { return launch_collect_lat<PDS_TASK_CIRCLE>(f, grid, s, ca); }
}  // namespace pds
