// pds_collect_takeoff.hip -- the fused off-policy collection kernels (pds_collect.h) of one task: control_mode PWM, noise off or the
// reference's default, without motor dynamics.
#include "pds_collect.h"

namespace pds {
bool launch_collect_takeoff(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) { return launch_collect_task<PDS_TASK_TAKEOFF>(f, grid, s, ca); }
}  // namespace pds
