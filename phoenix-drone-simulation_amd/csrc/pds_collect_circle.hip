// pds_collect_circle.hip -- the fused off-policy collection kernels (pds_collect.h) of one task: control_mode PWM, noise off or the
// reference's default, with and without motor dynamics.
#include "pds_collect.h"

namespace pds {
bool launch_collect_circle(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) { return launch_collect_task<PDS_TASK_CIRCLE>(f, grid, s, ca); }
}  // namespace pds
