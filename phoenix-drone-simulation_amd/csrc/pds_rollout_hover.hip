// pds_rollout_hover.hip -- the fused rollout (pds_rollout.h) for one task: dispatcher + the PID control modes and the
// Kalman hold; control_mode PWM with every noise setting: pds_rollout_hover_pwm.hip, the latency ring: pds_rollout_hover_lat.hip.
#include "pds_rollout.h"

namespace pds {
bool launch_rollout_hover(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutArgs &ra) {
  return fused_task<PDS_TASK_HOVER>(f, RolloutLaunch{grid, s, ra}, launch_rollout_hover_lat, launch_rollout_hover_pwm);
}
}  // namespace pds
