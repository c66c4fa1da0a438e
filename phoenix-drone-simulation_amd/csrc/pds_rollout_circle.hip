// pds_rollout_circle.hip -- the fused rollout (pds_rollout.h) for one task: dispatcher + the PID control modes and the
// Kalman hold; control_mode PWM with every noise setting: pds_rollout_circle_pwm.hip, the latency ring: pds_rollout_circle_lat.hip.
#include "pds_rollout.h"

namespace pds {
bool launch_rollout_circle(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutArgs &ra) {
  return fused_task<PDS_TASK_CIRCLE>(f, RolloutLaunch{grid, s, ra}, launch_rollout_circle_lat, launch_rollout_circle_pwm);
}
}  // namespace pds
