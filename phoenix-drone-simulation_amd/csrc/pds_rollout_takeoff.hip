// pds_rollout_takeoff.hip -- the fused rollout (pds_rollout.h) for TakeOff (control_mode PWM only, envs/takeoff.py:225):
// every noise setting, the latency ring, the Kalman hold.
#include "pds_rollout.h"

namespace pds {
bool launch_rollout_takeoff(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutArgs &ra) {
  return fused_task<PDS_TASK_TAKEOFF>(f, RolloutLaunch{grid, s, ra}, nullptr, nullptr);
}
}  // namespace pds
