// pds_rollout_circle_pwm.hip -- the fused rollout kernels of control_mode PWM without latency ring / Kalman hold: all eight
// settings of domain randomisation x thrust noise x observation noise, with and without motor dynamics.
#include "pds_rollout.h"

namespace pds {
bool launch_rollout_circle_pwm(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutArgs &ra) {
  return fused_pwm_family<PDS_TASK_CIRCLE>(f, RolloutLaunch{grid, s, ra});
}
}  // namespace pds
