// pds_rollout_deep_circle_l4.hip -- rollout_deep_kernel (pds_rollout_deep.h), 4 hidden layers: control_mode PWM, every noise setting x motor dynamics.
#include "pds_rollout_deep.h"

namespace pds {
PDS_ROLLOUT_DEEP_UNIT(launch_rollout_deep_circle_l4, PDS_TASK_CIRCLE, 4)
}  // namespace pds
