// pds_evaluate_deep_circle_l3.hip -- evaluate_deep_kernel (pds_evaluate_deep.h), 3 hidden layers: control_mode PWM, every noise setting x motor dynamics.
#include "pds_evaluate_deep.h"

namespace pds {
PDS_EVALUATE_DEEP_UNIT(launch_evaluate_deep_circle_l3, PDS_TASK_CIRCLE, 3)
}  // namespace pds
