// pds_evaluate_hover_lat.hip -- evaluate_kernel (pds_evaluate.h), plain form: the latency ring, PWM and PID modes.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_FAMILY_UNIT(launch_evaluate_hover_lat, fused_lat_family, PDS_TASK_HOVER, EvalForm::Plain)
}  // namespace pds
