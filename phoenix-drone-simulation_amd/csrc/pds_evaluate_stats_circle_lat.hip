// pds_evaluate_stats_circle_lat.hip -- evaluate_kernel (pds_evaluate.h), stats form: the latency ring, PWM and PID modes.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_FAMILY_UNIT(launch_evaluate_circle_lat, fused_lat_family, PDS_TASK_CIRCLE, EvalForm::Stats)
}  // namespace pds
