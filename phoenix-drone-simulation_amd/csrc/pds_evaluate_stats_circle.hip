// pds_evaluate_stats_circle.hip -- evaluate_kernel (pds_evaluate.h), stats form: the task's dispatcher, the PID control modes, the Kalman hold.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_TASK_UNIT(launch_evaluate_circle, PDS_TASK_CIRCLE, true, true, launch_evaluate_circle_lat<M, S>, launch_evaluate_circle_pwm<M, S>)
}  // namespace pds
