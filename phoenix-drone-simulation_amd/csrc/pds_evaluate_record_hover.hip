// pds_evaluate_record_hover.hip -- evaluate_kernel (pds_evaluate.h), record form: the task's dispatcher, the PID control modes, the Kalman hold.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_TASK_UNIT_FORM(launch_evaluate_hover, PDS_TASK_HOVER, true, false, true, launch_evaluate_hover_lat<M, S, R>, launch_evaluate_hover_pwm<M, S, R>)
}  // namespace pds
