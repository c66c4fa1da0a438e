// pds_evaluate_record_hover.hip -- evaluate_kernel (pds_evaluate.h), record form: the task's dispatcher, the PID control modes, the Kalman hold.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_TASK_UNIT(launch_evaluate_hover, PDS_TASK_HOVER, EvalForm::Record, launch_evaluate_hover_lat<F>, launch_evaluate_hover_pwm<F>)
}  // namespace pds
