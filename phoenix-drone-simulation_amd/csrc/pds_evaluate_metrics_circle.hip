// pds_evaluate_metrics_circle.hip -- evaluate_kernel (pds_evaluate.h), metrics form: the task's dispatcher, the PID control modes, the Kalman hold.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_TASK_UNIT(launch_evaluate_circle, PDS_TASK_CIRCLE, EvalForm::Metrics, launch_evaluate_circle_lat<F>, launch_evaluate_circle_pwm<F>)
}  // namespace pds
