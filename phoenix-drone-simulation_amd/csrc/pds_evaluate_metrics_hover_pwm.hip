// pds_evaluate_metrics_hover_pwm.hip -- evaluate_kernel (pds_evaluate.h), metrics form: control_mode PWM, every noise setting x motor dynamics.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_FAMILY_UNIT(launch_evaluate_hover_pwm, fused_pwm_family, PDS_TASK_HOVER, EvalForm::Metrics)
}  // namespace pds
