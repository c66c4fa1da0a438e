// pds_evaluate_record_circle_pwm.hip -- evaluate_kernel (pds_evaluate.h), record form: control_mode PWM, every noise setting x motor dynamics.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_FAMILY_UNIT(launch_evaluate_circle_pwm, fused_pwm_family, PDS_TASK_CIRCLE, EvalForm::Record)
}  // namespace pds
