// pds_evaluate_record_deep_hover_l3.hip -- evaluate_deep_kernel (pds_evaluate_deep.h), the record form, 3 hidden layers: control_mode PWM, every noise setting x motor dynamics.
#include "pds_evaluate_deep.h"

namespace pds {
PDS_EVALUATE_DEEP_FORM_UNIT(launch_evaluate_record_deep_hover_l3, PDS_TASK_HOVER, 3, EvalForm::Record)
}  // namespace pds
