// pds_evaluate_record_takeoff.hip -- evaluate_kernel (pds_evaluate.h), record form, TakeOff: all its families.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_TASK_UNIT(launch_evaluate_takeoff, PDS_TASK_TAKEOFF, EvalForm::Record, nullptr, nullptr)
}  // namespace pds
