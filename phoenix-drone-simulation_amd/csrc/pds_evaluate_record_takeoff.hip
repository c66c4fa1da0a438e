// pds_evaluate_record_takeoff.hip -- evaluate_kernel (pds_evaluate.h), record form, TakeOff: all its families.
#include "pds_evaluate.h"

namespace pds {
PDS_EVALUATE_TASK_UNIT_FORM(launch_evaluate_takeoff, PDS_TASK_TAKEOFF, true, false, true, nullptr, nullptr)
}  // namespace pds
