// pds_evaluate_hover_lat.hip -- the fused evaluation kernels of the latency ring (envs/agents.py:267-276) with control_mode PWM and
// with the PID modes: {lean, reference default} x {with, without motor dynamics}.
#include "pds_evaluate.h"

namespace pds {
bool launch_evaluate_hover_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalArgs &ea) { return eval_lat_family<PDS_TASK_HOVER>(f, EvalLaunch{grid, s, ea}); }
}  // namespace pds
