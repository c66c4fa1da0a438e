// pds_evaluate_hist_args.h -- launch interface of the fused evaluation of observation-history policies
// (csrc/pds_evaluate_hist.h; entry point pds_evaluate_policies_history in csrc/pds_api.hip).
#pragma once
#include "pds_evaluate_args.h"

namespace pds {

// Arguments of evaluate_hist_kernel: the metrics kernel's -- with shape.d_in = H x half, mean / stdv [P, H half], obs0 [N, H half]
// the histories on entry, and metrics NULL where the caller wants none -- and behind them the history size.  The env
// configurations it is built for are the history rollout's: rollout_hist_supported() (csrc/pds_types.h).
struct EvalHistArgs {
  EvalMetricsArgs m;  // FIRST member (the kernel reads the head of its argument block as an EvalArgs, and that as a StepArgs)
  int H;              // observation_history_size: a history row holds H halves of the handle's own row
};
static_assert(offsetof(EvalHistArgs, m) == 0, "the history kernel reads the head of its argument block as an EvalMetricsArgs");

// (the translation units mirror csrc/pds_rollout_hist_*.hip: the same variants, hn = rollout_hist_tiles(H x half))
bool launch_evaluate_hist_hover(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_circle(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_takeoff(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_hover_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_circle_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);

}  // namespace pds
