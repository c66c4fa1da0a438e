// pds_evaluate_deep_args.h -- launch interface of the fused evaluation of policies with THREE or FOUR hidden layers
// (csrc/pds_evaluate_deep.h; entry point pds_evaluate_policies_deep in csrc/pds_api.hip, include/pds_evaluate_deep.h).
#pragma once
#include "../../include/pds_evaluate_deep.h"
#include "pds_evaluate_args.h"

namespace pds {

// Arguments of evaluate_deep_kernel: the metrics kernel's -- params [P, deep_param_count], mean / stdv [P, D], obs0 [N, D], metrics
// NULL where the caller wants none; m.e.shape and m.e.param_count are not read (zero) -- and behind them the network's shape.
struct EvalDeepArgs {
  EvalMetricsArgs m;     // FIRST member (the kernel reads the head of its argument block as an EvalArgs, and that as a StepArgs)
  pds_mlp_deep deep;     // d_in, n_hidden, hidden[], d_out, activation of every policy; its pointers are not read
  int deep_param_count;  // floats of a row of params: W1 b1 .. W(L+1) b(L+1) (pds_mlp_deep_param_count layout)
};
static_assert(offsetof(EvalDeepArgs, m) == 0, "the deep kernel reads the head of its argument block as an EvalMetricsArgs");
// the block is the kernels' argument segment: size and the place of the last member, as the compiler laid it out
static_assert(sizeof(EvalDeepArgs) == 848 && offsetof(EvalDeepArgs, deep_param_count) == 840, "the kernarg layout of the deep evaluation");

// The env configurations evaluate_deep_kernel is built for: fused_pwm_family<TASK> (csrc/pds_rollout.h) -- control_mode PWM, no
// latency ring, no Kalman hold, all eight noise settings; motor dynamics on Hover and Circle, the ground effect on TakeOff.
// pds_evaluate_deep_supported and pds_evaluate_policies_deep ask BEFORE they touch the handle.
inline bool evaluate_deep_family(int task, const LaunchFlags &f) {
  return f.ctrl == 0 && !f.lat && !f.hold && rollout_supported(task, f);
}
// The variants of the family whose code object may be launched.  A variant whose env wave spilled VGPRs where the one-team
// evaluate_kernel of the same variant does not would be listed here and answer "not built"
// (profiles/evaluate_deep_kernel_resources.txt: none does).
inline bool evaluate_deep_variant_built(int /*task*/, const LaunchFlags & /*f*/, int /*n_hidden*/) { return true; }

// one translation unit per (task, depth): csrc/pds_evaluate_deep_<task>_l{3,4}.hip
bool launch_evaluate_deep_hover_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka);
bool launch_evaluate_deep_hover_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka);
bool launch_evaluate_deep_circle_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka);
bool launch_evaluate_deep_circle_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka);
bool launch_evaluate_deep_takeoff_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka);
bool launch_evaluate_deep_takeoff_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka);

}  // namespace pds
