// pds_rollout_deep_args.h -- launch interface of the one-launch rollout for actors with THREE or FOUR hidden layers
// (csrc/pds_rollout_deep.h; entry point pds_rollout_deep in csrc/pds_api.hip, include/pds_rollout_deep.h).
#pragma once
#include "../../include/pds_rollout_deep.h"
#include "pds_types.h"

namespace pds {

// Arguments of rollout_deep_kernel: RolloutHistArgs (csrc/pds_types.h) without the history and with the deep actor.  s.reward /
// term / trunc / cost point at the [T, N] rollout buffers, s.obs at obs_buf + N D (step t writes o(t + 1) into row t + 1, as in
// RolloutArgs).
struct RolloutDeepArgs {
  StepArgs s;  // FIRST member (reload_args reads the kernarg segment as a StepArgs)
  pds_mlp_deep pi;
  const float *mean, *stdv;  // optional standardisation of the network input (both or none)
  float eps;
  const float *log_std;      // [d_out]
  unsigned long long seed;   // Philox key of the action noise (pds_gaussian_sample)
  const unsigned long long *call_base;  // device word added to call_offset (hipGraph replays), or nullptr
  unsigned long long call_offset;       // step t samples with call = *call_base + call_offset + t + 1
  int deterministic, T, slots;
  const float *obs0;         // [N, D] o(0) (= obs_buf row 0)
  float *act_buf, *logp_buf;
  float *fin_rows;           // [slots, N, D]
  int *fin_step;             // [slots, N]: step whose fval entry the row's value is, -1 = unused (set by the caller)
  float *ep_ret, *ep_len, *stats;
};
static_assert(offsetof(RolloutDeepArgs, s) == 0, "reload_args() reads the head of the kernarg segment as a StepArgs");

// The env configurations rollout_deep_kernel is built for: fused_pwm_family<TASK> (csrc/pds_rollout.h) -- control_mode PWM, no
// latency ring, no Kalman hold, all eight noise settings; motor dynamics on Hover and Circle, the ground effect on TakeOff: the
// set evaluate_deep_kernel is built for.  pds_rollout_deep_supported and pds_rollout_deep ask BEFORE they touch the handle.
inline bool rollout_deep_family(int task, const LaunchFlags &f) {
  return f.ctrl == 0 && !f.lat && !f.hold && rollout_supported(task, f);
}
// The variants of the family whose code object may be launched.  A variant whose env wave spilled VGPRs where rollout_hist_kernel /
// evaluate_deep_kernel of the same variant does not would be listed here and answer "not built"
// (profiles/rollout_deep_kernel_resources.txt: none does).
inline bool rollout_deep_variant_built(int /*task*/, const LaunchFlags & /*f*/, int /*n_hidden*/) { return true; }

// one translation unit per (task, depth): csrc/pds_rollout_deep_<task>_l{3,4}.hip
bool launch_rollout_deep_hover_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra);
bool launch_rollout_deep_hover_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra);
bool launch_rollout_deep_circle_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra);
bool launch_rollout_deep_circle_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra);
bool launch_rollout_deep_takeoff_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra);
bool launch_rollout_deep_takeoff_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra);

}  // namespace pds
