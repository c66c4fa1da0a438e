// pds_collect_args.h -- launch interface of the fused off-policy collection (csrc/pds_collect.h; entry points pds_collect and
// pds_collect_supported in csrc/pds_api.hip).
#pragma once
#include "pds_types.h"

namespace pds {

constexpr int kCollectDdpg = 0, kCollectSac = 1;  // `mode` of pds_collect: which exploration rule, actor d_out 4 / 8
constexpr int kCollectStats = 8;                  // floats per tile in d_tile_stats

// Arguments of collect_kernel.
struct CollectArgs {
  StepArgs s;  // FIRST member (reload_args reads the kernarg segment as a StepArgs).  obs and final_obs are NULL (the rows stay in
               // LDS); reward / cost / term / trunc point at the handle's [N] sink row, as in EvalArgs: the ring block moves from
               // step to step and wraps, so the kernel stores `rew` and `done` itself
  pds_mlp pi;                // the actor: d_out 4 (DDPG: pre-tanh output) or 8 (SAC: [mu | log_std])
  int mode, K;
  float act_limit;
  const float *log_std;      // DDPG: [4] log of the exploration noise scale; SAC: unused
  unsigned long long seed, first_call;  // step s draws the noise of (seed, sample id = env row, call = first_call + s)
  float *oa, *obs2, *rew, *done;        // the ring: [capacity, D + 4], [capacity, D], [capacity], [capacity]
  long long capacity, ptr;   // multiples of N; step s fills rows (ptr + s N) mod capacity ...
  float *obs;                // [N, D] in: o(0), out: o(K)
  float *ep_ret, *ep_len;    // [N] running return / length, in / out
  float *tile_stats;         // [tiles, 8] count; sum, sum of squares, min, max of the return; sum, min, max of the length
};
static_assert(offsetof(CollectArgs, s) == 0, "reload_args() reads the head of the kernarg segment as a StepArgs");

// The env configurations collect_kernel is built for: control_mode PWM, no latency ring, no Kalman hold, no ground effect; noise
// all off or the reference's default (DR + thrust noise + observation noise); with and without motor dynamics (TakeOff: without).
inline bool collect_env_supported(int task, const LaunchFlags &f) {
  if (f.ge || f.hold || f.lat || f.ctrl != 0) return false;
  const bool lean = !f.dr && !f.tn && !f.on, full = f.dr && f.tn && f.on;
  return (lean || full) && !(task == PDS_TASK_TAKEOFF && f.motor);
}

// What pds_collect_control (include/pds_collect_control.h) flies beside those: Hover and Circle under a PID control mode
// (AttitudeRate, Attitude) and / or with the latency ring -- the five (control mode, latency) pairs other than (PWM, none) -- noise
// all off or the reference's default, with and without motor dynamics.  Not built: Kalman hold, ground effect, partial noise
// settings, TakeOff (envs/takeoff.py:225 fixes control_mode PWM; its latency form is not built either).
inline bool collect_control_env_supported(int task, const LaunchFlags &f) {
  if (f.ge || f.hold || task == PDS_TASK_TAKEOFF || (f.ctrl == 0 && !f.lat)) return false;
  const bool lean = !f.dr && !f.tn && !f.on, full = f.dr && f.tn && f.on;
  return lean || full;
}

// one translation unit per task: csrc/pds_collect_<task>.hip; the PID modes and the latency ring in three more per task:
// csrc/pds_collect_<task>_pid.hip (a PID mode, no ring), _lat.hip (PWM on the ring), _pid_lat.hip (a PID mode on the ring)
bool launch_collect_hover(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_circle(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_takeoff(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_hover_pid(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_hover_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_hover_pid_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_circle_pid(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_circle_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);
bool launch_collect_circle_pid_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca);

}  // namespace pds
