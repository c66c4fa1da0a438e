// pds_evaluate_args.h -- launch interface of the fused policy evaluation (csrc/pds_evaluate.h; entry point pds_evaluate_policies
// in csrc/pds_api.hip).
#pragma once
#include <type_traits>

#include "pds_types.h"

namespace pds {

// Arguments of evaluate_kernel.  The env configurations it is built for are the fused rollout's: rollout_supported()
// (csrc/pds_types.h) is the one statement of that rule, for pds_rollout and for pds_evaluate_policies.
struct EvalArgs {
  StepArgs s;  // FIRST member (reload_args reads the kernarg segment as a StepArgs).  obs and final_obs are NULL (the rows stay in
               // LDS); reward / cost / term / trunc point at the handle's [N] sink row: step_once (csrc/pds_step.h) streams every
               // step's outcome out, and the evaluation keeps that code path as it is -- each step overwrites the same row
  pds_mlp shape;             // d_in, h1, h2, d_out, activation of every policy; its pointers are not read
  const float *params;       // [P, param_count] W1 b1 W2 b2 W3 b3 of policy p in row p (pds_mlp_param_count layout)
  const float *mean, *stdv;  // [P, D] optional standardisation of policy p's inputs (both or none)
  float eps;
  int param_count;
  int tiles_per_policy;      // E / 64: tile t flies policy t / tiles_per_policy
  int T;                     // steps after which every episode still running is cut
  const float *obs0;         // [N, D] the observation every env holds on entry
  float *ret, *len, *cost;   // [N] return, length and cost of every env's first episode
};
static_assert(offsetof(EvalArgs, s) == 0, "reload_args() reads the head of the kernarg segment as a StepArgs");

// The four forms of evaluate_kernel (csrc/pds_evaluate.h has what each does) and of everything that launches it.  Plain:
// pds_evaluate_policies; Metrics: pds_evaluate_policies_metrics; Stats: pds_evaluate_policies_stats; Record:
// pds_evaluate_policies_record.
enum class EvalForm : int { Plain, Metrics, Stats, Record };
// the env wave sums the PDS_EM_* flight metrics
constexpr bool eval_sums_metrics(EvalForm f) { return f != EvalForm::Plain; }
// the env wave keeps the alive mask of the tile for the network waves
constexpr bool eval_keeps_alive_mask(EvalForm f) { return f == EvalForm::Stats || f == EvalForm::Record; }

// Arguments of the Metrics form: the plain kernel's, and behind them the array of the flight metrics.
struct EvalMetricsArgs {
  EvalArgs e;      // FIRST member (the kernel reads the head of its argument block as an EvalArgs, and that as a StepArgs)
  float *metrics;  // [N, PDS_EVAL_METRICS] the PDS_EM_* sums of every env's first episode (include/pds.h), 16-byte aligned
};
static_assert(offsetof(EvalMetricsArgs, e) == 0, "the metrics kernel reads the head of its argument block as an EvalArgs");
static_assert(PDS_EVAL_METRICS == 8, "a metrics row is stored as two float4");
// Arguments of the Stats form: the metrics kernel's, and behind them the slab of the observation sums.
struct EvalStatsArgs {
  EvalMetricsArgs m;  // FIRST member (the kernel reads the head of its argument block as an EvalMetricsArgs)
  float *obs_sums;    // [tiles, 4, 2, 64]: tile, network wave, S1 / S2, feature (include/pds.h), 16-byte aligned
};
static_assert(offsetof(EvalStatsArgs, m) == 0, "the stats kernel reads the head of its argument block as an EvalMetricsArgs");
// Arguments of the Record form: the metrics kernel's (`metrics` may be NULL here: summed, not stored) and behind them the record
// of the flights.  Of the E / 64 tiles of a policy the first rec_tiles record: tile t iff t % tiles_per_policy < rec_tiles
// (wave-uniform), its lane's column of the record
//   j = (t / tiles_per_policy) * 64 * rec_tiles + (t % tiles_per_policy) * 64 + lane,       N_rec = P * 64 * rec_tiles.
struct EvalRecordArgs {
  EvalMetricsArgs m;  // FIRST member (the kernel reads the head of its argument block as an EvalMetricsArgs)
  float4 *flight;     // [T, 4, N_rec, 4] floats, 16-byte aligned: step s, piece q, column j -- piece 0 = (px, py, pz, vx), 1 = (vy, vz,
                      // roll, pitch), 2 = (yaw, wx, wy, wz) of x(s), 3 = a(s) raw; a wave stores a piece as one 1 KiB line
  float *obs_rec;     // [T, N_rec, D] the raw observation o(s) the policy acted on, or NULL
  int rec_tiles;      // 1 <= rec_tiles <= tiles_per_policy
};
static_assert(offsetof(EvalRecordArgs, m) == 0, "the record kernel reads the head of its argument block as an EvalMetricsArgs");
// The four blocks are the kernels' argument segments: size and the place of the last member, as the compiler laid them out.
static_assert(sizeof(EvalArgs) == 720 && offsetof(EvalArgs, cost) == 712, "the kernarg layout of the Plain form");
static_assert(sizeof(EvalMetricsArgs) == 728 && offsetof(EvalMetricsArgs, metrics) == 720, "the kernarg layout of the Metrics form");
static_assert(sizeof(EvalStatsArgs) == 736 && offsetof(EvalStatsArgs, obs_sums) == 728, "the kernarg layout of the Stats form");
static_assert(sizeof(EvalRecordArgs) == 752 && offsetof(EvalRecordArgs, rec_tiles) == 744, "the kernarg layout of the Record form");

// form -> the argument block of evaluate_kernel<V, TEAMS, F>
template <EvalForm F> struct EvalKernelArgsOf;
template <> struct EvalKernelArgsOf<EvalForm::Plain> { using type = EvalArgs; };
template <> struct EvalKernelArgsOf<EvalForm::Metrics> { using type = EvalMetricsArgs; };
template <> struct EvalKernelArgsOf<EvalForm::Stats> { using type = EvalStatsArgs; };
template <> struct EvalKernelArgsOf<EvalForm::Record> { using type = EvalRecordArgs; };
template <EvalForm F> using EvalKernelArgs = typename EvalKernelArgsOf<F>::type;
// ... and the EvalArgs at its head, on the host and on the device, for a const or a mutable block (EvalHistArgs of
// csrc/pds_evaluate_hist_args.h too: its first member is an EvalMetricsArgs `m`, like EvalStatsArgs' and EvalRecordArgs'; the
// first member of that file's EvalHistRecordArgs is an EvalRecordArgs `r`)
struct EvalHistRecordArgs;
template <class KA>
__host__ __device__ inline auto &eval_head(KA &ka) {
  if constexpr (std::is_same_v<std::remove_const_t<KA>, EvalArgs>) return ka;
  else if constexpr (std::is_same_v<std::remove_const_t<KA>, EvalMetricsArgs>) return ka.e;
  else if constexpr (std::is_same_v<std::remove_const_t<KA>, EvalHistRecordArgs>) return ka.r.m.e;
  else return ka.m.e;
}

// The launch functions, one set for the four forms.  Each is defined and explicitly instantiated for one form by the translation
// unit that holds the form's kernels: csrc/pds_evaluate[_metrics|_stats|_record]_<task>.hip ...
template <EvalForm F> bool launch_evaluate_hover(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);
template <EvalForm F> bool launch_evaluate_circle(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);
template <EvalForm F> bool launch_evaluate_takeoff(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);
// ... and their families, csrc/pds_evaluate[_metrics|_stats|_record]_<task>_{pwm,lat}.hip, like the rollout's: control_mode PWM with every
// noise setting / the latency ring
template <EvalForm F> bool launch_evaluate_hover_pwm(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);
template <EvalForm F> bool launch_evaluate_hover_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);
template <EvalForm F> bool launch_evaluate_circle_pwm(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);
template <EvalForm F> bool launch_evaluate_circle_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka);

}  // namespace pds
