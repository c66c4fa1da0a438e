// pds_evaluate_hist_args.h -- launch interface of the fused evaluation of observation-history policies
// (csrc/pds_evaluate_hist.h; entry point pds_evaluate_policies_history in csrc/pds_api.hip).
#pragma once
#include "../../include/pds_history_record.h"
#include "../../include/pds_history_stats.h"
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
// Arguments of the record form of evaluate_hist_kernel: the Record form's -- flight [T, 4, N_rec, 4], obs_rec [T, N_rec, H half] or
// NULL, rec_tiles and the column of a lane as EvalRecordArgs (csrc/pds_evaluate_args.h) states them, `metrics` optional -- and
// behind them the history size.
struct EvalHistRecordArgs {
  EvalRecordArgs r;  // FIRST member (the kernel reads the head of its argument block as an EvalRecordArgs, that as an EvalArgs, ...)
  int H;             // observation_history_size
};
static_assert(offsetof(EvalHistRecordArgs, r) == 0, "the history record kernel reads the head of its argument block as an EvalRecordArgs");
// Arguments of the stats form of evaluate_hist_kernel: the Stats form's -- obs_sums [tiles, 4, 2, W] with W = 16 x rollout_hist_tiles(H half)
// features a row (include/pds_history_stats.h), `metrics` optional -- and behind them the history size.
struct EvalHistStatsArgs {
  EvalStatsArgs st;  // FIRST member (the kernel reads the head of its argument block as an EvalStatsArgs, that as an EvalMetricsArgs, ...)
  int H;             // observation_history_size
};
static_assert(offsetof(EvalHistStatsArgs, st) == 0, "the history stats kernel reads the head of its argument block as an EvalStatsArgs");
// the three blocks are the kernels' argument segments: size and the place of the last member, as the compiler laid them out
static_assert(sizeof(EvalHistArgs) == 736 && offsetof(EvalHistArgs, H) == 728, "the kernarg layout of the history evaluation");
static_assert(sizeof(EvalHistRecordArgs) == 760 && offsetof(EvalHistRecordArgs, H) == 752, "the kernarg layout of the history record");
static_assert(sizeof(EvalHistStatsArgs) == 744 && offsetof(EvalHistStatsArgs, H) == 736, "the kernarg layout of the history stats");
// the EvalArgs at the head of the stats block (eval_head of csrc/pds_evaluate_args.h knows the other two by their first member)
__host__ __device__ inline EvalArgs &eval_head(EvalHistStatsArgs &ka) { return ka.st.m.e; }
__host__ __device__ inline const EvalArgs &eval_head(const EvalHistStatsArgs &ka) { return ka.st.m.e; }

// The three forms of evaluate_hist_kernel (csrc/pds_evaluate_hist.h has what each does) and of everything that launches it.
// Metrics: pds_evaluate_policies_history; Record: pds_evaluate_policies_history_record; Stats: pds_evaluate_policies_history_stats.
enum class EvalHistForm : int { Metrics, Record, Stats };
// form -> the argument block of evaluate_hist_kernel<V, HN, F>
template <EvalHistForm F>
using EvalHistKernelArgs = std::conditional_t<F == EvalHistForm::Record, EvalHistRecordArgs, std::conditional_t<F == EvalHistForm::Stats, EvalHistStatsArgs, EvalHistArgs>>;
// The input widths hn = rollout_hist_tiles(H half) the stats form is built for: a network lane carries 8 hn accumulators through
// its loop, and a width whose code objects spilled a VGPR or took more scratch than their metrics twins would be left out here
// (profiles/evaluate_history_stats_kernel_resources.txt: none does).  pds_evaluate_history_stats_supported answers by it.
constexpr bool eval_hist_stats_width_built(int hn) { return hn == 4 || hn == 6 || hn == 8 || hn == 12; }

// (the translation units mirror csrc/pds_rollout_hist_*.hip: the same variants, hn = rollout_hist_tiles(H x half))
bool launch_evaluate_hist_hover(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_circle(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_takeoff(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_hover_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_circle_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
// ... and the record form's, csrc/pds_evaluate_hist_record_*.hip: the same variants once more
bool launch_evaluate_hist_record_hover(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_circle(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_takeoff(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_hover_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_circle_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
// ... and the stats form's, csrc/pds_evaluate_hist_stats_*.hip: the same variants a third time
bool launch_evaluate_hist_stats_hover(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_circle(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_takeoff(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_hover_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_circle_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
// ... and the three forms on the latency ring, csrc/pds_evaluate_hist_<task>[_pid]_lat.hip and
// csrc/pds_evaluate_hist_lat_{record,stats}_<task>[_pid].hip: the variants of csrc/pds_rollout_hist_*_lat.hip
// (rollout_hist_latency_supported: Hover and Circle)
bool launch_evaluate_hist_hover_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_circle_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_hover_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_circle_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka);
bool launch_evaluate_hist_record_hover_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_circle_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_hover_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_record_circle_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistRecordArgs &ka);
bool launch_evaluate_hist_stats_hover_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_circle_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_hover_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);
bool launch_evaluate_hist_stats_circle_pid_lat(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistStatsArgs &ka);

}  // namespace pds
