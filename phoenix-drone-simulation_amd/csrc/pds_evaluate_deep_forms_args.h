// pds_evaluate_deep_forms_args.h -- launch interface of the STATS and RECORD forms of the fused evaluation of policies with THREE or
// FOUR hidden layers (csrc/pds_evaluate_deep.h; entry points pds_evaluate_policies_deep_stats / _deep_record in csrc/pds_api.hip,
// include/pds_evaluate_deep_forms.h).  The plain / metrics form keeps EvalDeepArgs of csrc/pds_evaluate_deep_args.h as it is.
#pragma once
#include "../../include/pds_evaluate_deep_forms.h"
#include "pds_evaluate_deep_args.h"

namespace pds {

// Arguments of evaluate_deep_kernel<V, L, EvalForm::Stats>: the stats kernel's block (csrc/pds_evaluate_args.h) -- m.metrics NULL
// where the caller wants none, obs_sums [tiles, 4, 2, 64] -- and behind it the network's shape, as in EvalDeepArgs.
struct EvalDeepStatsArgs {
  EvalStatsArgs st;      // FIRST member (the kernel reads the head of its argument block as an EvalMetricsArgs, that as an EvalArgs)
  pds_mlp_deep deep;     // d_in, n_hidden, hidden[], d_out, activation of every policy; its pointers are not read
  int deep_param_count;  // floats of a row of params (pds_mlp_deep_param_count layout)
};
// Arguments of evaluate_deep_kernel<V, L, EvalForm::Record>: the record kernel's block and behind it the network's shape.
struct EvalDeepRecordArgs {
  EvalRecordArgs r;      // FIRST member (as above; flight, obs_rec or NULL, rec_tiles)
  pds_mlp_deep deep;
  int deep_param_count;
};
static_assert(offsetof(EvalDeepStatsArgs, st) == 0, "the deep stats kernel reads the head of its argument block as an EvalStatsArgs");
static_assert(offsetof(EvalDeepRecordArgs, r) == 0, "the deep record kernel reads the head of its argument block as an EvalRecordArgs");
// the blocks are the kernels' argument segments: size and the place of the last member, as the compiler laid them out
static_assert(sizeof(EvalDeepStatsArgs) == 856 && offsetof(EvalDeepStatsArgs, deep) == 736 && offsetof(EvalDeepStatsArgs, deep_param_count) == 848,
              "the kernarg layout of the deep stats form");
static_assert(sizeof(EvalDeepRecordArgs) == 872 && offsetof(EvalDeepRecordArgs, deep) == 752 && offsetof(EvalDeepRecordArgs, deep_param_count) == 864,
              "the kernarg layout of the deep record form");

// form -> the argument block of evaluate_deep_kernel<V, L, F> (Metrics: the plain and the metrics call, one code object)
template <EvalForm F> struct EvalDeepKernelArgsOf;
template <> struct EvalDeepKernelArgsOf<EvalForm::Metrics> { using type = EvalDeepArgs; };
template <> struct EvalDeepKernelArgsOf<EvalForm::Stats> { using type = EvalDeepStatsArgs; };
template <> struct EvalDeepKernelArgsOf<EvalForm::Record> { using type = EvalDeepRecordArgs; };
template <EvalForm F> using EvalDeepKernelArgs = typename EvalDeepKernelArgsOf<F>::type;
// ... and the EvalMetricsArgs at its head, on the host and on the device
__host__ __device__ inline const EvalMetricsArgs &eval_deep_head(const EvalDeepArgs &ka) { return ka.m; }
__host__ __device__ inline const EvalMetricsArgs &eval_deep_head(const EvalDeepStatsArgs &ka) { return ka.st.m; }
__host__ __device__ inline const EvalMetricsArgs &eval_deep_head(const EvalDeepRecordArgs &ka) { return ka.r.m; }
__host__ __device__ inline EvalMetricsArgs &eval_deep_head(EvalDeepArgs &ka) { return ka.m; }
__host__ __device__ inline EvalMetricsArgs &eval_deep_head(EvalDeepStatsArgs &ka) { return ka.st.m; }
__host__ __device__ inline EvalMetricsArgs &eval_deep_head(EvalDeepRecordArgs &ka) { return ka.r.m; }

// The variants of evaluate_deep_family (csrc/pds_evaluate_deep_args.h) whose stats / record code object may be launched.  A
// variant whose env wave spilled VGPRs where its metrics twin does not would be listed here and answer "not built"
// (profiles/evaluate_deep_forms_kernel_resources.txt: none does).
inline bool evaluate_deep_forms_variant_built(int task, const LaunchFlags &f, int n_hidden, EvalForm /*form*/) {
  return evaluate_deep_variant_built(task, f, n_hidden);
}

// one translation unit per (form, task, depth): csrc/pds_evaluate_{stats,record}_deep_<task>_l{3,4}.hip
#define PDS_EVALUATE_DEEP_FORM_DECL(FORM, ARGS)                                                                        \
  bool launch_evaluate_##FORM##_deep_hover_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const ARGS &ka);         \
  bool launch_evaluate_##FORM##_deep_hover_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const ARGS &ka);         \
  bool launch_evaluate_##FORM##_deep_circle_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const ARGS &ka);        \
  bool launch_evaluate_##FORM##_deep_circle_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const ARGS &ka);        \
  bool launch_evaluate_##FORM##_deep_takeoff_l3(const LaunchFlags &f, dim3 grid, hipStream_t s, const ARGS &ka);       \
  bool launch_evaluate_##FORM##_deep_takeoff_l4(const LaunchFlags &f, dim3 grid, hipStream_t s, const ARGS &ka);
PDS_EVALUATE_DEEP_FORM_DECL(stats, EvalDeepStatsArgs)
PDS_EVALUATE_DEEP_FORM_DECL(record, EvalDeepRecordArgs)
#undef PDS_EVALUATE_DEEP_FORM_DECL

}  // namespace pds
