/* pds_history_stats.h -- the entry points that stand beside the C ABI of include/pds.h: the one-launch evaluation of
 * observation-history policies that also sums the observations the policies acted on.  A header of its own, like
 * include/pds_history_record.h and for its reason: include/pds.h and its table in the Python binding (native.SIGNATURES) are pinned
 * entry for entry by tests/test_host_cpu.py; this header and native.HISTORY_STATS_SIGNATURES are held to the same comparison by
 * tests/test_evaluate_history_stats_cpu.py.  The library exports the symbols like every other. */
#ifndef PDS_HISTORY_STATS_H
#define PDS_HISTORY_STATS_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where pds_evaluate_policies_history_stats has a kernel for this handle and this observation_history_size, 0 where it has
 * none: what pds_evaluate_history_supported asks, and that the stats form is built for the input width
 * W = 64 / 96 / 128 / 192 >= history * half.  PDS_EINVAL for a NULL handle. */
int pds_evaluate_history_stats_supported(const pds_handle *h, int history);

/* pds_evaluate_policies_history that also SUMS the histories its policies acted on (csrc/pds_evaluate_hist.h, the stats form): the
 * sums of pds_evaluate_policies_stats for history policies.  d_obs_sums [tiles, 4, 2, W] float32, 16-byte aligned, tiles =
 * P * episodes_per_policy / 64 and W = 64, 96, 128 or 192, the smallest of them >= history * half: per 64-env tile and network
 * wave (the 16 envs 16 w .. 16 w + 15 of the tile), S1 = sum d and S2 = sum d * d per input k < history * half, d = the input
 * minus d_mean[p][k] (the input itself without statistics), over every step s < d_len of the wave's envs, steps in order, one
 * rounded float32 operation per difference, product and sum, the 16 envs added in the fixed tree rows j and j + 8, then + 4, + 2,
 * + 1.  Columns >= history * half are zero; the whole slab is written.  The four waves of a tile and the tiles of a policy are
 * the caller's to add.  d_ret / d_len / d_cost / d_metrics (optional) are the bits of pds_evaluate_policies_history; the slab is
 * bitwise what the per-step loop named there sums.  history = 2 is accepted: the slab then is pds_evaluate_policies_stats' on
 * the bits.  Behind the checks of pds_evaluate_policies_history PDS_EINVAL for a d_obs_sums that is NULL or not 16-byte aligned,
 * then PDS_EUNSUPPORTED where pds_evaluate_history_stats_supported answers 0.  The state of the handle afterwards is
 * pds_evaluate_policies'; a refused call leaves the handle as it was. */
int pds_evaluate_policies_history_stats(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                        const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                        const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                        float *d_obs_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HISTORY_STATS_H */
