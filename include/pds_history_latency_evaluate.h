/* pds_history_latency_evaluate.h -- the entry points that stand beside the C ABI of include/pds.h: the one-launch evaluation of
 * observation-history policies on the latency ring.  A header of its own, like include/pds_history_latency.h and for its reason:
 * include/pds.h, include/pds_history_latency.h and their tables in the Python binding (native.SIGNATURES,
 * native.HISTORY_LATENCY_SIGNATURES) are pinned entry for entry by existing tests; this header and
 * native.HISTORY_LATENCY_EVALUATE_SIGNATURES are held to the same comparison by tests/test_history_latency_evaluate_cpu.py.  The
 * library exports the symbols like every other. */
#ifndef PDS_HISTORY_LATENCY_EVALUATE_H
#define PDS_HISTORY_LATENCY_EVALUATE_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where pds_evaluate_policies_history_latency and pds_evaluate_policies_history_latency_record (the same variant set) have a
 * kernel for this handle and this observation_history_size, 0 where they have none.  Built: what
 * pds_rollout_history_latency_supported names -- Hover and Circle on the latency ring in every control mode, with and without motor
 * dynamics, noise off or the reference's default, auto_reset = 1, history x half <= 192.  Not built: TakeOff, the Kalman hold, the
 * ground effect, partial noise; and a handle WITHOUT the ring -- that is pds_evaluate_policies_history's, and
 * pds_evaluate_history_supported answers a ring handle 0 as before.  PDS_EINVAL for a NULL handle. */
int pds_evaluate_history_latency_supported(const pds_handle *h, int history);

/* ... and where pds_evaluate_policies_history_latency_stats has: the same question, and the stats form built for the input width
 * W = 64 / 96 / 128 / 192 >= history * half. */
int pds_evaluate_history_latency_stats_supported(const pds_handle *h, int history);

/* pds_evaluate_policies_history on the latency ring (csrc/pds_evaluate_hist.h with the ring in memory, as pds_evaluate_policies
 * flies it at history = 2): the same arguments, buffers and outcome, and the histories the actors read are those of
 * pds_history_advance_latency step by step -- the step count of the rule is the handle's own (PDS_F_STEP_COUNT), as in
 * pds_rollout_history_latency.  Bit for bit the per-step loop (pds_mlp_forward + pds_step + pds_history_advance_latency).  Behind
 * the checks of pds_evaluate_policies_history PDS_EUNSUPPORTED where pds_evaluate_history_latency_supported answers 0; a refused
 * call leaves the handle as it was.  The state of the handle afterwards is pds_evaluate_policies'. */
int pds_evaluate_policies_history_latency(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                          const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                          const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                          void *stream);

/* pds_evaluate_policies_history_record on the latency ring: d_flight [T, 4, N_rec, 4] and, where given, d_obs_rec
 * [T, N_rec, history x half] as include/pds_history_record.h states them; the recorded histories show the rule above. */
int pds_evaluate_policies_history_latency_record(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                 const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                 const float *d_std, float eps, int max_steps, const float *d_obs0, float *d_ret,
                                                 float *d_len, float *d_cost, float *d_metrics, int64_t record_per_policy,
                                                 float *d_flight, float *d_obs_rec, void *stream);

/* pds_evaluate_policies_history_stats on the latency ring: d_obs_sums [tiles, 4, 2, W] as include/pds_history_stats.h states it,
 * summed over the histories the policies acted on, the rule above included.  PDS_EUNSUPPORTED where
 * pds_evaluate_history_latency_stats_supported answers 0. */
int pds_evaluate_policies_history_latency_stats(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                const float *d_std, float eps, int max_steps, const float *d_obs0, float *d_ret,
                                                float *d_len, float *d_cost, float *d_metrics, float *d_obs_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HISTORY_LATENCY_EVALUATE_H */
