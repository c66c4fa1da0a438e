/* pds_history_record.h -- the entry point that stands beside the C ABI of include/pds.h: the one-launch evaluation of
 * observation-history policies that also records the flights.  A header of its own: include/pds.h and its table in the Python
 * binding (native.SIGNATURES) are pinned entry for entry by tests/test_host_cpu.py; this header and native.HISTORY_RECORD_SIGNATURES
 * are held to the same comparison by tests/test_evaluate_history_record_cpu.py.  The library exports the symbol like every other. */
#ifndef PDS_HISTORY_RECORD_H
#define PDS_HISTORY_RECORD_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pds_evaluate_policies_history that also RECORDS the flights it scores (csrc/pds_evaluate_hist.h, the record): the record of
 * pds_evaluate_policies_record for history policies.  record_per_policy, N_rec, the column of an env and d_flight
 * [max_steps, 4, N_rec, 4] are that entry point's.  d_obs_rec [max_steps, N_rec, history * half] float32 or NULL: the raw
 * (unstandardised) history the policy acted on at step s, the network's whole input.  Only the rows s < d_len of a recorded env
 * are written; every other element keeps what the caller put there.  Not recorded: the terminal state and the terminal history.
 * d_ret / d_len / d_cost / d_metrics (optional) are the bits of pds_evaluate_policies_history; d_flight and d_obs_rec are bitwise
 * what the per-step loop named there reads in front of every step.  In front of the checks of pds_evaluate_policies_history
 * (support: pds_evaluate_history_supported, for both) PDS_EINVAL for a record_per_policy that is not a positive multiple of 64 or
 * exceeds episodes_per_policy, a NULL or misaligned d_flight, or a d_obs_rec that is not 4-byte aligned.  The state of the
 * handle afterwards is pds_evaluate_policies'; a refused call leaves the handle as it was. */
int pds_evaluate_policies_history_record(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                         const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                         const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                         int64_t record_per_policy, float *d_flight, float *d_obs_rec, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HISTORY_RECORD_H */
