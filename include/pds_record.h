/*
 * pds_record.h -- one more entry point of libpds_hip.so, next to the C ABI of pds.h: the population evaluation that also
 * records the flights it scores.  It stands in a header of its own because pds.h and the binding's table of its prototypes
 * (native.SIGNATURES) are pinned to each other, entry point by entry point and by their number (tests/test_host_cpu.py); this
 * header and its own table (native.RECORD_SIGNATURES) are pinned to each other in the same way (tests/test_evaluate_record_cpu.py).
 * Conventions -- device pointers `d_*`, return codes, the stream, thread safety -- are those of pds.h.
 */
#ifndef PDS_RECORD_H
#define PDS_RECORD_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pds_evaluate_policies_metrics (d_metrics may be NULL here) that also RECORDS the flights it scores (csrc/pds_evaluate.h, RECORD):
 * of every policy's episodes_per_policy envs the first record_per_policy -- a positive multiple of 64, at most episodes_per_policy
 * -- are recorded, N_rec = P * record_per_policy columns, column j = p * record_per_policy + e for env e of policy p.
 * d_flight [max_steps, 4, N_rec, 4] float32, 16-byte aligned: for step s and column j four pieces of four floats,
 *     piece 0 = (px, py, pz, vx), 1 = (vy, vz, roll, pitch), 2 = (yaw, wx, wy, wz) of x(s), 3 = a(s),
 * x(s) the true state the policy acted in (what the PDS_EM_* sums are taken over) and a(s) the raw action handed to step s:
 * together the twelve columns of a flight log and the four commands.
 * d_obs_rec [max_steps, N_rec, D] float32 or NULL: the raw (unstandardised) observation o(s) the policy acted on.
 * Only the rows s < d_len of a recorded env are written; every other element keeps what the caller put there (zero-fill the
 * buffers).  Not recorded: the terminal state x(L) and the terminal observation -- a finished env is reset in place inside the step.
 * d_ret / d_len / d_cost / d_metrics are the bits of pds_evaluate_policies_metrics.  Checks, support (pds_evaluate_supported) and
 * the state of the handle afterwards are pds_evaluate_policies'; in front of them PDS_EINVAL for a record_per_policy that is not
 * a positive multiple of 64 or exceeds episodes_per_policy, a NULL or misaligned d_flight, or a d_obs_rec that is not 4-byte
 * aligned. */
int pds_evaluate_policies_record(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                 const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                 const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                 int64_t record_per_policy, float *d_flight, float *d_obs_rec, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_RECORD_H */
