/* pds_evaluate_deep_forms.h -- the entry points that stand beside include/pds_evaluate_deep.h: the STATS and the RECORD form of
 * the one-launch evaluation of a population of policies with THREE or FOUR hidden layers (csrc/pds_evaluate_deep.h) -- what
 * pds_evaluate_policies_stats and pds_evaluate_policies_record (include/pds.h) are to pds_evaluate_policies_metrics.  A header of
 * its own, for the reason include/pds_evaluate_deep.h has one: that header and native.EVALUATE_DEEP_SIGNATURES are pinned entry
 * for entry by tests/test_evaluate_deep_cpu.py; this header and native.EVALUATE_DEEP_FORMS_SIGNATURES are held to the same
 * comparison by tests/test_evaluate_deep_forms_cpu.py.  The library exports the symbols like every other. */
#ifndef PDS_EVALUATE_DEEP_FORMS_H
#define PDS_EVALUATE_DEEP_FORMS_H

#include "pds_evaluate_deep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the `form` of pds_evaluate_deep_forms_supported */
#define PDS_EVALUATE_DEEP_FORM_STATS 0  /* pds_evaluate_policies_deep_stats */
#define PDS_EVALUATE_DEEP_FORM_RECORD 1 /* pds_evaluate_policies_deep_record */

/* 1 where the entry point of `form` has a kernel for this handle and this network shape, 0 where it has none; host only.  1 needs
 * everything pds_evaluate_deep_supported (include/pds_evaluate_deep.h) needs, and the form's code object of the env's variant at
 * the shape's depth to be one the library launches (profiles/evaluate_deep_forms_kernel_resources.txt).  PDS_EINVAL for a NULL
 * handle or shape, or a form that is neither of the two above. */
int pds_evaluate_deep_forms_supported(const pds_handle *h, const pds_mlp_deep *shape, int32_t form);

/* pds_evaluate_policies_deep with the observation sums of pds_evaluate_policies_stats (include/pds.h) from the same launch:
 * d_obs_sums [tiles, 4, 2, 64] floats, 16-byte aligned -- tile, network wave, S1 / S2, feature; per feature k < D the sums of
 * d = o_k(s) - mean[p][k] (d = o_k without d_mean) and d * d over every observation a first-episode policy acted on, one rounded
 * instruction per difference, product and sum, the 16 rows of a wave added in the tree 8, 4, 2, 1, features >= D zero.  Bitwise
 * what max_steps x (pds_mlp_deep_forward per policy + pds_step) and the same sums in the same order give.
 * Semantics, argument checks, alignment rules and the state of the handle afterwards are pds_evaluate_policies_stats'; the struct
 * and family checks are pds_evaluate_policies_deep's, and so is d_metrics: optional, NULL: summed, not stored.  PDS_EINVAL, before
 * any device call, for a NULL d_obs_sums or one that is not 16-byte aligned and for everything pds_evaluate_policies_deep answers
 * PDS_EINVAL to; PDS_EUNSUPPORTED where pds_evaluate_deep_forms_supported(h, shape, PDS_EVALUATE_DEEP_FORM_STATS) is 0.  A refused
 * call leaves the handle as it was and writes nothing. */
int pds_evaluate_policies_deep_stats(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                                     const float *d_params, const float *d_mean, const float *d_std, float eps, int32_t max_steps,
                                     const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                     float *d_obs_sums, void *stream);

/* pds_evaluate_policies_deep with the recorded flights of pds_evaluate_policies_record (include/pds.h) from the same launch: of
 * every policy's first record_per_policy envs (a positive multiple of 64 up to episodes_per_policy) the state x(s) and the raw
 * action a(s) of every step the env's first episode was alive in front of, to d_flight [max_steps, 4, N_rec, 4] floats (16-byte
 * aligned, N_rec = P x record_per_policy), and, where d_obs_rec [max_steps, N_rec, D] is given, the raw observation o(s).  Nothing
 * else is written: rows past an episode's end keep what the caller put there.
 * Semantics, argument checks, alignment rules and the state of the handle afterwards are pds_evaluate_policies_record's -- the
 * record's own checks come first --; the struct and family checks are pds_evaluate_policies_deep's.  PDS_EUNSUPPORTED where
 * pds_evaluate_deep_forms_supported(h, shape, PDS_EVALUATE_DEEP_FORM_RECORD) is 0.  A refused call leaves the handle as it was and
 * writes nothing. */
int pds_evaluate_policies_deep_record(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                                      const float *d_params, const float *d_mean, const float *d_std, float eps, int32_t max_steps,
                                      const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                      int64_t record_per_policy, float *d_flight, float *d_obs_rec, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_EVALUATE_DEEP_FORMS_H */
