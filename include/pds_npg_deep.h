/* pds_npg_deep.h -- the entry points that stand beside the C ABI of include/pds.h: the natural-gradient policy step of NPG and
 * TRPO -- Fisher-vector product and line-search candidates -- for actors with THREE or FOUR hidden layers, struct pds_mlp_deep of
 * include/pds_mlp_deep.h (csrc/pds_npg_deep.hip).  The reference's architecture search (experiments/01_find_NN_architecture)
 * trains its (50, 30, 20) and (32, 32, 32, 32) actors with --alg trpo; pds_npg_fisher_vector_product and pds_npg_surrogate_kl take
 * struct pds_mlp, which has room for two hidden layers.  The conjugate-gradient iteration, pds_npg_cg_step, takes no network and
 * serves both depths.
 * A header of its own, like include/pds_mlp_deep.h and for its reason: include/pds.h and native.SIGNATURES are pinned entry for
 * entry by tests/test_host_cpu.py, include/pds_mlp_deep.h and native.MLP_DEEP_SIGNATURES by tests/test_mlp_deep_cpu.py; this header
 * and native.NPG_DEEP_SIGNATURES are held to the same comparison by tests/test_npg_deep_cpu.py.  The library exports the symbols
 * like every other. */
#ifndef PDS_NPG_DEEP_H
#define PDS_NPG_DEEP_H

#include "pds_mlp_deep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every entry point below takes the semantics of the pds_mlp entry point of the same name (include/pds.h: pds_npg_workspace_floats,
 * pds_npg_fisher_vector_product, pds_npg_surrogate_kl), word for word: d_x holds rows that are already standardised, the optional
 * row index of the Fisher product, d_out = F v + damping v over the flat layout W1 b1 ... W(L+1) b(L+1) with d_out allowed to alias
 * d_v, the candidates theta + fracs[j] * step with product and sum rounded separately, d_out[j] = {sum ratio adv, sum KL, non-finite
 * flag, sum ratio}, the optional d_theta_out [num_candidates][param_count].
 * Checks: those of include/pds_mlp_deep.h for the struct (at n_hidden == 2 the text of pds_last_error(NULL) names pds_mlp), and
 * PDS_EINVAL before any device call for a NULL tensor pointer (d_index and d_theta_out may be NULL), B < 1, num_candidates outside
 * 1..65535 (negative for the workspace query); PDS_EUNSUPPORTED behind them for d_in 65..192, where the workspace query is negative
 * too.  Every launch goes to the caller's stream, allocates nothing and does not synchronise (capturable into a hipGraph).  Partial
 * sums are added in a fixed order without atomics: the same inputs give the same bits. */

/* floats of d_workspace for both calls below: the larger of (waves of the largest grid) x param_count and waves x 3 x
 * num_candidates; host only */
int64_t pds_npg_deep_workspace_floats(const pds_mlp_deep *m, int num_candidates);
int pds_npg_deep_fisher_vector_product(const pds_mlp_deep *m, const float *d_x, const int64_t *d_index, int64_t B,
                                       const float *d_log_std, const float *d_v, float damping, float *d_out, float *d_workspace,
                                       void *stream);
int pds_npg_deep_surrogate_kl(const pds_mlp_deep *m, const float *d_step, const float *d_fracs, int num_candidates,
                              const float *d_x, const float *d_act, const float *d_adv, const float *d_logp_old,
                              const float *d_mu_old, const float *d_log_std, int64_t B, float *d_out, float *d_theta_out,
                              float *d_workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_NPG_DEEP_H */
