/* pds_mlp_deep.h -- the entry points that stand beside the C ABI of include/pds.h: forward, PPO-clip policy gradient and
 * value-regression gradient, each with the Adam step that may ride on it, for MLPs with THREE or FOUR hidden layers
 * (csrc/pds_mlp_deep.hip).  struct pds_mlp of include/pds.h has room for two; the reference's architecture search
 * (experiments/01_find_NN_architecture) also grids (50, 30, 20), (40, 40, 40), (30, 30, 30), (32, 32, 32, 32), (25, 25, 25, 25).
 * A header of its own, like include/pds_history_stats.h and for its reason: include/pds.h and native.SIGNATURES are pinned entry
 * for entry by tests/test_host_cpu.py; this header and native.MLP_DEEP_SIGNATURES are held to the same comparison by
 * tests/test_mlp_deep_cpu.py.  The library exports the symbols like every other. */
#ifndef PDS_MLP_DEEP_H
#define PDS_MLP_DEEP_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_MLP_DEEP_MAX_HIDDEN 4

/* Linear, act, ... , Linear with n_hidden hidden layers, torch nn.Linear layout, device pointers.  Range: n_hidden 3 or 4 (two
 * hidden layers are struct pds_mlp's), every hidden width 1..64, d_out 1..8, d_in 1..64 (65..192 is a valid network that these
 * kernels do not cover: PDS_EUNSUPPORTED).  Pointers of unused layers (w[4], b[4] at n_hidden == 3) are never read. */
typedef struct pds_mlp_deep {
  int32_t d_in, n_hidden, hidden[PDS_MLP_DEEP_MAX_HIDDEN], d_out, activation;   /* 0 relu, 1 tanh */
  const float *w[PDS_MLP_DEEP_MAX_HIDDEN + 1], *b[PDS_MLP_DEEP_MAX_HIDDEN + 1]; /* layer l: w[l] [out][in], b[l] [out] */
} pds_mlp_deep;

/* Every entry point below takes the semantics of the pds_mlp entry point of the same name (include/pds.h), word for word: the
 * standardisation (x - mean) / (std + eps), the optional row index, d_stats[4], opt == NULL for no step, the rule for a valid opt.
 * Checks: PDS_EINVAL before any device call for a NULL struct or tensor pointer among the first n_hidden + 1 layers, B < 1, a
 * width or activation outside the range, n_hidden other than 3 or 4 (at 2 the text of pds_last_error(NULL) names pds_mlp),
 * d_out != 1 for the value gradient, a bad opt; PDS_EUNSUPPORTED behind them for d_in 65..192.  Every launch goes to the caller's
 * stream, allocates nothing and does not synchronise (capturable into a hipGraph).  Gradients are summed in a fixed order without
 * atomics: the same inputs give the same bits, and a gradient call with opt gives the bits of the call without it followed by
 * pds_mlp_deep_adam_step. */

int pds_mlp_deep_supported(const pds_mlp_deep *m);           /* 1 / 0; host only */
int pds_mlp_deep_param_count(const pds_mlp_deep *m);         /* flat layout W1 b1 ... W(L+1) b(L+1), torch order; < 0 outside the range */
int64_t pds_mlp_deep_workspace_floats(const pds_mlp_deep *m); /* host only; < 0 where pds_mlp_deep_supported answers 0 */
int pds_mlp_deep_forward(const pds_mlp_deep *m, const float *d_x, const int64_t *d_index, int64_t B, const float *d_mean,
                         const float *d_std, float eps, float *d_y, void *stream);
int pds_mlp_deep_ppo_policy_grad_step(const pds_mlp_deep *m, const float *d_x, const float *d_act, const float *d_adv,
                                      const float *d_logp_old, const float *d_log_std, int64_t B, float clip_ratio,
                                      float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream);
int pds_mlp_deep_value_grad_step(const pds_mlp_deep *m, const float *d_x, const int64_t *d_index, const float *d_target,
                                 int64_t B, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream);
int pds_mlp_deep_adam_step(const pds_mlp_deep *m, const float *d_grads, float *d_exp_avg, float *d_exp_avg_sq, int64_t step,
                           float lr, float beta1, float beta2, float eps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_MLP_DEEP_H */
