/* pds_mlp_broad.h -- the entry points that stand beside the C ABI of include/pds.h for two-hidden-layer MLPs with a hidden width
 * ABOVE 64: forward, value-regression gradient and Adam step (csrc/pds_mlp_broad.hip), and DDPG's policy gradient, Bellman backup
 * and polyak step on such networks (csrc/pds_ddpg_broad.hip).  The reference's default for both off-policy trainers is
 * hidden_sizes (400, 300) with relu (algs/ddpg/defaults.py, algs/sac/defaults.py); include/pds.h stops at 64.
 * A header of its own, like include/pds_mlp_deep.h and for its reason: include/pds.h and native.SIGNATURES are pinned entry for
 * entry by tests/test_host_cpu.py; this header and native.MLP_BROAD_SIGNATURES are held to the same comparison by
 * tests/test_mlp_broad_cpu.py.  The library exports the symbols like every other. */
#ifndef PDS_MLP_BROAD_H
#define PDS_MLP_BROAD_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_MLP_BROAD_MAX_HIDDEN 512
#define PDS_MLP_BROAD_MAX_BATCH 65536 /* of the gradient calls: their workspace holds the activations of a whole batch */

/* The networks are struct pds_mlp of include/pds.h; its fields have room, only the range differs.  Range of these entry points:
 * h1, h2 in 1..512 with AT LEAST ONE of them above 64 (a shape with both at most 64 belongs to the entry points of include/pds.h:
 * PDS_EINVAL, and the text of pds_last_error(NULL) names them), d_in 1..64 (65..192 is a valid network that these kernels do not
 * cover: PDS_EUNSUPPORTED), d_out 1..8, activation 0 relu or 1 tanh.  Widths need not be multiples of 16 or of 4.
 *
 * Every entry point below takes the semantics of the include/pds.h entry point of the same name without `_broad`, word for word:
 * the flat layout W1 b1 W2 b2 W3 b3 in torch order, the standardisation (x - mean) / (std + eps), the optional row index,
 * d_stats[4], opt == NULL for no step, the rule for a valid opt, the row-wise write of the Bellman backup, the two rounded
 * products of the polyak step.
 * Checks: PDS_EINVAL before any device call for a NULL struct, tensor or argument pointer (other than d_index, d_mean / d_std and
 * opt), B < 1, a width or activation outside the range, d_out != 1 for the value gradient, a bad opt, an actor with d_out != 4, a
 * Q network with d_out != 1 or d_in != D + 4, a polyak outside [0, 1] or between networks of different shape; PDS_EUNSUPPORTED
 * behind them for D + 4 > 64 and for a gradient call with B > PDS_MLP_BROAD_MAX_BATCH.
 * Every launch goes to the caller's stream, allocates nothing and does not synchronise (capturable into a hipGraph).  Gradients
 * are summed in a fixed order without atomics: the same inputs give the same bits, and a gradient call with opt gives the bits of
 * the call without it followed by pds_mlp_broad_adam_step.  d_workspace of a gradient call: pds_mlp_broad_workspace_floats(m) /
 * pds_ddpg_broad_workspace_floats(pi, q) floats -- the activations and pre-activation gradients of a batch of up to
 * PDS_MLP_BROAD_MAX_BATCH samples between the chain kernel and the weight-gradient kernel, and the latter's partial sums. */

int pds_mlp_broad_supported(const pds_mlp *m);            /* 1 / 0; host only */
int pds_mlp_broad_param_count(const pds_mlp *m);          /* flat layout W1 b1 W2 b2 W3 b3, torch order; < 0 outside the range */
int64_t pds_mlp_broad_workspace_floats(const pds_mlp *m); /* host only; < 0 where pds_mlp_broad_supported answers 0 */
int pds_mlp_broad_forward(const pds_mlp *m, const float *d_x, const int64_t *d_index, int64_t B, const float *d_mean,
                          const float *d_std, float eps, float *d_y, void *stream);
int pds_mlp_broad_value_grad_step(const pds_mlp *m, const float *d_x, const int64_t *d_index, const float *d_target, int64_t B,
                                  float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream);
int pds_mlp_broad_adam_step(const pds_mlp *m, const float *d_grads, float *d_exp_avg, float *d_exp_avg_sq, int64_t step, float lr,
                            float beta1, float beta2, float eps, void *stream);

/* pi: D -> h1 -> h2 -> 4, q: D + 4 -> h1' -> h2' -> 1, each inside the range above (so each with a width above 64) */
int pds_ddpg_broad_supported(const pds_mlp *pi, const pds_mlp *q);
int64_t pds_ddpg_broad_workspace_floats(const pds_mlp *pi, const pds_mlp *q); /* host only */
int pds_ddpg_broad_policy_grad(const pds_mlp *pi, const pds_mlp *q, const float *d_oa, const int64_t *d_index, int64_t B,
                               float act_limit, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                               void *stream);
int pds_ddpg_broad_target(const pds_mlp *pi_targ, const pds_mlp *q_targ, const float *d_obs2, const int64_t *d_index, int64_t B,
                          const float *d_rew, const float *d_done, float gamma, float act_limit, float *d_target_rows,
                          void *stream);
int pds_polyak_broad(const pds_mlp *targ, const pds_mlp *src, double polyak, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_MLP_BROAD_H */
