/* pds_evaluate_deep.h -- the entry points that stand beside the C ABI of include/pds.h: the one-launch evaluation of a population
 * of policies with THREE or FOUR hidden layers (csrc/pds_evaluate_deep.h) -- the (50, 30, 20) and (32, 32, 32, 32) actors of the
 * reference's architecture search, which struct pds_mlp of pds_evaluate_policies has no room for.  A header of its own, like
 * include/pds_mlp_deep.h and for its reason: include/pds.h and native.SIGNATURES are pinned entry for entry by
 * tests/test_host_cpu.py; this header and native.EVALUATE_DEEP_SIGNATURES are held to the same comparison by
 * tests/test_evaluate_deep_cpu.py.  The library exports the symbols like every other. */
#ifndef PDS_EVALUATE_DEEP_H
#define PDS_EVALUATE_DEEP_H

#include "pds.h"
#include "pds_mlp_deep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where pds_evaluate_policies_deep has a kernel for this handle and this network shape, 0 where it has none; host only.  1 needs
 * all of: a handle created with auto_reset; observation_history_size 2 (the handle's own row is the network input); an env
 * configuration of the family the kernel is built for -- control_mode PWM, no latency ring, no Kalman hold, every noise setting,
 * motor dynamics on Hover and Circle, the ground effect on TakeOff --; a shape inside struct pds_mlp_deep's range (n_hidden 3 or
 * 4, every hidden width 1..64, activation 0 or 1); shape->d_in == pds_obs_dim(h); shape->d_out == 4.  The struct's pointers are
 * not read.  PDS_EINVAL for a NULL handle or shape. */
int pds_evaluate_deep_supported(const pds_handle *h, const pds_mlp_deep *shape);

/* pds_evaluate_policies_metrics (include/pds.h) for policies with three or four hidden layers: P policies x episodes_per_policy
 * episodes in one launch, action = actor mean, return, length and cost of every env's first episode to d_ret, d_len, d_cost [N]
 * and, where d_metrics [N, PDS_EVAL_METRICS] (16-byte aligned) is given, the PDS_EM_* flight metrics from the same launch; NULL:
 * summed, not stored.  Bitwise what max_steps x (pds_mlp_deep_forward per policy + pds_step) and the same sums in the same order
 * give.
 *   shape     d_in = D, n_hidden, hidden[], d_out = 4, activation of EVERY policy; its pointers are not read
 *   d_params  [P, pds_mlp_deep_param_count(shape)]: row p = W1 b1 ... W(L+1) b(L+1) of policy p, torch order
 *   d_mean, d_std [P, D] (both or none), eps: (o - mean[p]) / (std[p] + eps) in front of policy p
 * Semantics, argument checks and the state of the handle afterwards are pds_evaluate_policies_metrics', word for word: PDS_EINVAL,
 * before any device call, for a NULL pointer (d_metrics apart), P x episodes_per_policy != num_envs, episodes_per_policy not a
 * multiple of 64, a shape outside the range or with d_in != D or d_out != 4, max_steps < 1, a misaligned d_metrics, a handle that
 * was never reset; PDS_EUNSUPPORTED for a handle without auto_reset or an env configuration outside the family above
 * (pds_evaluate_deep_supported says so beforehand) -- a refused call leaves the handle as it was and writes nothing.  After a
 * successful call the handle is in the "not reset" state, as after pds_evaluate_policies. */
int pds_evaluate_policies_deep(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                               const float *d_params, const float *d_mean, const float *d_std, float eps, int32_t max_steps,
                               const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_EVALUATE_DEEP_H */
