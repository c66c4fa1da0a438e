/* pds_rollout_deep.h -- the entry points that stand beside the C ABI of include/pds.h: the one-launch rollout for ACTORS with
 * THREE or FOUR hidden layers (csrc/pds_rollout_deep.h) -- the (50, 30, 20) and (32, 32, 32, 32) actors of the reference's
 * architecture search (experiments/01_find_NN_architecture), which struct pds_mlp of pds_rollout has no room for.  A header of its
 * own, like include/pds_evaluate_deep.h and for its reason: include/pds.h and native.SIGNATURES are pinned entry for entry by
 * tests/test_host_cpu.py; this header and native.ROLLOUT_DEEP_SIGNATURES are held to the same comparison by
 * tests/test_rollout_deep_cpu.py.  The library exports the symbols like every other. */
#ifndef PDS_ROLLOUT_DEEP_H
#define PDS_ROLLOUT_DEEP_H

#include "pds.h"
#include "pds_mlp_deep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where pds_rollout_deep has a kernel for this handle and this actor, 0 where it has none; host only.  1 needs all of: a handle
 * created with auto_reset; observation_history_size 2 (the handle's own row is the network input); an env configuration of the
 * family the kernel is built for -- control_mode PWM, no latency ring, no Kalman hold, every noise setting, motor dynamics on Hover
 * and Circle, the ground effect on TakeOff --; pi->n_hidden 3 or 4, every hidden width 1..64, activation 0 or 1;
 * pi->d_in == pds_obs_dim(h); pi->d_out == 4.  The struct's pointers are not read.  PDS_EINVAL for a NULL handle or actor. */
int pds_rollout_deep_supported(const pds_handle *h, const pds_mlp_deep *pi);

/* pds_rollout_history (include/pds.h) without the history and for an actor with three or four hidden layers: the T closed-loop
 * steps o -> standardise -> actor -> a = mu + sigma z, log p -> env.step(a) -> buffers in ONE launch.  The critic is NOT in the
 * kernel: the caller evaluates V over d_obs_buf and over the slot list afterwards (any critic depth).
 *   d_obs_buf  [T + 1, N, D]: row 0 = o(0) on entry (the env's current observation), row t + 1 = o(t + 1), written by step t
 *   d_act_buf  [T, N, 4] (16-byte aligned), d_logp_buf, d_rew_buf, d_cost_buf [T, N] float, d_term_buf, d_trunc_buf [T, N] uint8
 *   d_fin_rows [slots, N, D], d_fin_step [slots, N] int32, preset to -1 by the caller: an env that the TimeLimit cut in step t,
 *              or that finished in step T - 1, leaves its LAST observation row (the row of final_obs) in its next free slot and
 *              t in d_fin_step; slots >= T / max_episode_steps + 2
 *   d_ep_ret, d_ep_len [N] run on; d_stats[0..2] += return, length and count of the episodes that finished
 *   step t samples with call = *d_call_base (NULL: 0) + call_offset + t + 1: the draws of pds_gaussian_sample
 * Bitwise what T x (pds_mlp_deep_forward + pds_gaussian_sample + pds_step + pds_rollout_record) give (d_stats: the same sums,
 * added by atomics in another order).  PDS_EINVAL, before any device call, for a NULL pointer (d_mean / d_std: both or none;
 * d_call_base may be NULL), T < 1, slots < 1 or too few, an actor outside the range above or with a missing tensor among its
 * 2 (n_hidden + 1), a misaligned buffer, a handle that was never reset; PDS_EUNSUPPORTED for a handle without auto_reset or an env
 * configuration outside the family (pds_rollout_deep_supported says so beforehand) -- a refused call leaves the handle as it was
 * and writes nothing.  After a successful call the handle is T ticks further, as after T pds_step calls. */
int pds_rollout_deep(pds_handle *h, int T, const pds_mlp_deep *pi, const float *d_mean, const float *d_std, float eps,
                     const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset, int deterministic,
                     float *d_obs_buf, float *d_act_buf, float *d_logp_buf, float *d_rew_buf, uint8_t *d_term_buf,
                     uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows, int32_t *d_fin_step, int slots, float *d_ep_ret,
                     float *d_ep_len, float *d_stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_ROLLOUT_DEEP_H */
