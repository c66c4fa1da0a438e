/* pds_history_latency.h -- the entry points that stand beside the C ABI of include/pds.h: observation histories other than 2 on
 * the latency ring.  A header of its own, like include/pds_history_record.h and for its reason: include/pds.h and its table in the
 * Python binding (native.SIGNATURES) are pinned entry for entry by tests/test_host_cpu.py; this header and
 * native.HISTORY_LATENCY_SIGNATURES are held to the same comparison by tests/test_history_latency_cpu.py.  The library exports the
 * symbols like every other. */
#ifndef PDS_HISTORY_LATENCY_H
#define PDS_HISTORY_LATENCY_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pds_history_advance for an env that delays its actions through the latency ring (csrc/pds_history.hip).  The reference's
 * action_history holds VIEWS of action_buffer[-1] after a reset (envs/agents.py:386, envs/base.py:424-429): at the j-th env.step
 * after a reset, j = 1, 2, ..., the action columns (the last 4 floats) of the history slots 0 .. history - j show what that ring
 * row holds now.  After the shift-and-append of pds_history_advance, where j <= history and
 * floor(j * agg / lat_steps) > floor((j - 1) * agg / lat_steps), those columns become the step's raw action d_actions[env]
 * ([n, 4], what was handed to pds_step), in d_hist_out and in d_final_hist alike; then the restart of the finished envs as in
 * pds_history_advance.  d_steps_in [n] int32: j - 1 per env, the env.step()s since its last reset; d_steps_out [n] (another
 * array) takes j, or 0 for an env that auto-reset.  The caller zeroes the count of an env it resets; a count >= history switches
 * the rule off for that env until then (what CrazyFlieAgent.set_latency leaves: a new ring, the views keep the old one).
 * lat_steps = pds_latency_steps of the handle that stepped, agg its aggregate_phy_steps.  lat_steps == 0: the bits of
 * pds_history_advance.  PDS_EINVAL as pds_history_advance, and for half < 5, a NULL d_actions / d_steps_in / d_steps_out,
 * d_steps_in == d_steps_out, lat_steps < 0 or agg outside 1 .. 4096. */
int pds_history_advance_latency(int64_t n, int half, int history, const float *d_obs2, const uint8_t *d_terminated,
                                const uint8_t *d_truncated, const float *d_final_obs2, int auto_reset, const float *d_hist_in,
                                float *d_hist_out, float *d_final_hist, const float *d_actions, const int32_t *d_steps_in,
                                int32_t *d_steps_out, int lat_steps, int agg, void *stream);

/* 1 where pds_rollout_history_latency has a kernel for this handle and this observation_history_size, 0 where it has none.  Built:
 * Hover and Circle on the latency ring (use_latency, or pds_set_latency >= one time step) in every control mode, with and without
 * motor dynamics, noise off or the reference's default, auto_reset = 1, history x half <= 192.  Not built: TakeOff, the Kalman
 * hold, the ground effect, partial noise; and a handle WITHOUT the ring -- that is pds_rollout_history's.  PDS_EINVAL for a NULL
 * handle. */
int pds_rollout_history_latency_supported(const pds_handle *h, int history);

/* pds_rollout_history on the latency ring (csrc/pds_rollout_hist.h with the ring in memory, as pds_rollout flies it): the same
 * arguments, buffers and outcome, and the histories in d_obs_buf / d_fin_rows are those of pds_history_advance_latency step by
 * step -- the step count of the rule is the handle's own (PDS_F_STEP_COUNT), so a caller that froze its views with
 * pds_set_latency in the middle of an episode steps per step until the next reset.  Bit for bit the per-step rollout
 * (pds_mlp_forward + pds_gaussian_sample_dev + pds_step + pds_history_advance_latency + pds_rollout_record).  Behind the checks
 * of pds_rollout_history PDS_EUNSUPPORTED where pds_rollout_history_latency_supported answers 0; a refused call leaves the handle
 * as it was. */
int pds_rollout_history_latency(pds_handle *h, int T, int history, const pds_mlp *pi, const float *d_mean, const float *d_std,
                                float eps, const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset,
                                int deterministic, float *d_obs_buf, float *d_act_buf, float *d_logp_buf, float *d_rew_buf,
                                uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows, int32_t *d_fin_step,
                                int slots, float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HISTORY_LATENCY_H */
