/* pds_collect_control.h -- the entry points that stand beside the C ABI of include/pds.h: the fused off-policy collection under the
 * PID control modes and with the latency ring.  A header of its own, like include/pds_history_record.h and for its reason:
 * include/pds.h and its table in the Python binding (native.SIGNATURES) are pinned entry for entry by tests/test_host_cpu.py, and
 * what pds_collect and pds_collect_supported answer is pinned by tests/test_gpu_collect*.py; this header and
 * native.COLLECT_CONTROL_SIGNATURES are held to the same comparison by tests/test_collect_control_cpu.py.  The library exports the
 * symbols like every other. */
#ifndef PDS_COLLECT_CONTROL_H
#define PDS_COLLECT_CONTROL_H

#include "pds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where pds_collect_control has a kernel for this handle, this actor and this mode, 0 where it has none: 1 wherever
 * pds_collect_supported answers 1, and for Hover and Circle handles with control_mode AttitudeRate or Attitude and / or with the
 * latency ring -- noise all off or domain randomisation + thrust noise + observation noise, with and without motor dynamics,
 * auto_reset, observation_history_size 2, the actor as pds_collect asks for it.  0 for the Kalman hold, the ground effect, any
 * other noise setting and TakeOff with the latency ring or motor dynamics.  PDS_EINVAL for a NULL handle or actor. */
int pds_collect_control_supported(const pds_handle *h, const pds_mlp *pi, int mode);

/* pds_collect (include/pds.h: arguments, checks, alignment, ring arithmetic, tile statistics, asynchronous on `stream`, no
 * allocation beyond the handle's per-step sink row) that also flies the env configurations above.  On a configuration pds_collect
 * takes it is the same launch and the same bits.  On the others the env wave of a tile (csrc/pds_collect.h) carries the PID state
 * -- PDS_F_PID: rate and attitude integrals and last errors -- in registers over the K steps and the index of the delayed-action
 * ring (PDS_F_ACTION_IDX) in its counter word; the ring (PDS_F_ACTION_BUFFER) receives the exploration action a of step s, the
 * PWM comes from the row written lat_steps physics steps earlier; an env that finishes inside the launch gets its integrals
 * zeroed and its ring redrawn in place.  d_oa holds the action the policy chose.  Every output and, afterwards, every state field
 * is bitwise what the loop pds_mlp_forward + pds_ddpg_explore / pds_sac_sample + pds_step + the ring writes leaves.
 * PDS_EUNSUPPORTED where pds_collect_control_supported answers 0; a refused call leaves the handle and every buffer as they
 * were. */
int pds_collect_control(pds_handle *h, int K, int mode, const pds_mlp *pi, float act_limit, const float *d_log_std /* DDPG: [4]; SAC: NULL */,
                        uint64_t seed, uint64_t first_call, float *d_oa, float *d_obs2, float *d_rew, float *d_done, int64_t capacity,
                        int64_t ptr, float *d_obs, float *d_ep_ret, float *d_ep_len, float *d_tile_stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_COLLECT_CONTROL_H */
