/*
 * pds.h -- C ABI of libpds_hip.so, the MI355X (gfx950) batched CrazyFlie SimplePhysics stepper.
 *
 * Drop-in boundary for ONE hot path of SvenGronauer/phoenix-drone-simulation: the per-env
 * `env.reset()` / `env.step(action)` loop of DroneHoverSimpleEnv-v0, DroneCircleSimpleEnv-v0 and
 * DroneTakeOffSimpleEnv-v0, replaced by a lockstep step over N independent environments whose state
 * lives SoA in HBM.  Reference interfaces each entry point replaces (paths relative to
 * phoenix_drone_simulation/ in the reference):
 *
 *   pds_default_config / pds_create  <- gym.make(id, **kwargs) -> DroneBaseEnv.__init__
 *                                       (envs/base.py:26-153, envs/hover.py:7-63, envs/circle.py:7-77,
 *                                        envs/takeoff.py:13-70, ids in __init__.py:8-50)
 *   pds_reset                        <- DroneBaseEnv.reset (envs/base.py:382-431) incl.
 *                                       task_specific_reset (hover.py:192-243, circle.py:213-277,
 *                                       takeoff.py:179-212) and apply_domain_randomization
 *                                       (base.py:239-296)
 *   pds_reset_from_samples           <- same, with the np.random draws supplied by the caller
 *                                       (parity injection; the reference draws from the global
 *                                       numpy stream)
 *   pds_step                         <- DroneBaseEnv.step (envs/base.py:433-475) =
 *                                       SimplePhysics.step_forward (envs/physics.py:130-200) +
 *                                       CrazyFlieAgent.apply_action (envs/agents.py:259-298) +
 *                                       compute_history/reward/info/done + TimeLimit truncation
 *   pds_get_state / pds_set_state    <- direct attribute access env.drone.{xyz,rpy,xyz_dot,rpy_dot,x,
 *                                       last_action,...} used by simopt/ and debug/ callers
 *   pds_step_k                       <- the open-loop replay loop `for i in range(T-1): sim_env.step(acs[i])`
 *                                       of simopt (simopt/pybullet.py:163-176), K steps per launch
 *   pds_set_latency                  <- CrazyFlieAgent.set_latency (envs/agents.py:388-404)
 *   pds_simopt_evaluate              <- ObjectiveFunctionPyBullet.evaluate / evaluate_once / loss_function /
 *                                       set_parameters (simopt/pybullet.py:72-248), P candidates per launch
 *   pds_destroy                      <- env.close()
 *
 * All pointers named `d_*` are DEVICE pointers on the handle's device; tensors are row-major fp32.
 * Every entry point returns 0 on success or a negative PDS_E* code; pds_last_error() gives the text.
 * Launches are asynchronous on the caller's stream (`stream` is a hipStream_t passed as void*).
 * A handle is not thread-safe; different handles are independent; there is no global state.
 * There is NO CPU fallback: without a HIP device pds_create fails with PDS_ENODEVICE.
 */
#ifndef PDS_H
#define PDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_VERSION 2

#define PDS_TASK_HOVER 0   /* DroneHoverSimpleEnv-v0   */
#define PDS_TASK_CIRCLE 1  /* DroneCircleSimpleEnv-v0  */
#define PDS_TASK_TAKEOFF 2 /* DroneTakeOffSimpleEnv-v0 */

#define PDS_CTRL_PWM 0           /* envs/control.py:91-100  */
#define PDS_CTRL_ATTITUDE_RATE 1 /* envs/control.py:120-191 */
#define PDS_CTRL_ATTITUDE 2      /* envs/control.py:194-287 */

#define PDS_MAX_LATENCY_STEPS 8 /* rows of the delayed-action ring: int(latency / time_step) <= 8 */
#define PDS_MAX_REF_POINTS 300  /* Circle: circle_time * observation_frequency <= 300 (envs/circle.py:49) */

#define PDS_OK 0
#define PDS_EINVAL -1
#define PDS_ENODEVICE -2
#define PDS_EHIP -3
#define PDS_ENOMEM -4
#define PDS_EUNSUPPORTED -5

/* Mirror of the reference's env kwargs on this path (same names, same defaults). */
typedef struct pds_config {
  int32_t struct_size; /* = sizeof(pds_config), set by pds_default_config */
  int32_t task;
  int64_t num_envs;    /* N envs stepped in lockstep on this device */
  int64_t env_id_base; /* global id of local env 0 (multi-GPU sharding; keys the in-kernel RNG) */
  uint64_t seed;
  int32_t device;                    /* HIP device ordinal */
  int32_t use_motor_dynamics;        /* first-order motor model, envs/agents.py:284-288; default 0 */
  int32_t use_ground_effect;         /* envs/physics.py:27-58 formula as opt-in; default 0 */
  int32_t observation_noise;         /* >0: SensorNoise path; reference default 1 */
  int32_t aggregate_phy_steps;       /* default 1 for the *Simple envs */
  int32_t enable_reset_distribution; /* default 1 */
  int32_t max_episode_steps;         /* TimeLimit, default 500 */
  int32_t auto_reset;                /* 1: envs that terminate/truncate are reset inside pds_step */
  double domain_randomization;       /* default 0.10; <=0 disables */
  double motor_thrust_noise;         /* default 0.05; OU sigma = 0.2*value */
  double time_step;                  /* 1/sim_freq = 0.01 */
  double motor_time_constant;        /* 0.080 s */
  double penalty_action, penalty_angle, penalty_spin, penalty_terminal, penalty_velocity, ARP;
  double target_pos[3];
  double init_xyz[3], init_rpy[3], init_xyz_dot[3], init_rpy_dot[3];
  int32_t control_mode;              /* PDS_CTRL_*: 'PWM' (default), 'AttitudeRate', 'Attitude' (envs/control.py) */
  int32_t use_latency;               /* CrazyFlieAgent(use_latency=...), envs/agents.py:125,165; the Simple agent passes
                                        False (agents.py:492), simopt flips it through set_latency; default 0 */
  double latency;                    /* [s] envs/base.py:40 (0.015); buf_size = max(1, latency // time_step) */
  int32_t observation_frequency;     /* envs/base.py:42 (100): obs_rate = sim_freq // observation_frequency
                                        (base.py:108) and Circle num_ref_points = 3 * observation_frequency */
  int32_t reserved_;
} pds_config;

typedef struct pds_handle pds_handle;

/* State fields for pds_get_state / pds_set_state: [N, width] row-major, fp32 unless noted. */
enum pds_field {
  PDS_F_POS = 0,         /* 3  drone.xyz */
  PDS_F_RPY = 1,         /* 3  drone.rpy */
  PDS_F_VEL = 2,         /* 3  drone.xyz_dot */
  PDS_F_OMEGA = 3,       /* 3  drone.rpy_dot (body rates) */
  PDS_F_QUAT = 4,        /* 4  drone.quaternion (derived: sign * Q(rpy); read-only) */
  PDS_F_MOTOR_X = 5,     /* 4  drone.x */
  PDS_F_LAST_ACTION = 6, /* 4  u(k-1): drone.last_action == action_history[-1] */
  PDS_F_PREV_ACTION = 7, /* 4  u(k-2): action_history[-2] */
  PDS_F_STEP_COUNT = 8,  /* 1  int32: env.step calls since reset (iteration / aggregate_phy_steps) */
  PDS_F_QUAT_SIGN = 9,   /* 1  int32 0/1: quaternion == -Q(rpy) (only right after reset) */
  PDS_F_REF_OFFSET = 10, /* 1  int32: Circle ref_offset */
  PDS_F_PARAMS = 11,     /* 6  dt, m, Jxx, Jyy, Jzz, force_torque_factor_1 */
  PDS_F_MOTOR_A = 12,    /* 4  drone.A (B = 1 - A) */
  PDS_F_MOTOR_K = 13,    /* 4  drone.K */
  PDS_F_OU = 14,         /* 4  thrust_noise.state */
  PDS_F_GYRO_BIAS = 15,  /* 3  sensor_noise.gyro_bias */
  PDS_F_GYRO_LPF = 16,   /* 3  gyro_lpf._x */
  PDS_F_NOISY_OBS = 17,  /* 10 observation_history[-1][0:10]: noisy xyz, quaternion, velocity */
  PDS_F_PID = 18,        /* 12 rate integral3, rate last_error3, attitude integral3, attitude last_error3 */
  PDS_F_ACTION_BUFFER = 19, /* 32 drone.action_buffer, PDS_MAX_LATENCY_STEPS rows x 4 (rows >= buf_size: 0) */
  PDS_F_ACTION_IDX = 20,    /* 1  int32: drone.action_idx */
  PDS_F_COUNT_ = 21
};

/* Layout of one row of `d_samples` for pds_reset_from_samples (the values np.random returned in
 * the reference's draw order; see oracle/phoenix_oracle.h po_reset_sample). */
#define PDS_SAMPLE_FLOATS 112
#define PDS_S_POS_OFFSET 0 /* 3 */
#define PDS_S_RPY 3        /* 3 */
#define PDS_S_VEL 6        /* 3 */
#define PDS_S_OMEGA 9      /* 3 */
#define PDS_S_MOTOR_X 12   /* 4 */
#define PDS_S_ACTION 16    /* 4 */
#define PDS_S_DR_DT 20
#define PDS_S_DR_M 21
#define PDS_S_DR_J 22      /* 3 */
#define PDS_S_DR_FTF0 25
#define PDS_S_DR_FTF1 26
#define PDS_S_DR_T 27      /* 4 */
#define PDS_S_DR_T2W 31    /* 4 */
#define PDS_S_REF_OFFSET 35
/* standard variates of the two SensorNoise.add_noise calls inside reset() (envs/base.py:419,429);
 * each call: PDS_N_OBS_* layout below (24 floats).  Only read when observation_noise > 0. */
#define PDS_S_NOISE_CALL0 36
#define PDS_S_NOISE_CALL1 60
/* use_latency with buf_size B > 1: rows 0..B-2 of np.random.normal(HOVER_ACTION, 0.02, size=(B, 4))
 * (envs/hover.py:226-228) before clipping; row B-1 is PDS_S_ACTION (it becomes drone.last_action). */
#define PDS_S_ACTION_BUF 84 /* (PDS_MAX_LATENCY_STEPS - 1) x 4 */

/* Layout of one row of `d_variates` for pds_step_with_variates: the STANDARD variates (z ~ N(0,1),
 * u ~ U[0,1)) one env.step() consumes, in the reference's draw order restricted to the draws whose
 * value reaches the state or the observation:
 *   OUNoise.noise (envs/utils.py:106) | first add_noise call (envs/base.py:464, only its gyro part
 *   survives at obs_rate 1) | second add_noise call (envs/base.py:468 -> compute_history) | the rest of the
 *   first call.  With obs_rate > 1 a call at an iteration that is not a multiple of obs_rate only draws the
 *   gyro part (add_noise_to_omega, envs/sensors.py:121-134); the unused entries are ignored.
 * With aggregate_phy_steps = A > 1 (envs/base.py:457-465: A x {step_forward; compute_observation}) a row is
 * A consecutive blocks of PDS_NOISE_FLOATS: block `sub` holds PDS_N_OU and the PDS_N_A_* entries of physics
 * sub-step `sub`; the one observing call (PDS_N_OBS) is read from block 0. */
#define PDS_NOISE_FLOATS 52
#define PDS_N_OU 0        /* 4 z */
#define PDS_N_A_BIAS 4    /* 3 z  gyro bias random walk   (envs/sensors.py:130) */
#define PDS_N_A_RW 7      /* 3 z  gyro_random_walk term   (envs/sensors.py:133) */
#define PDS_N_A_TO 10     /* 3 z  turn-on-bias term       (envs/sensors.py:134) */
#define PDS_N_OBS 13      /* second call, 24 floats: */
#define PDS_N_OBS_POS_Z 0  /* 3 z */
#define PDS_N_OBS_POS_U 3  /* 3 u */
#define PDS_N_OBS_VEL_Z 6  /* 3 z */
#define PDS_N_OBS_BIAS 9   /* 3 z */
#define PDS_N_OBS_RW 12    /* 3 z */
#define PDS_N_OBS_TO 15    /* 3 z */
#define PDS_N_OBS_TH_Z 18  /* 3 z */
#define PDS_N_OBS_TH_U 21  /* 3 u */
/* position / velocity / angle draws of the FIRST call: they reach the observation only through the held
 * "Kalman" state when obs_rate = sim_freq // observation_frequency > 1 (envs/hover.py:134-156) */
#define PDS_N_A_POS_Z 37  /* 3 z */
#define PDS_N_A_POS_U 40  /* 3 u */
#define PDS_N_A_VEL_Z 43  /* 3 z */
#define PDS_N_A_TH_Z 46   /* 3 z */
#define PDS_N_A_TH_U 49   /* 3 u */

int pds_version(void);

/* Fill `cfg` with the reference ctor defaults of `task` (N = 1, device 0, auto_reset = 1). */
int pds_default_config(int task, pds_config *cfg);

/* Allocate the SoA state for cfg->num_envs envs on cfg->device.  State is undefined until the first
 * pds_reset*.  *out receives the handle. */
int pds_create(const pds_config *cfg, pds_handle **out);
int pds_destroy(pds_handle *h);

/* Observation width D = 2 * (|o| + 4): 42/40/48 noise-free, 34/40/48 with observation_noise. */
int pds_obs_dim(const pds_handle *h);
int64_t pds_num_envs(const pds_handle *h);

/* Reset the envs with d_mask[i] != 0 (d_mask == NULL: all) from the in-kernel Philox stream keyed by
 * (seed, env_id_base + i, reset tick); writes the reset observation [o0,u0,o0,u0] into d_obs rows of
 * the reset envs (d_obs: [N, D]). */
int pds_reset(pds_handle *h, const uint8_t *d_mask, float *d_obs, void *stream);

/* Same, with the sampled values supplied per env: d_samples [N, PDS_SAMPLE_FLOATS]. */
int pds_reset_from_samples(pds_handle *h, const uint8_t *d_mask, const float *d_samples,
                           float *d_obs, void *stream);

/* One lockstep env.step() for all N envs.
 *   d_actions   [N,4] in      d_obs        [N,D] out (reset obs for envs auto-reset in this step)
 *   d_reward    [N]   out     d_terminated [N] u8 out      d_truncated [N] u8 out
 *   d_cost      [N]   out (info['cost'])
 *   d_final_obs [N,D] or NULL: rows of envs that finished in this step receive their last obs. */
int pds_step(pds_handle *h, const float *d_actions, float *d_obs, float *d_reward,
             uint8_t *d_terminated, uint8_t *d_truncated, float *d_cost, float *d_final_obs,
             void *stream);

/* pds_step with the noise variates supplied by the caller (parity injection for the stochastic
 * parts: OU thrust noise, SensorNoise): d_variates [N, aggregate_phy_steps * PDS_NOISE_FLOATS].  The reference draws them
 * from the global numpy stream (envs/utils.py:106, envs/sensors.py:84-134). */
int pds_step_with_variates(pds_handle *h, const float *d_actions, const float *d_variates, float *d_obs,
                           float *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_cost,
                           float *d_final_obs, void *stream);

/* K lockstep env.step()s in ONE launch for open-loop action sequences (the replay of recorded actions
 * in simopt, simopt/pybullet.py:127-183: `for i in range(T-1): sim_env.step(acs[i])`): the env state
 * stays in registers between the K steps, only actions (in) and observations / rewards / flags (out)
 * stream through HBM.  Bitwise identical to K pds_step calls.  (Two launches on `stream` for the observation-noise
 * configurations: the kept noisy observation, which pds_step regenerates instead of storing, is materialised first.)
 *   d_actions [K,N,4]   d_obs [K,N,D]   d_reward, d_cost [K,N]   d_terminated, d_truncated [K,N] u8
 *   d_final_obs [K,N,D] or NULL */
int pds_step_k(pds_handle *h, int k_steps, const float *d_actions, float *d_obs, float *d_reward,
               uint8_t *d_terminated, uint8_t *d_truncated, float *d_cost, float *d_final_obs, void *stream);
/* 1 when pds_step_k is ONE launch for this handle, 0 when it loops over pds_step (same bits, K launches, the state through
 * HBM every step).  One launch: control_mode PWM in every configuration, and the PID modes (AttitudeRate / Attitude, the PID
 * integrals and previous errors in registers with the rest of the state) with and without the latency ring.  The loop: a PID
 * mode together with the ground effect or with the Kalman hold (observation_frequency below the simulation frequency).
 * pds_bytes_per_env_step_k prices the handle accordingly. */
int pds_step_k_fused(const pds_handle *h);

/* CrazyFlieAgent.set_latency (envs/agents.py:388-404; called by simopt/pybullet.py:248): latency <
 * time_step disables the delay, otherwise buf_size = int(latency / time_step) and the action buffer and
 * its index are zeroed for every env.  Synchronises the device (not a hot path). */
int pds_set_latency(pds_handle *h, double latency);
int pds_latency_steps(const pds_handle *h); /* current buf_size, 0 when use_latency is off */

/* ---- sim-opt objective (csrc/pds_simopt.hip) -------------------------------------------------------
 * ObjectiveFunctionPyBullet.evaluate (simopt/pybullet.py:72-248) for P parameter candidates x M logged mini-trajectories of
 * length T in ONE launch, on the SimplePhysics path with the PT1 motor model on (the recipe switches it on whatever the env was
 * made with).  For every pair (p, m): set_parameters(params[p]) -- values clipped at 0, T clipped to >= time_step,
 * A = 1 - T_s / T, K = 0.028 G t2w / 4 in float64 --, reset (motor state and delayed-action ring zero), pre_steps steps of
 * pre_inputs[m], keep the motor state, reset to the logged state (ring zeroed again), T - 1 steps of actions[m] with
 *   loss[p, m] = mean_i gamma^i (||e_i||_1 + ||e_i||_2),
 *   e_i = [euler(quat) - rpy, 100 (xyz - xyz_real), 10 (v - v_real), omega - omega_real]  against logged row i + 1;
 * score[p] = mean_m loss[p, m], summed in a fixed order: a candidate's score does not depend on the rest of the batch.  No
 * termination, no TimeLimit, no auto-reset.  This is the DETERMINISTIC objective: a handle with thrust or observation noise,
 * domain randomisation, ground effect or a PID control mode is refused with PDS_EUNSUPPORTED.
 *
 * `h` supplies the configuration only (model constants, time_step, aggregate_phy_steps): no state, tick or latency of the
 * handle is read or changed (only its error text, on failure); num_envs is irrelevant.  Asynchronous on `stream`, no
 * allocation, no synchronisation, capturable into a hipGraph.
 *   d_params     [P,3]  thrust_to_weight_ratio, motor_time_constant [s], latency [s] (the latency is used through d_lat_steps)
 *   d_lat_steps  [P]    int32 buf_size of every candidate = pds_simopt_latency_steps (the reference's float64
 *                       int(latency / time_step), 0 below one time step); max_lat_steps = their maximum, by value: above
 *                       PDS_MAX_LATENCY_STEPS the whole call is refused before anything is launched
 *   d_actions    [T][M][4]      time-major, 16-byte aligned (row T-1 is not read)
 *   d_obs        [T][3][M][4]   time-major quads (x y z vx | vy vz roll pitch | yaw wx wy wz): row 0 = the state the sample
 *                               starts from (the reset's pose read-back of the logged row, body rates R^T R^T (R w)), rows
 *                               1..T-1 = the logged rows
 *   d_pre_inputs [pre_steps][M][4]
 *   d_loss [P,M] out    d_score [P] out    d_sim_obs [T-1,P,M,13] out or NULL: xyz, quaternion, velocity, body rates after
 *   every step (bitwise the first 13 observation columns of pds_step_k replaying the same actions). */
int pds_simopt_latency_steps(const pds_handle *h, double latency);
int pds_simopt_evaluate(pds_handle *h, int64_t P, const float *d_params, const int32_t *d_lat_steps, int max_lat_steps,
                        int64_t M, int T, int pre_steps, double gamma, const float *d_actions, const float *d_obs,
                        const float *d_pre_inputs, float *d_loss, float *d_score, float *d_sim_obs, void *stream);

int pds_field_width(int field);
int pds_get_state(pds_handle *h, int field, void *d_out, void *stream);
/* Edits ONE field of every env.  What an env has observed is not edited with it: with observation noise the history half of
 * the next observation row stays the (noisy) observation the previous step returned -- the kernels regenerate it from the
 * state and the previous tick's draws, so pds_set_state (like a masked pds_reset and pds_set_tick) first writes it to memory,
 * one extra launch on `stream`; pds_set_state(PDS_F_NOISY_OBS) replaces it.  Without observation noise o(k) is rebuilt from
 * the state the step loads, i.e. it follows an edit of PDS_F_POS / PDS_F_RPY / PDS_F_VEL / PDS_F_OMEGA. */
int pds_set_state(pds_handle *h, int field, const void *d_in, void *stream);

/* Number of reset/step ticks issued so far (the Philox counter word). */
/* Diagnostic (synchronises the stream): number of envs whose position / attitude / velocity / body
 * rates hold a NaN or an Inf.  The reference has no such guard; its explicit Euler
 * step can overflow on envs that never terminate (TakeOff with domain randomisation). */
int pds_count_nonfinite(pds_handle *h, int64_t *count, void *stream);

/* The tick and the parity of the action ring live in DEVICE memory (one word per 64-env tile, advanced
 * by the kernels themselves), so no kernel argument changes between two pds_step calls with the same
 * pointers: a sequence of pds_step / pds_reset calls can be captured into a hipGraph and replayed.
 * pds_tick returns the host's mirror (exact unless a captured graph was replayed);
 * pds_sync_tick(h, stream) synchronises `stream`, re-reads the device word and returns it.
 *
 * The tick also sets the phase of the lean configurations' state store (control_mode PWM without motor dynamics, domain
 * randomisation, thrust / observation noise and latency; with or without the ground effect): a pds_step launched at an EVEN
 * tick is a write step, one launched at an ODD tick a skip step, which leaves position / attitude / velocity / body rates
 * in memory one step behind and says so in the env's counter word; the next pds_step recomputes them from the stored state
 * and the action ring, bit for bit.  No caller sees it: every entry point that reads or edits the state brings it up to
 * date first (one extra launch on its stream when a step has run since), and what a step returns does not depend on the
 * phase.  Handles whose launch is at most one round of resident blocks (3 blocks of 256 envs per compute unit) store every
 * step: such a launch is bound by a wave's latency, not by memory.  PDS_STATE_EVERY_STEP=1 / =0 in the environment of
 * pds_create forces either form (tests, A/B runs); a library built with -DPDS_STATE_EVERY_OTHER_STEP=0 stores every step. */
uint64_t pds_tick(const pds_handle *h);
uint64_t pds_sync_tick(pds_handle *h, void *stream);
/* Restore the tick of a checkpoint: a handle created with the same config whose fields were all set
 * with pds_set_state and whose tick was set to the saved one continues the saved run bit for bit
 * (there is no other hidden state: the reference offers no checkpointing of its envs; its trainer
 * checkpoints are model.pt / state.pkl, utils/loggers.py:382-407). */
int pds_set_tick(pds_handle *h, uint64_t tick);

/* Algorithmic HBM bytes one pds_step moves per env for this configuration. */
int pds_bytes_per_env_step(const pds_handle *h);
/* the same for pds_step_k with k_steps per launch (state traffic amortised over the K steps where pds_step_k_fused is 1;
 * pds_bytes_per_env_step where it loops) */
int pds_bytes_per_env_step_k(const pds_handle *h, int k_steps);

const char *pds_last_error(const pds_handle *h);

/* The generator of the RNG contract, exposed for verification: d_out[i] =
 * Philox4x32-<rounds>(counter d_ctr[i][0..3], key d_key[i][0..1]) for i < n, computed by the same device
 * function the step / reset kernels use (rounds 10: reset sampling, 7: per-step noise).  tests/ check it
 * against the Random123 known-answer vectors.  Runs on the current device. */
int pds_philox4x32(const uint32_t *d_ctr, const uint32_t *d_key, int rounds, int64_t n, uint32_t *d_out, void *stream);

/* The standard normals of the per-step noise, exposed for verification: d_out[i][0..7] = the four
 * one-word Box-Muller pairs of Philox4x32-7(counter (env_id_base + i, tick lo, tick hi, block), key = seed) for i < n --
 * the device functions the step kernels draw the OU / gyro / sensor normals with (envs/sensors.py:75-134, envs/base.py:457-468).
 * tests/ hold 2^26 of them against N(0, 1): Kolmogorov-Smirnov distance, moments, tail mass.  Runs on the current device. */
int pds_noise_normals(uint64_t seed, uint64_t tick, uint32_t block, uint64_t env_id_base, int64_t n, float *d_out, void *stream);

/* The two-word Box-Muller of the Gaussian policy sampler and the ES noise, exposed for verification:
 * d_out[i][0..1] = (r cos 2 pi u2, r sin 2 pi u2), r = sqrt(-2 ln u1), u1 = ((a >> 8) + 1) 2^-24, u2 = (b >> 8) 2^-24 for the
 * word pair (a, b) = d_words[i][0..1], i < n -- computed by the device function pds_gaussian_sample, the fused rollouts and
 * pds_es_* draw their normals with.  tests/ sweep all 2^24 radii and all 2^24 angles against float64.  PDS_EINVAL: a NULL
 * pointer, n < 1.  Runs on the current device. */
int pds_box_muller(const uint32_t *d_words, int64_t n, float *d_out, void *stream);

/* observation_history_size = H other than 2 (envs/base.py:44, 303-319, 417-431): advances the [N, H, half]
 * history of every env by the step's new row `d_obs2` [N, 2 * half] (the pds_step output) in one launch.
 * Running envs: hist' = [hist[1:], newest half].  Finished envs (auto_reset != 0): their final history
 * [hist[1:], newest half of d_final_obs2] goes to d_final_hist (rows of other envs untouched; may be NULL) and
 * hist' = [H - 1 copies of the reset row's first half, its second half].  d_hist_out must not alias d_hist_in. */
int pds_history_advance(int64_t n, int half, int history, const float *d_obs2, const uint8_t *d_terminated,
                        const uint8_t *d_truncated, const float *d_final_obs2, int auto_reset, const float *d_hist_in,
                        float *d_hist_out, float *d_final_hist, void *stream);

/* ---- caller-side helper: GAE over a lockstep rollout ----------------------
 * Replaces core.Buffer.finish_path / calculate_adv_and_value_targets (algs/core.py:461-533, one
 * scipy lfilter per finished path) for a [T, N] rollout: d_rew, d_val [T,N] f32; d_terminated,
 * d_truncated [T,N] u8 (the flags pds_step returned); d_final_val [T,N] = V(final_obs) read where
 * truncated -- the cut wins over a termination on the same step, algs/iwpg/iwpg.py:374-379 -- (may be NULL); d_last_val [N] = V(o_T).  rew_scale = 1/(ret_std + eps) with clipping to
 * +-rew_clip (use_reward_scaling) or 0 for raw rewards.  Outputs [T,N]: advantages, value targets,
 * discounted returns.  Runs on the current device, asynchronously on `stream`. */
int pds_gae(const float *d_rew, const float *d_val, const uint8_t *d_terminated, const uint8_t *d_truncated,
            const float *d_final_val, const float *d_last_val, float gamma, float lam, float rew_scale,
            float rew_clip, int64_t T, int64_t N, float *d_adv, float *d_target_v, float *d_disc_ret,
            void *stream);

/* ---- caller-side dense kernels on the f32 matrix cores ----------------------
 * A 3-layer MLP in torch's nn.Linear layout (weights [out][in] row-major, device pointers):
 * y = W3 act(W2 act(W1 x + b1) + b2) + b3; d_in <= 192 (more than 64 inputs -- observation_history_size >= 4,
 * envs/base.py:303-319 -- run the K-tiled kernels of csrc/pds_mlp_wide.hip), h1, h2 <= 64, d_out <= 8; activation 0 relu, 1 tanh.
 * Mirrors build_mlp_network / MLPGaussianActor.net / MLPCritic.net (algs/core.py:65-103, 228-311). */
typedef struct pds_mlp {
  int32_t d_in, h1, h2, d_out, activation;
  const float *w1, *b1, *w2, *b2, *w3, *b3;
} pds_mlp;

/* ONE launch per rollout (csrc/pds_rollout.h): the T closed-loop steps of the caller's roll_out
 * (algs/iwpg/iwpg.py:350-385; ActorCritic.step algs/core.py:370-393) --
 *   V(o) -> d_val_buf[t];  a = mu(o) + exp(log_std) z, log p -> d_act_buf[t], d_logp_buf[t] (the draws of
 *   pds_gaussian_sample with call = *d_call_base + call_offset + t + 1);  env.step(a) (bitwise pds_step) ->
 *   d_rew_buf[t], d_term_buf[t], d_trunc_buf[t], d_cost_buf[t], next observation -> d_obs_buf[t + 1];
 *   V(final observation) of the envs whose episode the TimeLimit cut at step t (truncated, terminated or not: the
 *   bootstrap value of algs/iwpg/iwpg.py:374-379; at t = T - 1 also of the envs that only terminated, for a caller that
 *   mirrors the reference's epoch-end cut) -> d_fval_buf[t] (other entries are left alone: pds_gae never reads them);  episode return / length bookkeeping of pds_rollout_record -> d_ep_ret, d_ep_len, d_stats[3]
 * -- and V(o(T)) -> d_last_val.  d_obs_buf is [T + 1, N, D]: row 0 holds o(0) on entry, rows 1..T are written.
 * Networks: actor d_in = D, d_out = 4; critic d_in = D, d_out = 1; hidden <= 64; inputs standardised with
 * d_mean / d_std / eps when given (OnlineMeanStd.forward).  All other buffers are [T, N] ([T, N, 4] actions).
 * PDS_EUNSUPPORTED for env configurations the kernel is not built for (the caller falls back to the per-step
 * entry points, which give the same bits). */
int pds_rollout(pds_handle *h, int T, const pds_mlp *pi, const pds_mlp *vf, const float *d_mean, const float *d_std, float eps,
                const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset, int deterministic,
                float *d_obs_buf, float *d_act_buf, float *d_logp_buf, float *d_val_buf, float *d_rew_buf,
                uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fval_buf, float *d_last_val,
                float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream);

/* The same for observation histories other than 2 (observation_history_size = H, envs/base.py:44, 303-319, 417-431;
 * csrc/pds_rollout_hist.h): the actor reads the last `history` [o, u] halves of every env, history x half <= 192 inputs.
 * In the kernel: actor, sampling, env.step (bitwise pds_step), the history update of pds_history_advance, the episode
 * bookkeeping.  NOT in the kernel: the critic -- the caller evaluates V over d_obs_buf afterwards (pds_mlp_forward), and
 * over d_fin_rows: the final histories of the envs whose path bootstraps with V (the TimeLimit cut it, or it finished on
 * step T - 1: algs/iwpg/iwpg.py:374-379), one slot list per env -- d_fin_rows [slots, N, history x half], d_fin_step
 * [slots, N] = the step t whose d_fval_buf[t] entry the row's value is; the caller presets d_fin_step to -1 (unused);
 * slots >= T / max_episode_steps + 2.  d_obs_buf [T + 1, N, history x half]: row 0 = the histories on entry, rows 1..T
 * written.  Other buffers as pds_rollout.  Built for every control mode (PWM, AttitudeRate, Attitude; TakeOff fixes PWM) with
 * noise off or at the reference's default (domain randomisation + thrust noise + observation noise), with and without motor
 * dynamics (TakeOff: without).  PDS_EUNSUPPORTED, before the handle is touched, for the rest -- the latency ring, the Kalman hold,
 * the ground effect, partial noise settings -- (the per-step path gives the same bits). */
int pds_rollout_history(pds_handle *h, int T, int history, const pds_mlp *pi, const float *d_mean, const float *d_std, float eps,
                        const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset,
                        int deterministic, float *d_obs_buf, float *d_act_buf, float *d_logp_buf, float *d_rew_buf,
                        uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows, int32_t *d_fin_step,
                        int slots, float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream);

/* ONE launch evaluates a POPULATION of policies (csrc/pds_evaluate.h): the evaluation loop of the reference
 * (EnvironmentEvaluator.eval / eval_once, utils/evaluation.py:52-107: reset, act deterministically until terminated or truncated,
 * sum reward and info['cost']; ActorCritic.step in eval mode, algs/core.py:370-393) for P policies x E = episodes_per_policy
 * episodes.  The handle's N = P x E envs are P contiguous blocks of E envs (E a multiple of 64); block p flies policy p with
 * action = actor mean.  Every env plays ONE episode from the observation it holds on entry (d_obs0 [N, D]: what pds_reset
 * returned): return, length and cost accumulate in registers, freeze at the env's first terminated | truncated (the env itself
 * is reset in place and flies on, as under a per-step loop) and go to d_ret, d_len, d_cost [N] -- the only outputs; episodes
 * still running after max_steps steps are cut there.  Bitwise what max_steps x (pds_mlp_forward per policy + pds_step) and the
 * same sums in the same order give.
 *   shape     d_in = D, h1, h2 <= 64, d_out = 4, activation of EVERY policy; its pointers are ignored
 *   d_params  [P, pds_mlp_param_count(shape)]: row p = W1 b1 W2 b2 W3 b3 of policy p, torch order
 *   d_mean, d_std [P, D] (both or none), eps: (o - mean[p]) / (std[p] + eps) in front of policy p (OnlineMeanStd.forward)
 * PDS_EINVAL: a NULL pointer, P x episodes_per_policy != num_envs, episodes_per_policy not a multiple of 64, a wrong network
 * shape, max_steps < 1, a handle that was never reset.  PDS_EUNSUPPORTED: a handle without auto_reset, or an env
 * configuration pds_rollout is not built for (pds_evaluate_supported says so beforehand: 1 / 0).  A refused call leaves the
 * handle as it was.  After a successful call the tick and every tile's device clock are max_steps further -- also for a tile
 * that stopped early: a tile stops once none of its 64 envs is in its first episode -- and the handle is back in the "not
 * reset" state: tiles stopped at different steps, so pds_step, pds_rollout and the rest answer PDS_EINVAL "before pds_reset"
 * until pds_reset has run for EVERY env: a pds_reset with a mask is refused (PDS_EINVAL) until then, and an edit of a state
 * field (pds_set_state) does not lift the state either.  The parity of the state ring (which slot holds the last action) is
 * the same in every tile afterwards, as after max_steps steps.  Asynchronous on `stream`; the first call on a handle allocates 16 N bytes that the steps' per-step
 * outputs stream into. */
int pds_evaluate_supported(const pds_handle *h);
int pds_evaluate_policies(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape, const float *d_params,
                          const float *d_mean, const float *d_std, float eps, int max_steps, const float *d_obs0, float *d_ret,
                          float *d_len, float *d_cost, void *stream);

/* The same launch, also reporting flight-quality metrics (csrc/pds_evaluate.h, the flight metrics): what the reference tabulates per real
 * flight (experiments/02_zero_shot_policy_transfer_hover_task/02_eval_hover_task.py: mean squared roll and pitch, the oscillation
 * of the rates and of the motor commands, the flight time) as raw sums over the states x(0) .. x(L - 1) the first episode's
 * policy acted in -- x(0) the state pds_reset left, x(s) the TRUE state before step s (not the noisy observation), L the episode
 * length; the sums freeze with d_len.  The state after the last step is not counted: the same step resets it away.
 * a(s): the actor's raw output of step s; u: PDS_F_LAST_ACTION before the step (after a reset, the reset's own action).
 * Every product and every sum is rounded on its own, steps in order: bitwise what separate elementwise float32 operations give. */
#define PDS_EVAL_METRICS 8
enum {
  PDS_EM_ROLL_SQ = 0,              /* += roll * roll */
  PDS_EM_PITCH_SQ = 1,             /* += pitch * pitch */
  PDS_EM_RATE_SQ = 2,              /* += (wx * wx + wy * wy) + wz * wz */
  PDS_EM_ACTION_RATE_SQ = 3,       /* d = a(s) - u; += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3 */
  PDS_EM_TILT_MAX = 4,             /* max over the steps of |roll| and |pitch|, from 0; m = (v > m) ? v : m, so a NaN is passed over */
  PDS_EM_SATURATED_STEPS = 5,      /* += 1 when any |a_j(s)| > 1: the steps whose action control_mode PWM clips */
  PDS_EM_ROLL_RATE_CROSSINGS = 6,  /* += 1 for s >= 1 when (wx(s - 1) < 0) != (wx(s) < 0) */
  PDS_EM_PITCH_RATE_CROSSINGS = 7  /* the same for wy */
};
/* pds_evaluate_policies with one more output: d_metrics [N, PDS_EVAL_METRICS], 16-byte aligned, row n = the PDS_EM_* values of
 * env n.  Checks, support (pds_evaluate_supported), d_ret / d_len / d_cost (the same bits) and the state of the handle afterwards
 * are pds_evaluate_policies'; in addition PDS_EINVAL for a NULL or misaligned d_metrics. */
int pds_evaluate_policies_metrics(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                  const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                  const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics, void *stream);

/* pds_evaluate_policies_metrics with one more output: the sums a running observation standardisation is updated from
 * (csrc/pds_evaluate.h, the observation sums), over every observation o(s) a first-episode policy acted on -- o(s) of env n for s < d_len[n], so
 * their count per policy is the sum of its d_len.  Per feature k < D
 *     d = o_k - d_mean[p][k]   (d = o_k when d_mean is NULL),   S1 += d,   S2 += d * d,
 * every difference, product and sum rounded on its own in float32; the shift by the policy's own mean keeps S2 well conditioned.
 * d_obs_sums [tiles, 4, 2, 64] float32, 16-byte aligned, tiles = N / 64 (tile t = envs 64 t .. 64 t + 63, of policy
 * t / (episodes_per_policy / 64)): [t][w][0][k] = S1 and [t][w][1][k] = S2 of feature k over the envs 64 t + 16 w .. 64 t + 16 w + 15,
 * zero for k >= D.  Per env the steps are added in order; the 16 envs of a part are then added as a fixed tree: env j + env j + 8,
 * then j + (j + 4), then + 2, then + 1.  The four parts of a tile and the tiles of a policy are left to the caller (sum them in
 * float64).  Every element is written.  Checks, support (pds_evaluate_supported), d_ret / d_len / d_cost / d_metrics (the same
 * bits) and the state of the handle afterwards are pds_evaluate_policies_metrics'; in addition PDS_EINVAL for a NULL or
 * misaligned d_obs_sums. */
int pds_evaluate_policies_stats(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                float *d_obs_sums, void *stream);

/* pds_evaluate_policies_metrics (d_metrics may be NULL here) that also RECORDS the flights it scores (csrc/pds_evaluate.h, the
 * record): of every policy's episodes_per_policy envs the first record_per_policy -- a positive multiple of 64, at most
 * episodes_per_policy -- are recorded, N_rec = P * record_per_policy columns, column j = p * record_per_policy + e for env e of
 * policy p.
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

/* The population evaluation for policies that read an observation HISTORY (csrc/pds_evaluate_hist.h; observation_history_size =
 * `history`, envs/base.py:44, 303-319, 417-431): the actors read the last `history` halves [o, u] of their env, history * half
 * inputs with half = pds_obs_dim / 2.  d_obs0 [N, history * half]: the histories on entry -- after pds_reset, history - 1 copies
 * of the first half of the row it returned, then its second half.  Behind every step a history is shifted by one half and the
 * second half of the step's row appended; the history of an env that finished restarts from its reset row in the same way (what
 * pds_history_advance does under a per-step loop).  shape->d_in = history * half; d_mean, d_std [P, history * half].
 * d_metrics [N, PDS_EVAL_METRICS], 16-byte aligned, or NULL: the PDS_EM_* values, from the same launch.
 * Bitwise what max_steps x (pds_mlp_forward per policy + pds_step + pds_history_advance) and the same sums in the same order give.
 * Checks and the state of the handle afterwards are pds_evaluate_policies'.  PDS_EUNSUPPORTED: a handle without auto_reset, an env
 * configuration pds_rollout_history is not built for, or history * half > 192 (pds_evaluate_history_supported says so beforehand:
 * 1 / 0).  history = 2 is accepted: the same bits as pds_evaluate_policies and pds_evaluate_policies_metrics. */
int pds_evaluate_history_supported(const pds_handle *h, int history);
int pds_evaluate_policies_history(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                  const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                  const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics, void *stream);

/* (pds_evaluate_policies_history_record, the same launch with the flights recorded, is declared in include/pds_history_record.h) */

/* number of parameters; flat gradient layout = [W1, b1, W2, b2, W3, b3] (torch parameter order) */
int pds_mlp_param_count(const pds_mlp *m);
/* floats of scratch the *_grad entry points need (per-wave partial sums) */
int64_t pds_mlp_workspace_floats(const pds_mlp *m);

/* d_y[B, d_out] = MLP(x'), x' = row d_index[g] (or g when d_index is NULL) of d_x[rows, d_in],
 * standardised as (x - mean) / (std + eps) when d_mean / d_std are given (OnlineMeanStd.forward,
 * utils/online_mean_std.py:32-43).  Replaces ActorCritic.step's network calls (algs/core.py:370-393). */
int pds_mlp_forward(const pds_mlp *m, const float *d_x, const int64_t *d_index, int64_t B, const float *d_mean,
                    const float *d_std, float eps, float *d_y, void *stream);

/* Gradient of the PPO-clip policy loss  -mean(min(r A, clip(r, 1-c, 1+c) A)),  r = exp(logp - logp_old),
 * logp = Normal(MLP(x), exp(log_std)).log_prob(act).sum(-1)  (compute_loss_pi, algs/ppo/ppo.py:22-40)
 * with respect to the MLP parameters: d_grads[param_count]; d_stats[4] = {sum of -min(..), sum of r,
 * sum over samples and actions of 0.5 z^2 (approx_kl numerator), sample count}.  d_x is the
 * already standardised observation batch [B, d_in]. */
int pds_ppo_policy_grad(const pds_mlp *m, const float *d_x, const float *d_act, const float *d_adv,
                        const float *d_logp_old, const float *d_log_std, int64_t B, float clip_ratio, float *d_grads,
                        float *d_stats, float *d_workspace, void *stream);

/* Gradient of mse_loss(MLP(x[index]), target[index]) (compute_loss_v, algs/iwpg/iwpg.py:272-275) for a
 * critic (d_out == 1); d_index selects the mini-batch rows (NULL: rows 0..B-1); d_stats[0] = sum of
 * squared errors, d_stats[3] = sample count. */
int pds_value_grad(const pds_mlp *m, const float *d_x, const int64_t *d_index, const float *d_target, int64_t B,
                   float *d_grads, float *d_stats, float *d_workspace, void *stream);

/* a[n, d_out] = mu + exp(log_std) z with z ~ N(0, 1) (Philox4x32-10, key = seed, counter = (global
 * sample id = id_base + row, call)), logp[n] = Normal(mu, sigma).log_prob(a).sum(-1); deterministic != 0
 * gives a = mu (evaluation mode).  dist.sample() + log_prob of ActorCritic.step, algs/core.py:370-393. */
int pds_gaussian_sample(const float *d_mu, const float *d_log_std, int64_t n, int d_out, uint64_t seed, uint64_t call,
                        uint64_t id_base, int deterministic, float *d_act, float *d_logp, void *stream);

/* The same with the call counter split into a DEVICE word and a by-value offset: call = *d_call_base + call_offset.
 * A rollout captured into a hipGraph passes the step index as the offset and advances the device word once
 * per replay with pds_counter_add (*d_counter += inc, one thread), so every replay draws fresh variates.
 * The counter packing holds sample ids below 2^56: PDS_EINVAL (both entry points) when id_base + n > 2^56. */
int pds_gaussian_sample_dev(const float *d_mu, const float *d_log_std, int64_t n, int d_out, uint64_t seed,
                            const uint64_t *d_call_base, uint64_t call_offset, uint64_t id_base, int deterministic,
                            float *d_act, float *d_logp, void *stream);
int pds_counter_add(uint64_t *d_counter, uint64_t inc, void *stream);

/* d_out[i] = p(i), i < n: a pseudo-random permutation of 0 .. n-1 keyed by (seed, call) -- a 6-round Feistel network
 * (round keys from Philox4x32-10) over the next even-width power of two, cycle-walked into [0, n).  One elementwise
 * launch; stands in for the index shuffle of the value net's mini-batches (np.random.shuffle in
 * IWPGAlgorithm.update_value_net, algs/iwpg/iwpg.py:487-522), whose stream the GPU trainer does not share anyway. */
int pds_permutation(int64_t *d_out, int64_t n, uint64_t seed, uint64_t call, void *stream);

/* One rollout step's bookkeeping (buf.store + episode statistics of IWPGAlgorithm.roll_out,
 * algs/iwpg/iwpg.py:350-385): copies reward / terminated / truncated [n] into their [T, N] slices, adds
 * the reward to the running episode return and 1 to the length, and for finished envs adds
 * (return, length, 1) to d_stats[0..2] and zeroes their running values. */
int pds_rollout_record(const float *d_rew, const uint8_t *d_term, const uint8_t *d_trunc, int64_t n, float *d_rew_buf,
                       uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_ep_ret, float *d_ep_len, float *d_stats,
                       void *stream);

/* torch.optim.Adam.step (no weight decay / amsgrad) for the six tensors of `m` from their flat gradient;
 * d_exp_avg / d_exp_avg_sq [param_count] are the optimiser state, step counts from 1. */
int pds_adam_step(const pds_mlp *m, const float *d_grads, float *d_exp_avg, float *d_exp_avg_sq, int64_t step, float lr,
                  float beta1, float beta2, float eps, void *stream);

/* Gradient + optimiser step in the SAME two launches as the gradient alone: the partial-sum kernel of
 * pds_ppo_policy_grad / pds_value_grad applies torch.optim.Adam.step to each parameter right after it has summed its
 * gradient (same arithmetic as pds_adam_step: the two routes give the same bits; d_grads and d_stats are written as
 * before).  opt == NULL: no step (= the plain entry points).  For single-process training without gradient clipping --
 * with several ranks the gradient all-reduce sits between the two. */
typedef struct pds_adam {
  float *d_exp_avg, *d_exp_avg_sq; /* optimiser state [param_count] */
  int64_t step;                    /* counts from 1 */
  float lr, beta1, beta2, eps;
} pds_adam;
int pds_ppo_policy_grad_step(const pds_mlp *m, const float *d_x, const float *d_act, const float *d_adv,
                             const float *d_logp_old, const float *d_log_std, int64_t B, float clip_ratio, float *d_grads,
                             float *d_stats, float *d_workspace, const pds_adam *opt, void *stream);
int pds_value_grad_step(const pds_mlp *m, const float *d_x, const int64_t *d_index, const float *d_target, int64_t B,
                        float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream);

/* The natural-gradient policy step of NPG / TRPO (algs/npg/npg.py:52-160, algs/trpo/trpo.py:16-66; csrc/pds_npg.hip).
 * Scratch floats the three entry points below need (per-wave partial sums), for up to num_candidates line-search
 * candidates. */
int64_t pds_npg_workspace_floats(const pds_mlp *m, int num_candidates);

/* Fisher-vector product of the Gaussian policy with a fixed log_std: d_out = F v + damping v,
 * F v = 1 / (B d_out) sum_i J_i^T diag(exp(-2 log_std)) J_i v with J_i = d MLP(x_i) / d theta -- the double backward of
 * kl_divergence(p_old, p_theta).mean() at theta_old (NaturalPolicyGradientAlgorithm.Fvp, algs/npg/npg.py:52-77).
 * x_i = row d_index[i] (or i when d_index is NULL) of the standardised rows d_x; d_v and d_out [param_count] in the flat
 * layout of pds_mlp_param_count (d_out may alias d_v); d_workspace: pds_npg_workspace_floats(m, 0) floats.  Summed in a
 * fixed order: the same inputs give the same bits. */
int pds_npg_fisher_vector_product(const pds_mlp *m, const float *d_x, const int64_t *d_index, int64_t B, const float *d_log_std,
                                  const float *d_v, float damping, float *d_out, float *d_workspace, void *stream);

/* One iteration of conjugate_gradients (algs/utils.py:5-38) on n floats, one workgroup, no host sync.  d_state[2] =
 * {r.r, stopped}.  init != 0: x = 0, r = p = d_z (= b; Avp(0) is 0), d_state = {b.b, 0}.  Otherwise d_z = Avp(p) and,
 * unless stopped: alpha = r.r / (p.z + eps), x += alpha p, r -= alpha z; when sqrt(r.r) < residual_tol the iteration
 * stops (the reference's break: x and r updated, then x, r, p frozen); else p = r + (r.r_new / (r.r + eps)) p. */
int pds_npg_cg_step(int64_t n, float *d_x, float *d_r, float *d_p, const float *d_z, float *d_state, float eps,
                    float residual_tol, int init, void *stream);

/* The line-search candidates of TRPO (algs/trpo/trpo.py:16-66) in one launch: candidate j has the parameters
 * theta_old + f_j s (theta_old = the network `m`, s = d_step [param_count], f_j = d_fracs[j]; product and sum rounded
 * separately, as torch's `theta + f * s`).  d_out[4 j .. 4 j + 3] = {sum over samples of ratio adv, sum over samples x
 * actions of KL(Normal(mu_old, sigma) || Normal(mu_j, sigma)), 1 if either sum is not finite else 0, sum of ratio}, ratio =
 * exp(logp_j(act) - logp_old), sigma = exp(log_std); d_x [B, d_in] standardised, d_act / d_mu_old [B, d_out], d_adv /
 * d_logp_old [B].  d_theta_out (optional, [num_candidates, param_count]): the candidates' parameters.  d_workspace:
 * pds_npg_workspace_floats(m, num_candidates) floats.  Summed in a fixed order. */
int pds_npg_surrogate_kl(const pds_mlp *m, const float *d_step, const float *d_fracs, int num_candidates, const float *d_x,
                         const float *d_act, const float *d_adv, const float *d_logp_old, const float *d_mu_old,
                         const float *d_log_std, int64_t B, float *d_out, float *d_theta_out, float *d_workspace, void *stream);

/* An evolution strategy over the flat parameters of one actor (es.py ESTrainer; csrc/pds_es.hip).  No
 * handle: like pds_gaussian_sample the entry points run on the current device, asynchronously on `stream`.
 * Noise contract: a population of 2 * pairs policies is `pairs` antithetic pairs; with Q = ceil(n / 8), element j = 8 q + r of
 * the noise vector eps_i of GLOBAL pair i = pair_base + row is variate r (of d_out = 8) that pds_gaussian_sample draws for
 * sample id i * Q + q in call `generation` under `seed` -- so a slice (pair_base, pairs) of a population is bitwise those rows
 * of the whole one.  (pair_base + pairs) * Q must stay below 2^56 (the sample ids of pds_gaussian_sample).
 *
 * pds_es_perturb: d_theta[2 i, j] = fmaf(sigma, eps_i[j], mu[j]), d_theta[2 i + 1, j] = fmaf(-sigma, eps_i[j], mu[j]);
 * d_theta is [2 pairs, n], the layout of pds_evaluate_policies' d_params for n = pds_mlp_param_count.  sigma > 0.
 *
 * pds_es_gradient: d_grad[j] = scale * sum_i d_pair_weights[i] * eps_i[j] + l2 * d_mu[j] (no l2 term when d_mu is NULL), the
 * noise REGENERATED from the contract -- it is never stored and theta is not read.  Summed in a fixed order (chunks of pairs
 * into [n] partial slabs in d_workspace, the slabs added in chunk order; no atomics): the same inputs give the same bits on
 * every run and for every grid.  d_workspace: pds_es_workspace_floats(n, pairs) = ceil(pairs / chunk) * n floats.
 * PDS_EINVAL (before any device call): a NULL pointer (other than d_mu of pds_es_gradient), n < 1, pairs < 1, ids beyond
 * 2^56, sigma not finite or <= 0, scale or l2 not finite. */
int64_t pds_es_workspace_floats(int64_t n, int64_t pairs); /* host only */
int pds_es_perturb(const float *d_mu, int64_t n, int64_t pairs, float sigma, uint64_t seed, uint64_t generation,
                   uint64_t pair_base, float *d_theta /* [2 pairs, n] */, void *stream);
int pds_es_gradient(const float *d_pair_weights /* [pairs] */, const float *d_mu /* [n] or NULL */, int64_t n, int64_t pairs,
                    float scale, float l2, uint64_t seed, uint64_t generation, uint64_t pair_base, float *d_grad /* [n] */,
                    float *d_workspace, void *stream);

/* The deterministic policy gradient of DDPG (algs/ddpg/ddpg.py:316-340, 431-464; ddpg.py DDPGTrainer; csrc/pds_ddpg.hip).  No
 * handle: the entry points run on the current device, asynchronously on `stream`, allocate nothing and never synchronise
 * (graph-capturable).  pi is the actor D -> h1 -> h2 -> 4 (its output is act_limit * tanh(MLP)), q the Q network
 * D + 4 -> h1 -> h2 -> 1 over rows [obs | act]; the hidden activation of each is relu or tanh, chosen independently.
 * Built for D + 4 <= 64 and h1, h2 <= 64 of both networks: pds_ddpg_supported answers 1 / 0 beforehand.
 * PDS_EINVAL (before any device call): a NULL pointer (other than d_index and opt), B < 1, a network outside
 * pds_mlp's range, an actor with d_out != 4, a Q network with d_out != 1 or d_in != D + 4.  PDS_EUNSUPPORTED: D + 4 > 64.
 *
 * pds_ddpg_policy_grad: d_grads[pds_mlp_param_count(pi)] = the gradient of -mean_g Q(o_g, act_limit tanh(pi(o_g)))
 * (compute_loss_pi, algs/ddpg/ddpg.py:336-340) with respect to the ACTOR's parameters, o_g = the first D columns of row
 * d_index[g] (or g when d_index is NULL) of d_oa [rows, D + 4]: the gradient runs backwards through Q into its action
 * columns and from there through the actor.  Q's parameters are only read, the stored actions are not read at all.
 * d_stats[4] = {sum_g Q(o_g, pi(o_g)), 0, 0, B}.  opt != NULL: the partial-sum kernel also takes the torch.optim.Adam step on
 * pi (the arithmetic of pds_adam_step: both routes give the same bits, as pds_value_grad_step).  d_workspace:
 * pds_ddpg_workspace_floats(pi, q) floats (host only; PDS_EINVAL / PDS_EUNSUPPORTED as above).  Summed in a fixed order
 * without atomics: the same inputs give the same bits.
 *
 * pds_ddpg_target: for g < B and i = d_index[g] (or g): d_target_rows[i] = d_rew[i] + gamma * (1 - d_done[i]) *
 * Q_targ(obs2_i, act_limit tanh(pi_targ(obs2_i))), obs2_i = row i of d_obs2 [rows, D]; d_rew, d_done (0 / 1 as float) and
 * d_target_rows are [rows]; the products and the sum are rounded separately (the Bellman backup of compute_loss_q,
 * algs/ddpg/ddpg.py:323-326).  Written at the ROW, not at g -- pds_value_grad reads target[index[g]] -- so the Q update is
 * pds_value_grad_step on d_oa with the same index; rows outside the index are left alone, repeated indices write the same
 * bits.
 *
 * pds_polyak: t = rn(rn(polyak * t) + rn((float)(1 - polyak) * s)) for every parameter t of `targ` and s of `src` (two
 * networks of one shape; the six tensors in one launch), 1 - polyak formed in double: the bits of the reference's
 * p_targ.mul_(polyak); p_targ.add_((1 - polyak) * p) (algs/ddpg/ddpg.py:459-464).  PDS_EINVAL: shapes that differ, polyak
 * outside [0, 1]. */
int pds_ddpg_supported(const pds_mlp *pi, const pds_mlp *q);
int64_t pds_ddpg_workspace_floats(const pds_mlp *pi, const pds_mlp *q); /* host only */
int pds_ddpg_policy_grad(const pds_mlp *pi, const pds_mlp *q, const float *d_oa, const int64_t *d_index, int64_t B,
                         float act_limit, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                         void *stream);
int pds_ddpg_target(const pds_mlp *pi_targ, const pds_mlp *q_targ, const float *d_obs2, const int64_t *d_index, int64_t B,
                    const float *d_rew, const float *d_done, float gamma, float act_limit, float *d_target_rows,
                    void *stream);
int pds_polyak(const pds_mlp *targ, const pds_mlp *src, double polyak, void *stream);

/* Soft Actor-Critic (algs/sac/sac.py:35-124, 295-337, 439-474; sac.py SACTrainer; csrc/pds_sac.hip).  No handle: the entry
 * points run on the current device, asynchronously on `stream`, allocate nothing and never synchronise (graph-capturable).
 * pi is the squashed-Gaussian actor D -> h1 -> h2 -> 8 as ONE pds_mlp: rows 0 .. 3 of w3 / b3 are the reference's mu_layer,
 * rows 4 .. 7 its log_std_layer.  q1, q2 are the twin Q networks D + 4 -> h1 -> h2 -> 1 over rows [obs | act], of one shape and
 * activation; the hidden activation is relu or tanh, chosen independently for the actor and the Qs.
 * Built for D + 4 <= 64 and h1, h2 <= 64 of the three networks: pds_sac_supported answers 1 / 0 beforehand.
 * PDS_EINVAL (before any device call): a NULL pointer (other than d_index, d_logp and opt), B < 1 (n < 1), a network outside
 * pds_mlp's range, an actor with d_out != 8, a Q network with d_out != 1 or d_in != D + 4, q1 and q2 of different shape or
 * activation, sample ids beyond 2^56.  PDS_EUNSUPPORTED: D + 4 > 64.
 *
 * The sample.  From a row [mu | log_std] of the actor's output: ls = clamp(log_std, -20, 2), u = fmaf(exp(ls), eps, mu),
 * a = act_limit * tanh(u), logp = sum_j (-0.5 eps_j^2 - ls_j - 0.5 log 2 pi) - sum_j 2 (log 2 - u_j - softplus(-2 u_j)) with
 * softplus(x) = max(x, 0) + log1p(exp(-|x|)) (SquashedGaussianMLPActor.forward, algs/sac/sac.py:47-76).
 * Noise contract: eps of sample g -- its POSITION in the call's batch, not its buffer row, so repeated rows get independent
 * noise -- is the four variates pds_gaussian_sample draws for sample id id_base + g (id_base = 0 in pds_sac_target and
 * pds_sac_policy_grad), block 0, in `call` under `seed`: pds_gaussian_sample with mu = 0, log_std = 0 and d_out = 4 returns them.
 *
 * pds_sac_sample: d_act[n, 4] and d_logp[n] (or NULL) from d_head [n, 8]; deterministic != 0: eps = 0, a = act_limit tanh(mu).
 *
 * pds_sac_target: for g < B and i = d_index[g] (or g): a2, logp2 = the sample of the CURRENT policy pi at obs2_i = row i of
 * d_obs2 [rows, D]; d_target_rows[i] = d_rew[i] + gamma * (1 - d_done[i]) * (min(Q1_targ, Q2_targ)(obs2_i, a2) - alpha * logp2),
 * every product and sum rounded separately (the backup of compute_loss_q, algs/sac/sac.py:303-311).  Written at the ROW, as
 * pds_ddpg_target: the Q update is pds_value_grad_step on d_oa with the same index, once per Q network; rows outside the index
 * are left alone.  With alpha = 0, q2_targ = q1_targ and sigma too small to move u off mu it gives the bits of pds_ddpg_target.
 *
 * pds_sac_policy_grad: d_grads[pds_mlp_param_count(pi)] = the gradient of mean_g (alpha logp_g - min(Q1, Q2)(o_g, a_g))
 * (compute_loss_pi, algs/sac/sac.py:324-337) with respect to the ACTOR's parameters, o_g = the first D columns of row d_index[g]
 * (or g) of d_oa [rows, D + 4]: through the smaller Q into its action columns, through tanh and u = mu + exp(ls) eps into both
 * heads; the log_std head receives no gradient where the clamp binds (torch.clamp: open on [-20, 2] inclusive).  Where
 * Q1 == Q2 the gradient is Q1's.  Q1 and Q2 are only read, the stored actions are not read at all.
 * d_stats[4] = {sum_g min Q, sum_g logp_g, 0, B}.  opt != NULL: the partial-sum kernel also takes the torch.optim.Adam step on pi
 * (the arithmetic of pds_adam_step: both routes give the same bits).  d_workspace: pds_sac_workspace_floats(pi, q1, q2) floats
 * (host only; PDS_EINVAL / PDS_EUNSUPPORTED as above).  Summed in a fixed order without atomics: the same inputs give the same
 * bits. */
int pds_sac_supported(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2);
int64_t pds_sac_workspace_floats(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2); /* host only */
int pds_sac_sample(const float *d_head /* [n, 8] actor output */, int64_t n, float act_limit, uint64_t seed, uint64_t call,
                   uint64_t id_base, int deterministic, float *d_act /* [n, 4] */, float *d_logp /* [n] or NULL */, void *stream);
int pds_sac_target(const pds_mlp *pi, const pds_mlp *q1_targ, const pds_mlp *q2_targ, const float *d_obs2, const int64_t *d_index,
                   int64_t B, const float *d_rew, const float *d_done, float gamma, float alpha, float act_limit, uint64_t seed,
                   uint64_t call, float *d_target_rows, void *stream);
int pds_sac_policy_grad(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2, const float *d_oa, const int64_t *d_index,
                        int64_t B, float alpha, float act_limit, uint64_t seed, uint64_t call, float *d_grads, float *d_stats,
                        float *d_workspace, const pds_adam *opt, void *stream);

/* ---- The fused off-policy collection (csrc/pds_collect.h): K closed-loop vector steps of a DDPG / SAC trainer in ONE launch,
 * the transitions written into the replay ring the update entry points above read in place.
 *
 * pds_collect: for s = 0 .. K - 1, with ring block b(s) = (ptr + s N) mod capacity (N = the handle's envs; ptr and capacity are
 * multiples of N, so a block never straddles the wrap):
 *   a     = mode 0 (DDPG, actor d_out 4): clamp(fmaf(exp(d_log_std[q]), z_q, act_limit * tanh(pi(o)_q)), +-act_limit)
 *           mode 1 (SAC,  actor d_out 8): act_limit * tanh(fmaf(exp(clamp(log_std)), z, mu)) on the head row [mu | log_std]
 *           with pi(o) the bits of pds_mlp_forward and z the variates pds_gaussian_sample draws for sample id = env row, block 0,
 *           call = first_call + s under `seed`: the bits of pds_mlp_forward + pds_ddpg_explore / pds_sac_sample
 *   env.step(a): the bits of pds_step
 *   d_oa  [b(s) + i] = [o_i(s) | a_i]      d_obs2[b(s) + i] = the final observation where env i finished, else o_i(s + 1)
 *   d_rew [b(s) + i] = the step reward      d_done[b(s) + i] = 1.f where terminated and not truncated, else 0.f
 * d_obs [N, D]: in o(0) (what pds_reset / pds_step returned last), out o(K).  d_ep_ret / d_ep_len [N]: running return and length
 * of every env, in / out (zero where the env finished).  The handle's state and tick advance K steps.
 * d_tile_stats [ceil(N / 64), 8], written without atomics, every row: over the episodes of that 64-env tile that finished within
 * the launch { count, sum, sum of squares, min, max of the return, sum, min, max of the length }; neutral values 0, +inf, -inf.
 * PDS_EINVAL: K < 1, a mode other than 0 / 1, a NULL pointer (d_log_std may be NULL in mode 1), a call before pds_reset, an actor
 * whose d_out does not match the mode, act_limit <= 0, capacity < N, ptr or capacity not a multiple of N, ptr outside
 * [0, capacity), d_oa / d_obs2 not 16-byte aligned.  PDS_EUNSUPPORTED: a handle without auto_reset; an env configuration outside
 * { control_mode PWM, no latency ring, no Kalman hold, no ground effect, noise all off or domain randomisation + thrust noise +
 * observation noise, TakeOff without motor dynamics }; an actor with d_in != the handle's observation width, more than 64 inputs
 * or hidden units, or another activation than relu / tanh -- pds_collect_supported answers 1 / 0 beforehand.  A refused call
 * leaves the handle and every buffer as they were.
 *
 * pds_ddpg_explore: DDPG's exploration rule above as an elementwise entry point, d_act[n, 4] from the actor's pre-tanh output
 * d_net_out [n, 4] (both 16-byte aligned), z of row i = the variates of pds_gaussian_sample for sample id id_base + i. */
int pds_collect_supported(const pds_handle *h, const pds_mlp *pi, int mode);
int pds_collect(pds_handle *h, int K, int mode, const pds_mlp *pi, float act_limit, const float *d_log_std /* DDPG: [4]; SAC: NULL */,
                uint64_t seed, uint64_t first_call, float *d_oa, float *d_obs2, float *d_rew, float *d_done, int64_t capacity,
                int64_t ptr, float *d_obs, float *d_ep_ret, float *d_ep_len, float *d_tile_stats, void *stream);
int pds_ddpg_explore(const float *d_net_out /* [n, 4] */, const float *d_log_std, int64_t n, float act_limit, uint64_t seed,
                     uint64_t call, uint64_t id_base, float *d_act, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_H */
