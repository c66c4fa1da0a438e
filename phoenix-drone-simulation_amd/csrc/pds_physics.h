// pds_physics.h -- the ONE statement of a SimplePhysics sub-step: PWM -> (PT1 motor) -> thrust -> Newton-Euler ->
// semi-implicit Euler -> quaternion.  step_once (csrc/pds_step.h) and the sim-opt objective (csrc/pds_simopt.hip) both
// expand these blocks, so under -ffp-contract=on (contraction decided per source expression) the two evaluate the same
// operation sequence and agree bit for bit.
//
// They are MACROS, not device functions, on purpose: step_once had this code inline, and the macros expand to the very
// tokens it had, so every kernel that existed before the sim-opt objective compiles to what it compiled to (as functions --
// forced inline, same expressions -- the register allocation of ~200 of the step / K-step / rollout kernels moved by a VGPR
// or a spill).  Each block names the locals it expects in the expanding scope.
//
// Reference (paths relative to phoenix_drone_simulation/): envs/control.py:94-100, envs/agents.py:259-298,
// envs/physics.py:130-200.
#pragma once
#include "pds_types.h"

// PWM.act (envs/control.py:94-100): action in [-1, 1] -> PWM in [0, 60000].  Scope: float av[4], pwmv[4].
#define PDS_PWM_FROM_ACTION()                                                                   \
  _Pragma("unroll")                                                                             \
  for (int j = 0; j < 4; ++j) pwmv[j] = 30000.f + clampf(av[j], -1.f, 1.f) * 30000.f;

// CrazyFlieAgent.apply_action from the PWMs on (envs/agents.py:278-293): OU thrust noise (TN_; OU_ its state, OU_Z_ its four
// standard variates), PT1 motor state xm (MOTOR_), per-motor thrust f.  Scope: const Consts &k; Params par; float pwmv[4],
// f[4]; float *xm.
#define PDS_MOTOR_THRUST(MOTOR_, TN_, OU_, OU_Z_)                                               \
  _Pragma("unroll")                                                                             \
  for (int j = 0; j < 4; ++j) {                                                                 \
    const float un = pwmv[j] * (1.0f / 60000.f);                                                \
    float noise1 = 1.0f;                                                                        \
    if (TN_) { /* OUNoise.noise, envs/utils.py:104-108 (theta .15, mu 0); never reset */        \
      OU_[j] = OU_[j] + (0.15f * (0.f - OU_[j]) + k.ou_sigma * OU_Z_[j]);                       \
      noise1 = 1.0f + OU_[j];                                                                   \
    }                                                                                           \
    float n;                                                                                    \
    if (MOTOR_) {                                                                               \
      xm[j] = par.A[j] * xm[j] + (1.0f - par.A[j]) * fast_sqrt(un);                             \
      n = noise1 * (xm[j] * xm[j]);                                                             \
    } else {                                                                                    \
      n = noise1 * un;                                                                          \
    }                                                                                           \
    f[j] = par.K[j] * clampf(n, 0.f, 1.f);                                                      \
  }

// SimplePhysics.step_forward from the motor forces on (envs/physics.py:160-182).  q is the quaternion of the PREVIOUS
// sub-step on entry and, when REQUAT_, Q(new rpy) on exit.  Scope: const Consts &k; Params par; float f[4]; EnvRegs e; Quat q;
// float inv_m, inv_Jx, inv_Jy, inv_Jz (v_rcp_f32 of the mass / inertia).
#define PDS_RIGID_BODY_SUBSTEP(GE_, REQUAT_)                                                    \
  /* yaw torque: sum of +-(ftf1*f_i + ftf0); ftf0 cancels (envs/agents.py:295-297) */           \
  const float tz_ = par.ftf1 * (-f[0] + f[1] - f[2] + f[3]);                                    \
  float R[9];                                                                                   \
  matrix_from_quat(q, R); /* envs/physics.py:160 (quaternion of the PREVIOUS step) */           \
  if (GE_) {                                                                                    \
    /* BasePhysics.calculate_ground_effect, envs/physics.py:27-58, applied as extra per-motor   \
       thrust (envs/physics.py:117-120); branch-free per-env scale */                           \
    const float ok = (fabsf(e.roll) < kHalfPi && fabsf(e.pitch) < kHalfPi) ? 1.f : 0.f;         \
    const float ox[4] = {0.028f, -0.028f, -0.028f, 0.028f};                                     \
    const float oy[4] = {-0.028f, -0.028f, 0.028f, 0.028f};                                     \
    _Pragma("unroll")                                                                           \
    for (int j = 0; j < 4; ++j) {                                                               \
      const float hz = fmaxf(e.pz + (R[6] * ox[j] + R[7] * oy[j]), k.h_clip);                   \
      const float qq = k.prop_r * fast_rcp(4.f * hz);                                           \
      f[j] = f[j] + ok * (f[j] * k.gec * (qq * qq));                                            \
    }                                                                                           \
  }                                                                                             \
  const float thrust = ((f[0] + f[1]) + f[2]) + f[3];                                           \
  const float Fx = R[2] * thrust, Fy = R[5] * thrust, Fz = R[8] * thrust - k.G * par.m;         \
  const float tx_ = (-f[0] - f[1] + f[2] + f[3]) * k.Lq; /* envs/physics.py:167 */              \
  const float ty_ = (-f[0] + f[1] + f[2] - f[3]) * k.Lq; /* envs/physics.py:168 */              \
  const float Jwx = par.Jx * e.wx, Jwy = par.Jy * e.wy, Jwz = par.Jz * e.wz;                    \
  const float t0 = tx_ - (e.wy * Jwz - e.wz * Jwy); /* tau - w x (J w), physics.py:170-171 */   \
  const float t1 = ty_ - (e.wz * Jwx - e.wx * Jwz);                                             \
  const float t2 = tz_ - (e.wx * Jwy - e.wy * Jwx);                                             \
  const float dt = par.dt;                                                                      \
  e.vx += dt * (Fx * inv_m); e.vy += dt * (Fy * inv_m); e.vz += dt * (Fz * inv_m);    /* :173,175 */ \
  e.wx += dt * (t0 * inv_Jx); e.wy += dt * (t1 * inv_Jy); e.wz += dt * (t2 * inv_Jz); /* :172,176 */ \
  e.px += dt * e.vx; e.py += dt * e.vy; e.pz += dt * e.vz;                            /* :177 */ \
  e.roll += dt * e.wx; e.pitch += dt * e.wy; e.yaw += dt * e.wz;                      /* :178 */ \
  if (REQUAT_) q = quat_from_euler(e.roll, e.pitch, e.yaw);                           /* :179 */ \
  e.pz = fmaxf(e.pz, 0.f);                                                            /* :182 */
