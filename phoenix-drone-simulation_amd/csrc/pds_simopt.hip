// pds_simopt.hip -- the fused sim-opt objective for MI355X (gfx950, wave64): P parameter candidates x M logged
// mini-trajectories per launch.
//
// Reference (paths relative to phoenix_drone_simulation/): simopt/pybullet.py:72-248 (ObjectiveFunctionPyBullet.evaluate,
// evaluate_once, loss_function, set_parameters), envs/agents.py:208-224 (update_motor_dynamics), 388-404 (set_latency).
//
// Mapping: ONE CANDIDATE PER WAVE, 64 mini-trajectories on its lanes (M tiled in 64s).  The candidate's A, K and buf_size are
// then wave-uniform: they live in SGPRs and every branch on them is uniform.  The env state (12 floats), the motor state (4) and
// the loss accumulator stay in registers for the whole sample; the only streams are the shared data set -- time-major, one
// 16 B load per lane and step, read by all P candidates and therefore cache-resident -- and one float per (p, m) out.  The kernel
// is bound by the vector ALU and by latency, not by HBM.
//
// The delayed-action ring is not materialised: both resets of evaluate_once zero it and its index, so the ring is a pure delay
// line -- physics sub-step n applies the action of sub-step n - buf_size (zero before that) -- and the delayed action is a load
// from the data set at an earlier, wave-uniform time index.  Same values as the ring of step_once, no registers, no LDS.
//
// The sub-step itself is csrc/pds_physics.h, the blocks step_once expands: the simulated observations agree bit for bit
// with pds_step_k replaying the same actions (tests/test_gpu_simopt.py).
#include "pds_simopt.h"
#include "pds_physics.h"

namespace pds {

namespace {

constexpr int kSimoptBlock = 256;
constexpr int kSimoptWaves = kSimoptBlock / kWave;

// The action the controller sees in physics sub-step n of a phase that started with a zeroed ring: the action of sub-step
// n - buf_size.  `wait` counts the sub-steps that still see zeros, (`row`, `sub`) is the position of the delayed stream.
struct DelayLine {
  int wait, row, sub;
  PDS_DEV void start(int buf_size) { wait = buf_size; row = 0; sub = 0; }
  PDS_DEV float4 next(const float4 *rows, int m_total, int mc, int agg) {  // all members wave-uniform
    if (wait > 0) {
      --wait;
      return make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float4 v = rows[(size_t)row * (size_t)m_total + (size_t)mc];
    if (++sub == agg) { sub = 0; ++row; }
    return v;
  }
};

__global__ __launch_bounds__(kSimoptBlock) void simopt_kernel(const SimoptArgs a) {
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int tiles = (a.M + kWave - 1) / kWave;
  const long long w = (long long)blockIdx.x * kSimoptWaves + wave;
  if (w >= (long long)a.P * tiles) return;  // (wave-uniform)
  const int p = (int)(w / tiles);
  const int tile = (int)(w - (long long)p * tiles);
  const int m = tile * kWave + lane;
  const bool live = m < a.M;
  const int mc = live ? m : a.M - 1;  // lanes past the end recompute the last sample; their stores are masked

  // ---- set_parameters (simopt/pybullet.py:233-248) in the reference's float64, rounded once ----
  const Consts &k = a.k;
  Params par;
  default_params(k, par);
  {
    const double t2w = fmax((double)a.params[3 * (size_t)p], 0.0);
    const double T = fmax(fmax((double)a.params[3 * (size_t)p + 1], 0.0), a.time_step);  // clipped to >= T_s
    const float A = (float)(1.0 - a.time_step / T);
    const float K = (float)(0.028 * a.G * t2w / 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { par.A[j] = A; par.K[j] = K; }
  }
  const int buf_size = min(max(a.lat_steps[p], 0), kMaxLatSteps);
  const int agg = k.agg;

  // ---- 1) pre-steps from a reset env: only the motor state survives them, and it depends on the actions alone ----
  float xm[4] = {0.f, 0.f, 0.f, 0.f};
  float ou_unused[4] = {0.f, 0.f, 0.f, 0.f};
  DelayLine line;
  line.start(buf_size);
  for (int n = 0; n < a.pre_steps * agg; ++n) {
    const float4 d = line.next(a.pre, a.M, mc, agg);
    const float av[4] = {d.x, d.y, d.z, d.w};
    float pwmv[4], f[4];
    PDS_PWM_FROM_ACTION()
    PDS_MOTOR_THRUST(true, false, ou_unused, ou_unused)
  }

  // ---- 2) + 3) second reset: the logged state, ring zeroed again, motor state kept ----
  const float4 *obs = a.obs;
  const size_t M = (size_t)a.M;
  EnvRegs e;
  {
    const float4 s0 = obs[mc], s1 = obs[M + mc], s2 = obs[2 * M + mc];
    e = EnvRegs{s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w};
  }
  Quat q = quat_from_euler(e.roll, e.pitch, e.yaw);
  const float inv_m = fast_rcp(par.m), inv_Jx = fast_rcp(par.Jx), inv_Jy = fast_rcp(par.Jy), inv_Jz = fast_rcp(par.Jz);
  line.start(buf_size);

  // ---- 4) replay + discounted loss (simopt/pybullet.py:166-227) ----
  float acc = 0.f;
  double discount = 1.0;  // gamma^i in float64 like the reference (one multiply per step)
  for (int i = 0; i + 1 < a.T; ++i) {
    for (int sub = 0; sub < agg; ++sub) {
      const float4 d = line.next(a.acts, a.M, mc, agg);
      const float av[4] = {d.x, d.y, d.z, d.w};
      float pwmv[4], f[4];
      PDS_PWM_FROM_ACTION()
      PDS_MOTOR_THRUST(true, false, ou_unused, ou_unused)
      PDS_RIGID_BODY_SUBSTEP(false, true)
    }
    if (a.sim_obs != nullptr && live) {
      float *row = a.sim_obs + (((size_t)i * (size_t)a.P + (size_t)p) * M + (size_t)m) * 13;
      row[0] = e.px; row[1] = e.py; row[2] = e.pz;
      row[3] = q.x; row[4] = q.y; row[5] = q.z; row[6] = q.w;
      row[7] = e.vx; row[8] = e.vy; row[9] = e.vz;
      row[10] = e.wx; row[11] = e.wy; row[12] = e.wz;
    }
    const float4 *tgt = obs + (size_t)(i + 1) * 3 * M;
    const float4 r0 = tgt[mc], r1 = tgt[M + mc], r2 = tgt[2 * M + mc];  // x y z vx | vy vz roll pitch | yaw wx wy wz
    float roll, pitch, yaw;
    euler_from_quat(q, roll, pitch, yaw);
    const float err[12] = {roll - r1.z, pitch - r1.w, yaw - r2.x,
                           100.f * (e.px - r0.x), 100.f * (e.py - r0.y), 100.f * (e.pz - r0.z),
                           10.f * (e.vx - r0.w), 10.f * (e.vy - r1.x), 10.f * (e.vz - r1.y),
                           e.wx - r2.y, e.wy - r2.z, e.wz - r2.w};
    float l1 = 0.f, l2 = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) { l1 += fabsf(err[j]); l2 = fmaf(err[j], err[j], l2); }
    acc += (float)discount * (l1 + fast_sqrt(l2));
    discount *= a.gamma;
  }
  if (live) a.loss[(size_t)p * M + (size_t)m] = acc / (float)(a.T - 1);
}

// score[p] = mean over m of loss[p, m]: one wave per candidate, every lane sums its strided share in order, then a fixed
// butterfly over the lanes -- float64 throughout, no atomics: the result depends on row p of d_loss alone.
__global__ __launch_bounds__(kSimoptBlock) void simopt_score_kernel(const float *loss, float *score, int P, int M) {
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const long long p = (long long)blockIdx.x * kSimoptWaves + (long long)(threadIdx.x / kWave);
  if (p >= P) return;
  const float *row = loss + (size_t)p * (size_t)M;
  double s = 0.0;
  for (int m = lane; m < M; m += kWave) s += (double)row[m];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  if (lane == 0) score[p] = (float)(s / (double)M);
}

}  // namespace

void launch_simopt(const SimoptArgs &a, hipStream_t s) {
  const long long tiles = (a.M + kWave - 1) / kWave;
  const long long waves = (long long)a.P * tiles;
  hipLaunchKernelGGL(simopt_kernel, dim3((unsigned)((waves + kSimoptWaves - 1) / kSimoptWaves)), dim3(kSimoptBlock), 0, s, a);
  hipLaunchKernelGGL(simopt_score_kernel, dim3((unsigned)((a.P + kSimoptWaves - 1) / kSimoptWaves)), dim3(kSimoptBlock), 0, s,
                     (const float *)a.loss, a.score, a.P, a.M);
}

}  // namespace pds
