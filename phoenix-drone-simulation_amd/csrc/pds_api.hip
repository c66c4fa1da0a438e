// pds_api.hip -- host side of libpds_hip.so: the C ABI of include/pds.h (+ the state pack/unpack
// kernel behind pds_get_state / pds_set_state).  The fused step / reset kernels live in pds_step.h /
// pds_reset.h and are instantiated per task in pds_task_{hover,circle,takeoff}.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "pds_reset.h"  // (pds_types.h + regen_kept_obs for pds_get_state)
#include "pds_physics.h"  // (the sub-step blocks for materialize_state_kernel)
#include "pds_collect_args.h"
#include "pds_evaluate_args.h"
#include "pds_evaluate_deep_args.h"
#include "pds_evaluate_deep_forms_args.h"
#include "pds_evaluate_hist_args.h"
#include "pds_rollout_deep_args.h"
#include "pds_simopt.h"
#include "../../include/pds_history_latency.h"
#include "../../include/pds_history_latency_evaluate.h"

namespace pds {

// ---- state access (parity injection, checkpointing) -------------------------------------------
struct FieldArgs {
  DevState st;
  Consts k;
  void *user;
  long long n;
  int field;
  int task;
  int set;
  int has_motor, has_dr, has_tn, has_on, ctrl;
  int regen_obs;  // observation noise without the Kalman hold: the kept observation is regenerated unless kCtrOhBit (pds_types.h)
  unsigned long long env_id_base;
  uint32_t seed_lo, seed_hi;
};

__global__ __launch_bounds__(kBlock) void field_kernel(const FieldArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  float *uf = reinterpret_cast<float *>(a.user);
  int32_t *ui = reinterpret_cast<int32_t *>(a.user);
  float4 q0 = a.st.s0[i], q1 = a.st.s1[i], q2 = a.st.s2[i];
  const uint32_t c = a.st.ctr[i];
  const int parity = (int)(a.st.clk[0].z & 1u);  // every tile's clock holds the same value between launches
  switch (a.field) {
    case PDS_F_POS:
      if (a.set) { q0.x = uf[3 * i]; q0.y = uf[3 * i + 1]; q0.z = uf[3 * i + 2]; a.st.s0[i] = q0; }
      else { uf[3 * i] = q0.x; uf[3 * i + 1] = q0.y; uf[3 * i + 2] = q0.z; }
      break;
    case PDS_F_VEL:
      if (a.set) { q0.w = uf[3 * i]; q1.x = uf[3 * i + 1]; q1.y = uf[3 * i + 2]; a.st.s0[i] = q0; a.st.s1[i] = q1; }
      else { uf[3 * i] = q0.w; uf[3 * i + 1] = q1.x; uf[3 * i + 2] = q1.y; }
      break;
    case PDS_F_RPY:
      if (a.set) { q1.z = uf[3 * i]; q1.w = uf[3 * i + 1]; q2.x = uf[3 * i + 2]; a.st.s1[i] = q1; a.st.s2[i] = q2; }
      else { uf[3 * i] = q1.z; uf[3 * i + 1] = q1.w; uf[3 * i + 2] = q2.x; }
      break;
    case PDS_F_OMEGA:
      if (a.set) { q2.y = uf[3 * i]; q2.z = uf[3 * i + 1]; q2.w = uf[3 * i + 2]; a.st.s2[i] = q2; }
      else { uf[3 * i] = q2.y; uf[3 * i + 1] = q2.z; uf[3 * i + 2] = q2.w; }
      break;
    case PDS_F_QUAT:
      if (!a.set) {
        const Quat q = quat_from_euler(q1.z, q1.w, q2.x);
        const float sgn = ctr_sign(c) ? -1.f : 1.f;
        uf[4 * i] = sgn * q.x; uf[4 * i + 1] = sgn * q.y; uf[4 * i + 2] = sgn * q.z; uf[4 * i + 3] = sgn * q.w;
      }
      break;
    case PDS_F_MOTOR_X:
    case PDS_F_LAST_ACTION:
    case PDS_F_PREV_ACTION:
    case PDS_F_MOTOR_A:
    case PDS_F_MOTOR_K:
    case PDS_F_OU: {
      float4 *arr = nullptr;
      float4 dflt = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.field == PDS_F_MOTOR_X) arr = a.has_motor ? a.st.mx : nullptr;
      else if (a.field == PDS_F_LAST_ACTION) arr = a.st.hist[parity];
      else if (a.field == PDS_F_PREV_ACTION) arr = a.st.hist[parity ^ 1];
      else if (a.field == PDS_F_OU) arr = a.has_tn ? a.st.ou : nullptr;
      else if (a.field == PDS_F_MOTOR_A) { arr = (a.has_motor && a.has_dr) ? a.st.mA : nullptr; dflt = make_float4(a.k.A, a.k.A, a.k.A, a.k.A); }
      else { arr = (a.has_motor && a.has_dr) ? a.st.mK : nullptr; dflt = make_float4(a.k.K, a.k.K, a.k.K, a.k.K); }
      if (a.set) { if (arr) arr[i] = make_float4(uf[4 * i], uf[4 * i + 1], uf[4 * i + 2], uf[4 * i + 3]); }
      else { const float4 v = arr ? arr[i] : dflt; uf[4 * i] = v.x; uf[4 * i + 1] = v.y; uf[4 * i + 2] = v.z; uf[4 * i + 3] = v.w; }
      break;
    }
    case PDS_F_STEP_COUNT:
      if (a.set) {
        uint32_t off = ctr_off(c);
        const uint32_t s_new = (uint32_t)ui[i] & 0xFFFFu;
        if (a.task == PDS_TASK_CIRCLE)  // keep ref_offset: the stored phase is (steps + ref_offset) mod num_ref_points
          off = (circle_ref_offset(c, a.k.ref_points) + s_new % (uint32_t)a.k.ref_points) % (uint32_t)a.k.ref_points;
        a.st.ctr[i] = ctr_pack(s_new, ctr_sign(c), off, ctr_lat(c)) | (c & kCtrOhBit);
      }
      else ui[i] = (int32_t)ctr_step(c);
      break;
    case PDS_F_QUAT_SIGN:
      if (a.set) a.st.ctr[i] = ctr_pack(ctr_step(c), ui[i] ? 1u : 0u, ctr_off(c), ctr_lat(c)) | (c & kCtrOhBit);
      else ui[i] = (int32_t)ctr_sign(c);
      break;
    case PDS_F_REF_OFFSET:
      if (a.task == PDS_TASK_CIRCLE) {
        const uint32_t P = (uint32_t)a.k.ref_points;
        if (a.set) a.st.ctr[i] = ctr_pack(ctr_step(c), ctr_sign(c), ((uint32_t)ui[i] % P + ctr_step(c) % P) % P, ctr_lat(c)) | (c & kCtrOhBit);
        else ui[i] = (int32_t)circle_ref_offset(c, a.k.ref_points);
      } else if (!a.set) {
        ui[i] = 0;
      }
      break;
    case PDS_F_PARAMS:
      if (a.has_dr) {
        if (a.set) {
          a.st.par0[i] = make_float4(uf[6 * i], uf[6 * i + 1], uf[6 * i + 2], uf[6 * i + 3]);
          a.st.par1[i] = make_float2(uf[6 * i + 4], uf[6 * i + 5]);
        } else {
          const float4 p0 = a.st.par0[i]; const float2 p1 = a.st.par1[i];
          uf[6 * i] = p0.x; uf[6 * i + 1] = p0.y; uf[6 * i + 2] = p0.z; uf[6 * i + 3] = p0.w; uf[6 * i + 4] = p1.x; uf[6 * i + 5] = p1.y;
        }
      } else if (!a.set) {
        uf[6 * i] = a.k.dt; uf[6 * i + 1] = a.k.m; uf[6 * i + 2] = a.k.Jx; uf[6 * i + 3] = a.k.Jy; uf[6 * i + 4] = a.k.Jz; uf[6 * i + 5] = a.k.ftf1;
      }
      break;
    case PDS_F_GYRO_BIAS:
    case PDS_F_GYRO_LPF:
      if (a.has_on) {
        float4 n0 = a.st.nz0[i]; float2 n1 = a.st.nz1[i];
        if (a.field == PDS_F_GYRO_BIAS) {
          if (a.set) { n0.x = uf[3 * i]; n0.y = uf[3 * i + 1]; n0.z = uf[3 * i + 2]; a.st.nz0[i] = n0; }
          else { uf[3 * i] = n0.x; uf[3 * i + 1] = n0.y; uf[3 * i + 2] = n0.z; }
        } else {
          if (a.set) { n0.w = uf[3 * i]; n1.x = uf[3 * i + 1]; n1.y = uf[3 * i + 2]; a.st.nz0[i] = n0; a.st.nz1[i] = n1; }
          else { uf[3 * i] = n0.w; uf[3 * i + 1] = n1.x; uf[3 * i + 2] = n1.y; }
        }
      } else if (!a.set) { uf[3 * i] = 0.f; uf[3 * i + 1] = 0.f; uf[3 * i + 2] = 0.f; }
      break;
    case PDS_F_NOISY_OBS:
      if (a.has_on) {
        if (a.set) {
          a.st.oh0[i] = make_float4(uf[10 * i], uf[10 * i + 1], uf[10 * i + 2], uf[10 * i + 3]);
          a.st.oh1[i] = make_float4(uf[10 * i + 4], uf[10 * i + 5], uf[10 * i + 6], uf[10 * i + 7]);
          a.st.oh2[i] = make_float2(uf[10 * i + 8], uf[10 * i + 9]);
          if (a.regen_obs) a.st.ctr[i] = c | kCtrOhBit;  // from now on it is what the next step reads
        } else if (a.regen_obs && !ctr_oh(c)) {
          // not in memory: what the next step will regenerate (csrc/pds_reset.h regen_kept_obs), from the same inputs
          const WaveClock ck = a.st.clk[i / kWave];
          const RngKey now{a.seed_lo, a.seed_hi, ck.x, ck.y};
          const EnvRegs e{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
          NoisyObs o;
          regen_kept_obs(a.k, (uint32_t)(a.env_id_base + (unsigned long long)i), now, ctr_step(c) == 0u, e, o);
          uf[10 * i] = o.x; uf[10 * i + 1] = o.y; uf[10 * i + 2] = o.z; uf[10 * i + 3] = o.qx;
          uf[10 * i + 4] = o.qy; uf[10 * i + 5] = o.qz; uf[10 * i + 6] = o.qw; uf[10 * i + 7] = o.vx;
          uf[10 * i + 8] = o.vy; uf[10 * i + 9] = o.vz;
        } else {
          const float4 o0 = a.st.oh0[i], o1 = a.st.oh1[i]; const float2 o2 = a.st.oh2[i];
          uf[10 * i] = o0.x; uf[10 * i + 1] = o0.y; uf[10 * i + 2] = o0.z; uf[10 * i + 3] = o0.w;
          uf[10 * i + 4] = o1.x; uf[10 * i + 5] = o1.y; uf[10 * i + 6] = o1.z; uf[10 * i + 7] = o1.w;
          uf[10 * i + 8] = o2.x; uf[10 * i + 9] = o2.y;
        }
      } else if (!a.set) {
        for (int j = 0; j < 10; ++j) uf[10 * i + j] = 0.f;
      }
      break;
    case PDS_F_PID: {
      float v[12];
      for (int j = 0; j < 12; ++j) v[j] = 0.f;
      if (a.set) {
        for (int j = 0; j < 12; ++j) v[j] = uf[12 * i + j];
        if (a.ctrl >= 1) { a.st.pid0[i] = make_float4(v[0], v[1], v[2], v[3]); a.st.pid1[i] = make_float2(v[4], v[5]); }
        if (a.ctrl == 2) { a.st.pid2[i] = make_float4(v[6], v[7], v[8], v[9]); a.st.pid3[i] = make_float2(v[10], v[11]); }
      } else {
        if (a.ctrl >= 1) { const float4 p0 = a.st.pid0[i]; const float2 p1 = a.st.pid1[i]; v[0] = p0.x; v[1] = p0.y; v[2] = p0.z; v[3] = p0.w; v[4] = p1.x; v[5] = p1.y; }
        if (a.ctrl == 2) { const float4 p2 = a.st.pid2[i]; const float2 p3 = a.st.pid3[i]; v[6] = p2.x; v[7] = p2.y; v[8] = p2.z; v[9] = p2.w; v[10] = p3.x; v[11] = p3.y; }
        for (int j = 0; j < 12; ++j) uf[12 * i + j] = v[j];
      }
      break;
    }
    case PDS_F_ACTION_BUFFER:  // drone.action_buffer, rows >= buf_size read as 0 / are ignored
      for (int b = 0; b < kMaxLatSteps; ++b) {
        const bool live = a.st.lat != nullptr && b < a.k.lat_steps;
        if (a.set) {
          if (live) a.st.lat[(long long)b * a.n + i] = make_float4(uf[32 * i + 4 * b], uf[32 * i + 4 * b + 1], uf[32 * i + 4 * b + 2], uf[32 * i + 4 * b + 3]);
        } else {
          const float4 v = live ? a.st.lat[(long long)b * a.n + i] : make_float4(0.f, 0.f, 0.f, 0.f);
          uf[32 * i + 4 * b] = v.x; uf[32 * i + 4 * b + 1] = v.y; uf[32 * i + 4 * b + 2] = v.z; uf[32 * i + 4 * b + 3] = v.w;
        }
      }
      break;
    case PDS_F_ACTION_IDX:
      if (a.set) a.st.ctr[i] = ctr_pack(ctr_step(c), ctr_sign(c), ctr_off(c), a.k.lat_steps > 0 ? (uint32_t)ui[i] % (uint32_t)a.k.lat_steps : 0u) | (c & kCtrOhBit);
      else ui[i] = (int32_t)ctr_lat(c);
      break;
    default: break;
  }
}

// pds_set_tick / pds_create: every tile's clock word <- (tick, parity kept or 0)
__global__ __launch_bounds__(256) void clock_fill_kernel(WaveClock *clk, long long ntiles, unsigned long long tick, int keep_parity) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t par = keep_parity ? (clk[t].z & 1u) : 0u;
  clk[t] = make_uint4((uint32_t)tick, (uint32_t)(tick >> 32), par, 0u);
}

// pds_set_latency: action buffer and index of every env <- 0 (envs/agents.py:403-404)
__global__ __launch_bounds__(256) void latency_clear_kernel(DevState st, long long n, int rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int b = 0; b < rows; ++b) st.lat[(long long)b * n + i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t c = st.ctr[i];
  st.ctr[i] = ctr_pack(ctr_step(c), ctr_sign(c), ctr_off(c), 0u) | (c & kCtrOhBit);
}

// The kept noisy observation of every env that does not have it in oh0-2 (i.e. every env after a pds_step, none after a
// pds_step_k / pds_rollout / reset) is regenerated there and flagged in the counter word -- what the single-step kernels do in
// their prologue (init_kept_obs), as a pass of its own: in front of the K-step and rollout kernels (so that their loops are not
// compiled around it, csrc/pds_step.h step_k_kernel) and in front of every call that changes the regeneration's inputs without
// stepping the env (materialize_kept_obs below).  Same function, same inputs, same bits.  4 B per env when every env is
// flagged, 52 + 44 B otherwise.
__global__ __launch_bounds__(kBlock) void materialize_oh_kernel(DevState st, Consts k, long long n, unsigned long long env_id_base,
                                                                uint32_t seed_lo, uint32_t seed_hi) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = st.ctr[i];
  if (ctr_oh(c) != 0u) return;
  const WaveClock ck = st.clk[i / kWave];
  const RngKey now{seed_lo, seed_hi, ck.x, ck.y};
  const float4 q0 = st.s0[i], q1 = st.s1[i], q2 = st.s2[i];
  const EnvRegs e{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
  NoisyObs o;
  regen_kept_obs(k, (uint32_t)(env_id_base + (unsigned long long)i), now, ctr_step(c) == 0u, e, o);
  st.oh0[i] = make_float4(o.x, o.y, o.z, o.qx);
  st.oh1[i] = make_float4(o.qy, o.qz, o.qw, o.vx);
  st.oh2[i] = make_float2(o.vy, o.vz);
  st.ctr[i] = c | kCtrOhBit;
}

// s0-s2 of every env whose counter word says that they are one step behind (kCtrBehindBit: the lean single-step kernels store
// them every other step, csrc/pds_step.h skip_state_variant) are advanced by that step -- u(k-1) out of the action ring, the
// blocks of csrc/pds_physics.h in step_once's order, so the bits the skip step computed (-ffp-contract=on: contraction is
// decided per source expression) -- and stored, and the bit is cleared.  What the next write step would do in its prologue, as
// a pass of its own in front of everything else that reads s0-s2, writes them for some envs only or rewrites the counter word
// (materialize_state below).  4 B per env when no env is flagged, 72 + 52 B otherwise.
__global__ __launch_bounds__(kBlock) void materialize_state_kernel(DevState st, Consts k, long long n, int ge) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = st.ctr[i];
  if (ctr_behind(c) == 0u) return;
  const int parity = (int)(st.clk[i / kWave].z & 1u);
  const float4 q0 = st.s0[i], q1 = st.s1[i], q2 = st.s2[i];
  const float4 act = st.hist[parity][i];  // u(k-1)
  EnvRegs e{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
  Params par;
  default_params(k, par);
  float xm_[4] = {0.f, 0.f, 0.f, 0.f}, ou_[4] = {0.f, 0.f, 0.f, 0.f};
  float *xm = xm_;
  Quat q = quat_from_euler(e.roll, e.pitch, e.yaw);
  const float inv_m = fast_rcp(par.m), inv_Jx = fast_rcp(par.Jx), inv_Jy = fast_rcp(par.Jy), inv_Jz = fast_rcp(par.Jz);
  for (int sub = 0; sub < k.agg; ++sub) {
    float av[4] = {act.x, act.y, act.z, act.w};
    float f[4], pwmv[4];
    PDS_PWM_FROM_ACTION()
    PDS_MOTOR_THRUST(false, false, ou_, ou_)
    PDS_RIGID_BODY_SUBSTEP(ge != 0, true)
  }
  st.s0[i] = make_float4(e.px, e.py, e.pz, e.vx);
  st.s1[i] = make_float4(e.vy, e.vz, e.roll, e.pitch);
  st.s2[i] = make_float4(e.yaw, e.wx, e.wy, e.wz);
  st.ctr[i] = c & ~kCtrBehindBit;
}


}  // namespace pds

// =================================================================================================
// the C ABI of include/pds.h
// =================================================================================================
using namespace pds;

struct pds_handle {
  pds_config cfg;
  DevState st;
  Consts k;
  LaunchFlags flags;
  int force_tile;  // PDS_FORCE_TILE=half|full (tests / A-B runs): 1 half, 2 full, 0 pick per launch
  bool store_every_step;  // pds_step launches the kernels that store s0-s2 every step: by size, or PDS_STATE_EVERY_STEP (pds_create)
  float2 *d_circle_ref;
  void *slab;  // one allocation holds every state array (staggered, see pds_create)
  float4 *lat_buf;  // [PDS_MAX_LATENCY_STEPS][N] delayed-action ring, allocated when latency is first enabled
  unsigned long long *d_count;  // pds_count_nonfinite result word (in the slab)
  unsigned long long *d_stamps;  // diagnostic builds: pds_debug_stamps
  void *eval_sink;  // 16 N bytes: the [N] reward, cost (float), term, trunc (u8) rows the steps of pds_evaluate_policies stream into, allocated by its first call
  int obs_dim;
  int num_cus;    // hipDeviceProp.multiProcessorCount (256 on MI355X): drives the half-tile rule
  uint64_t tick;  // host mirror of the device clock words (pds_sync_tick refreshes it)
  bool was_reset;
  bool after_evaluate;  // pds_evaluate_policies ran and no unmasked reset since: every tile stopped at a step of its own
  // state stored every other step (kCtrBehindBit): a lean single-step launch was issued since the last materialize_state /
  // unmasked reset, so s0-s2 of some envs may be one step behind ...
  bool state_maybe_behind;
  // ... and one was issued into a stream capture: a replay steps the envs without the host seeing it, so from then on the
  // handle never knows better and materialize_state always launches its pass
  bool step_captured;
  char err[512];
};

// Every entry point runs on the handle's device and leaves the caller's current device as it found it.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = err == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

static int fail(pds_handle *h, int code, const char *fmt, ...) {
  if (h) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h->err, sizeof(h->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

static thread_local char g_create_err[512] = "";
namespace pds_api_detail {
// what pds_last_error(NULL) returns on this thread, for entry points without a handle (csrc/pds_mlp_deep.hip)
void set_thread_error(const char *msg) { snprintf(g_create_err, sizeof(g_create_err), "%s", msg); }
}  // namespace pds_api_detail

#define PDS_HIP(h, call)                                                                        \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return fail(h, PDS_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// The kept noisy observation of every env into oh0-2 (flagged in the counter word) where the variant regenerates it from the
// previous tick's Philox blocks and the env's state: in front of everything that moves a tile's clock, an env's state or its step
// counter WITHOUT stepping the env -- a masked reset (the reset kernel advances the clock of every tile, also for the envs outside
// the mask), pds_set_tick, the pds_set_state edits -- and in front of the K-step / rollout kernels, which read it from memory.
// The history half of the next observation is then the observation that was returned, as in the reference (envs/base.py:303-319).
static int materialize_kept_obs(pds_handle *h, hipStream_t s) {
  if (!(h->flags.on && !h->flags.hold)) return PDS_OK;
  const long long n = h->cfg.num_envs;
  hipLaunchKernelGGL(pds::materialize_oh_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, h->st, h->k, n,
                     (unsigned long long)h->cfg.env_id_base, (uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32));
  PDS_HIP(h, hipGetLastError());
  return PDS_OK;
}

// The configurations whose single-step kernel stores s0-s2 every other step (csrc/pds_step.h skip_state_variant).
static bool skips_state(const pds_handle *h) {
  const LaunchFlags &f = h->flags;
  return PDS_STATE_EVERY_OTHER_STEP != 0 && !h->store_every_step && !f.motor && !f.dr && !f.tn && !f.on && f.ctrl == 0 && !f.lat;
}

// s0-s2 of every env up to date with its counter word, in front of everything that reads them, writes them for some envs only or
// rewrites the counter word without going through the lean single-step kernel: pds_get_state / pds_set_state (hence checkpoint and
// resume), a masked pds_reset*, pds_set_tick, pds_set_latency (the handle leaves the lean family), pds_step_k, pds_rollout*,
// pds_evaluate_policies*, pds_collect, pds_simopt_evaluate, pds_count_nonfinite.  Not launched when the handle knows that no
// lean step ran since the last pass or unmasked reset.
static int materialize_state(pds_handle *h, hipStream_t s) {
  if (!h->state_maybe_behind && !h->step_captured) return PDS_OK;
  const long long n = h->cfg.num_envs;
  hipLaunchKernelGGL(pds::materialize_state_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, h->st, h->k, n,
                     h->flags.ge ? 1 : 0);
  PDS_HIP(h, hipGetLastError());
  h->state_maybe_behind = false;
  return PDS_OK;
}

extern "C" int pds_version(void) { return PDS_VERSION; }

// ctor defaults: envs/base.py:26-48, envs/hover.py:7-45, envs/circle.py:7-61, envs/takeoff.py:13-56
extern "C" int pds_default_config(int task, pds_config *c) {
  if (!c || task < 0 || task > 2) return PDS_EINVAL;
  memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(pds_config);
  c->task = task;
  c->num_envs = 1;
  c->env_id_base = 0;
  c->seed = 0;
  c->device = 0;
  c->use_motor_dynamics = 0;
  c->use_ground_effect = 0;
  c->observation_noise = 1;
  c->aggregate_phy_steps = 1;
  c->enable_reset_distribution = 1;
  c->max_episode_steps = 500;
  c->auto_reset = 1;
  c->domain_randomization = 0.10;
  c->motor_thrust_noise = 0.05;
  c->time_step = 1.0 / 100.0;
  c->motor_time_constant = 0.080;
  c->penalty_action = 1e-4;
  c->penalty_angle = 0.0;
  c->penalty_spin = (task == PDS_TASK_CIRCLE) ? 1e-3 : 1e-4;
  c->penalty_terminal = 100.0;
  c->penalty_velocity = (task == PDS_TASK_CIRCLE) ? 1e-4 : 0.0;
  c->ARP = (task == PDS_TASK_CIRCLE) ? 1e-3 : 0.0;
  c->target_pos[2] = 1.0;
  c->init_xyz[2] = (task == PDS_TASK_TAKEOFF) ? (double)0.0125f : 1.0;
  c->control_mode = PDS_CTRL_PWM;
  c->use_latency = 0;          // CrazyFlieSimpleAgent: use_latency=False (envs/agents.py:492)
  c->latency = 0.015;          // envs/base.py:40
  c->observation_frequency = 100;  // envs/base.py:42
  return PDS_OK;
}

/* Python's `a // b` for floats (Objects/floatobject.c float_divmod): NOT floor(a / b) -- 0.03 // 0.01 == 2.0
 * while 0.03 / 0.01 == 3.0 -- because the remainder is taken exactly (fmod) first. */
static double py_float_floordiv(double vx, double wx) {
  double mod = fmod(vx, wx);
  double div = (vx - mod) / wx;
  if (mod != 0 && ((wx < 0) != (mod < 0))) div -= 1.0;
  if (div == 0) return 0.0;
  double fl = floor(div);
  if (div - fl > 0.5) fl += 1.0;
  return fl;
}

// buf_size of the delayed-action ring: ctor form max(1, int(LATENCY // time_step)) (envs/agents.py:180),
// set_latency form int(latency / TIME_STEP) (envs/agents.py:401); 0 = no delay
static int latency_steps_ctor(double latency, double time_step) {
  if (!(latency >= time_step)) return 0;  // use_latency if latency >= time_step else False, agents.py:165
  const int b = (int)py_float_floordiv(latency, time_step);
  return b < 1 ? 1 : b;
}

static void set_latency_consts(Consts &k, int lat_steps, int agg) {
  k.lat_steps = lat_steps;
  k.lat_own1 = k.lat_own2 = 0;
  if (lat_steps > 0) {
    // the row action_buffer[-1] is rewritten by every lat_steps-th apply_action; after env.step s
    // (agg sub-steps each) it holds the action of step ceil(m / agg), m = floor(s agg / B) B (0: reset row)
    for (int s = 1; s <= 2; ++s) {
      const int m = (s * agg / lat_steps) * lat_steps;
      (s == 1 ? k.lat_own1 : k.lat_own2) = (m + agg - 1) / agg;
    }
  }
}

static void fill_consts(const pds_config &c, Consts &k) {
  // envs/assets/cf21x_sys_eq.urdf:10,16-17 and envs/agents.py:138-156
  const double M = 0.027, L = 0.0397, T2W = 2.25, IXX = 1.7e-5, IYY = 1.7e-5, IZZ = 2.9e-5;
  const double KF = 3.16e-10, GEC = 11.36859, PR = 2.31348e-2, FTF1 = 5.96e-3, G = 9.81;
  const double MAX_THRUST = G * M * T2W / 4;
  const double MAX_RPM = sqrt((T2W * G * M) / (4 * MAX_THRUST));
  memset(&k, 0, sizeof(k));
  k.K = (float)MAX_THRUST; k.G = (float)G; k.m = (float)M;
  k.Jx = (float)IXX; k.Jy = (float)IYY; k.Jz = (float)IZZ; k.ftf1 = (float)FTF1;
  k.Lq = (float)(L / sqrt(2.0));
  k.dt = (float)c.time_step;
  k.A = (float)(1.0 - c.time_step / c.motor_time_constant);
  k.hover_x = (float)sqrt(1 / T2W);
  k.hover_action = (float)(2 * 1 / T2W - 1);
  k.gec = (float)GEC; k.prop_r = (float)PR;
  k.h_clip = (float)(0.25 * PR * sqrt((15 * MAX_RPM * MAX_RPM * KF * GEC) / MAX_THRUST));
  k.t2w = (float)T2W; k.mtc = (float)c.motor_time_constant;
  k.M_nom = (float)M; k.Jx_nom = (float)IXX; k.Jy_nom = (float)IYY; k.Jz_nom = (float)IZZ;
  k.ftf1_nom = (float)FTF1; k.dt_nom = (float)c.time_step;
  k.pa = (float)c.penalty_action; k.pang = (float)c.penalty_angle; k.pspin = (float)c.penalty_spin;
  k.pterm = (float)c.penalty_terminal; k.pvel = (float)c.penalty_velocity; k.arp = (float)c.ARP;
  for (int i = 0; i < 3; ++i) {
    k.target[i] = (float)c.target_pos[i];
    k.init_xyz[i] = (float)c.init_xyz[i]; k.init_rpy[i] = (float)c.init_rpy[i];
    k.init_vel[i] = (float)c.init_xyz_dot[i]; k.init_w[i] = (float)c.init_rpy_dot[i];
  }
  k.dr = (float)(c.domain_randomization > 0 ? c.domain_randomization : 0.0);
  // OUNoise(sigma = 0.2 * motor_thrust_noise), envs/agents.py:206
  k.ou_sigma = (float)(0.2 * (c.motor_thrust_noise > 0 ? c.motor_thrust_noise : 0.0));
  // SensorNoise defaults, envs/sensors.py:14-23; gyro model envs/sensors.py:124-128 with
  // dt = 1/sim_freq (envs/hover.py:143)
  const double D2R = M_PI / 180.0, dt = c.time_step;
  k.pos_std = 0.002f; k.pos_unif = 0.001f; k.vel_std = 0.01f;
  k.q_std = (float)(0.1 * D2R); k.q_unif = (float)(0.05 * D2R);
  const double gnd = 0.000175, corr = 1000.0;
  const double sigma_g_d = gnd / sqrt(dt);
  k.gyro_sb = (float)sqrt(-(sigma_g_d * sigma_g_d) * (corr / 2) * (exp(-2 * dt / corr) - 1));
  k.gyro_pi = (float)exp(-dt / corr);
  k.gyro_rw = 0.0105f;
  k.gyro_to = (float)(5 * D2R);
  k.agg = c.aggregate_phy_steps; k.max_steps = c.max_episode_steps;
  k.reset_dist = c.enable_reset_distribution ? 1 : 0;
  k.ref_points = (c.task == PDS_TASK_CIRCLE) ? 3 * c.observation_frequency : kRefPoints;  // envs/circle.py:47-49
  {
    const double dth = 2.0 * M_PI / (double)k.ref_points;
    k.ref_dth_hi = (float)dth;
    k.ref_dth_lo = (float)(dth - (double)k.ref_dth_hi);
  }
  k.obs_rate = 1;
  if (c.observation_noise > 0) {  // obs_rate = sim_freq // observation_frequency, envs/base.py:108
    const int r = (int)llround(1.0 / c.time_step) / c.observation_frequency;
    k.obs_rate = r < 1 ? 1 : r;
  }
  set_latency_consts(k, c.use_latency ? latency_steps_ctor(c.latency, c.time_step) : 0, c.aggregate_phy_steps);
}

static int obs_dim_of(const pds_config &c) {
  const bool noisy = c.observation_noise > 0;
  const int o = noisy ? (c.task == PDS_TASK_HOVER ? 13 : (c.task == PDS_TASK_CIRCLE ? 16 : 20))
                      : (c.task == PDS_TASK_HOVER ? 17 : (c.task == PDS_TASK_CIRCLE ? 16 : 20));
  return 2 * (o + 4);
}

// DroneBaseEnv.__init__ evaluates compute_observation() once to size the observation space
// (envs/base.py:142): with sensor noise that advances the gyro bias random walk by one draw
// (envs/sensors.py:130-131) before the first reset, and the bias is never reset afterwards.
constexpr uint32_t kBlkCtor = 16;  // Philox block of tick 0 (oracle: PO_BLK_CTOR)
__global__ __launch_bounds__(256) void ctor_noise_kernel(DevState st, long long n, unsigned long long id_base, float gyro_sb,
                                                         uint32_t seed_lo, uint32_t seed_hi) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U4 r = philox4x32_7((uint32_t)(id_base + (unsigned long long)i), 0u, 0u, kBlkCtor, seed_lo, seed_hi);
  float z0, z1, z2, z3;
  box_muller_word(r.x, z0, z1);
  box_muller_word(r.y, z2, z3);
  st.nz0[i] = make_float4(gyro_sb * z0, gyro_sb * z1, gyro_sb * z2, 0.f);
}

#define PDS_CREATE_FAIL(code, ...)                                   \
  do {                                                               \
    snprintf(g_create_err, sizeof(g_create_err), __VA_ARGS__);       \
    return code;                                                     \
  } while (0)

static int ensure_latency_buffer(pds_handle *h) {
  if (h->lat_buf) return PDS_OK;
  const size_t bytes = (size_t)kMaxLatSteps * (size_t)h->cfg.num_envs * sizeof(float4);
  hipError_t e = hipMalloc((void **)&h->lat_buf, bytes);
  if (e == hipSuccess) e = hipMemset(h->lat_buf, 0, bytes);
  if (e != hipSuccess) {
    if (h->lat_buf) (void)hipFree(h->lat_buf);
    h->lat_buf = nullptr;
    return fail(h, e == hipErrorOutOfMemory ? PDS_ENOMEM : PDS_EHIP, "latency buffer (%zu bytes): %s", bytes, hipGetErrorString(e));
  }
  h->st.lat = h->lat_buf;
  return PDS_OK;
}

extern "C" int pds_create(const pds_config *cfg, pds_handle **out) {
  if (!cfg || !out) return PDS_EINVAL;
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(pds_config)) PDS_CREATE_FAIL(PDS_EINVAL, "pds_config size mismatch (built against another pds.h?)");
  if (cfg->task < 0 || cfg->task > 2 || cfg->num_envs < 1 || cfg->aggregate_phy_steps < 1 ||
      cfg->max_episode_steps < 1 || cfg->max_episode_steps > 65535 || cfg->time_step <= 0)
    PDS_CREATE_FAIL(PDS_EINVAL, "invalid pds_config (task, num_envs, aggregate_phy_steps, max_episode_steps or time_step)");
  if (cfg->num_envs > (1ll << 30)) PDS_CREATE_FAIL(PDS_EINVAL, "num_envs %lld exceeds 2^30 per handle", (long long)cfg->num_envs);
  // the Philox counter carries a 32-bit global env id
  if (cfg->env_id_base < 0 || cfg->env_id_base + cfg->num_envs > (1ll << 32))
    PDS_CREATE_FAIL(PDS_EINVAL, "env_id_base %lld + num_envs %lld leaves the 32-bit global env id range [0, 2^32)",
                    (long long)cfg->env_id_base, (long long)cfg->num_envs);
  if (cfg->device < 0) PDS_CREATE_FAIL(PDS_EINVAL, "device %d is negative", cfg->device);
  if (cfg->control_mode < 0 || cfg->control_mode > 2) PDS_CREATE_FAIL(PDS_EINVAL, "control_mode %d", cfg->control_mode);
  if (cfg->control_mode != PDS_CTRL_PWM && cfg->task == PDS_TASK_TAKEOFF)
    PDS_CREATE_FAIL(PDS_EUNSUPPORTED, "control_mode %d: the PID modes exist for Hover/Circle (TakeOff fixes control_mode PWM, envs/takeoff.py:225)", cfg->control_mode);
  if (cfg->control_mode != PDS_CTRL_PWM && cfg->use_ground_effect) {
    // round 5: PID + ground effect is built; not together with the latency ring or the Kalman hold
    const int sf = (int)llround(1.0 / cfg->time_step);
    const bool hold = cfg->observation_noise > 0 && cfg->observation_frequency > 0 && sf / cfg->observation_frequency != 1;
    if (cfg->use_latency || hold)
      PDS_CREATE_FAIL(PDS_EUNSUPPORTED, "control_mode %d with the ground-effect extension: not with use_latency or observation_frequency < sim_freq", cfg->control_mode);
  }
  if (cfg->observation_frequency < 1) PDS_CREATE_FAIL(PDS_EINVAL, "observation_frequency %d", cfg->observation_frequency);
  if (cfg->task == PDS_TASK_CIRCLE && 3 * cfg->observation_frequency > PDS_MAX_REF_POINTS)
    PDS_CREATE_FAIL(PDS_EUNSUPPORTED, "Circle with observation_frequency %d needs %d reference points (limit %d)",
                    cfg->observation_frequency, 3 * cfg->observation_frequency, PDS_MAX_REF_POINTS);
  if (cfg->observation_noise > 0) {
    // obs_rate = sim_freq // observation_frequency (envs/base.py:108)
    const int sim_freq = (int)llround(1.0 / cfg->time_step);
    const int obs_rate = sim_freq / cfg->observation_frequency;
    if (obs_rate < 1) PDS_CREATE_FAIL(PDS_EINVAL, "observation_frequency %d above sim_freq %d: obs_rate 0 (the reference divides by it)", cfg->observation_frequency, sim_freq);
  }
  // (observation noise with obs_rate > 1 -- the Kalman-hold branch -- together with a PID control mode or the latency
  //  ring: built since round 4)
  const int lat_steps = cfg->use_latency ? latency_steps_ctor(cfg->latency, cfg->time_step) : 0;
  if (lat_steps > kMaxLatSteps) PDS_CREATE_FAIL(PDS_EUNSUPPORTED, "latency %g s = %d steps (limit %d)", cfg->latency, lat_steps, kMaxLatSteps);
  // (use_latency + the ground-effect extension: built for control_mode PWM since round 3; the PID modes have no
  //  ground-effect instantiation at all, refused above)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device >= ndev)
    PDS_CREATE_FAIL(PDS_ENODEVICE, "no HIP device %d (found %d); there is no CPU fallback", cfg->device, ndev);
  pds_handle *h = new (std::nothrow) pds_handle();
  if (!h) return PDS_ENOMEM;
  memset((void *)h, 0, sizeof(*h));
  h->cfg = *cfg;
  fill_consts(*cfg, h->k);
  h->obs_dim = obs_dim_of(*cfg);
  h->flags.motor = cfg->use_motor_dynamics != 0;
  h->flags.dr = cfg->domain_randomization > 0;
  h->flags.ge = cfg->use_ground_effect != 0;
  h->flags.tn = cfg->motor_thrust_noise > 0;
  h->flags.on = cfg->observation_noise > 0;
  h->flags.ctrl = cfg->control_mode;
  h->flags.lat = lat_steps > 0;
  h->flags.hold = h->k.obs_rate != 1;
  h->flags.half_tile = false;
  if (const char *ft = getenv("PDS_FORCE_TILE")) h->force_tile = (ft[0] == 'h') ? 1 : ((ft[0] == 'f') ? 2 : 0);
  const size_t n = (size_t)cfg->num_envs;
  const size_t ntiles = (n + kWave - 1) / kWave;
  const LaunchFlags &f = h->flags;
  DeviceGuard guard(cfg->device);
  hipError_t e = guard.err;
  if (e == hipSuccess) {
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, cfg->device);
    h->num_cus = (e == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  {
    // State every other step (kCtrBehindBit) where a launch is more than one round of resident blocks, i.e. where it is bound
    // by what HBM takes: a launch of one round or less is bound by the latency of a single wave, and the extra pass through
    // the physics on the write steps shows (Hover 65 536: 7.22 against 7.10 us, profiles/state_every_other_step.txt).
    // PDS_STATE_EVERY_STEP=1: every step, =0: every other step at any size (tests / A-B runs).
    const size_t blocks = (n + kBlock - 1) / kBlock;
    h->store_every_step = blocks <= (size_t)kFullTileBlocksPerCU * (size_t)h->num_cus * (256 / kBlock);
    if (const char *es = getenv("PDS_STATE_EVERY_STEP")) h->store_every_step = es[0] == '1';
  }
  // All state arrays live in ONE slab (one allocation, one free, contiguous pages); consecutive arrays
  // are staggered by an odd multiple of 256 B so that the 6-21 concurrent streams of the step kernel do
  // not start at the same offset modulo a power of two (measured neutral on MI355X: 62.4-63.7 us for
  // staggers of 0 B ... 1 MiB, so this is hygiene, not a lever).
  std::vector<std::pair<void **, size_t>> req;
  auto alloc = [&](void **p, size_t bytes) { req.emplace_back(p, bytes); };
  alloc((void **)&h->st.s0, n * 16); alloc((void **)&h->st.s1, n * 16); alloc((void **)&h->st.s2, n * 16);
  alloc((void **)&h->st.hist[0], n * 16); alloc((void **)&h->st.hist[1], n * 16);
  alloc((void **)&h->st.ctr, n * 4);
  alloc((void **)&h->st.clk, ntiles * sizeof(WaveClock));
  alloc((void **)&h->d_count, 256);
  if (f.motor) alloc((void **)&h->st.mx, n * 16);
  if (f.dr) { alloc((void **)&h->st.par0, n * 16); alloc((void **)&h->st.par1, n * 8); }
  if (f.dr && f.motor) { alloc((void **)&h->st.mA, n * 16); alloc((void **)&h->st.mK, n * 16); }
  if (f.tn) alloc((void **)&h->st.ou, n * 16);
  if (f.on) {
    alloc((void **)&h->st.nz0, n * 16); alloc((void **)&h->st.nz1, n * 8);
    alloc((void **)&h->st.oh0, n * 16); alloc((void **)&h->st.oh1, n * 16); alloc((void **)&h->st.oh2, n * 8);
  }
  if (f.ctrl >= 1) { alloc((void **)&h->st.pid0, n * 16); alloc((void **)&h->st.pid1, n * 8); }
  if (f.ctrl == 2) { alloc((void **)&h->st.pid2, n * 16); alloc((void **)&h->st.pid3, n * 8); }
  alloc((void **)&h->d_circle_ref, kRefPoints * sizeof(float2));
  {
    const size_t stagger = (size_t)kStaggerBytes;
    size_t total = 0;
    std::vector<size_t> off;
    for (size_t j = 0; j < req.size(); ++j) {
      total = (total + 255) / 256 * 256 + stagger;
      off.push_back(total);
      total += req[j].second;
    }
    if (e == hipSuccess) e = hipMalloc(&h->slab, total + 256);
    if (e == hipSuccess) e = hipMemset(h->slab, 0, total + 256);  // tick 0, parity 0, OU / PID / stale-rate state 0
    if (e == hipSuccess)
      for (size_t j = 0; j < req.size(); ++j) *req[j].first = (char *)h->slab + off[j];
  }
  if (e == hipSuccess) {
    float2 ref[kRefPoints];  // envs/circle.py:45-56
    const int np = h->k.ref_points;
    for (int t = 0; t < kRefPoints; ++t) {
      const double ts = 2 * M_PI * (double)(t % np) / np;
      ref[t].x = (float)(0.25 * (1 - cos(ts)));
      ref[t].y = (float)(0.25 * sin(ts));
    }
    e = hipMemcpy(h->d_circle_ref, ref, sizeof(ref), hipMemcpyHostToDevice);
  }
  h->st.circle_ref = h->d_circle_ref;
  if (e == hipSuccess && h->flags.on) {
    hipLaunchKernelGGL(ctor_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, h->st, (long long)n,
                       (unsigned long long)cfg->env_id_base, h->k.gyro_sb, (uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32));
    e = hipGetLastError();
  }
  // The zero fill and the constructor draw ran on the null stream; the caller's stream may be a
  // non-blocking one that is not ordered behind it, so the state is made visible here, always.
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    snprintf(g_create_err, sizeof(g_create_err), "allocation of %zu envs failed: %s", n, hipGetErrorString(e));
    pds_destroy(h);
    return e == hipErrorOutOfMemory ? PDS_ENOMEM : PDS_EHIP;
  }
  if (h->flags.lat) {
    const int rc = ensure_latency_buffer(h);
    if (rc != PDS_OK) {
      snprintf(g_create_err, sizeof(g_create_err), "%s", h->err);
      pds_destroy(h);
      return rc;
    }
  }
  *out = h;
  return PDS_OK;
}

extern "C" int pds_destroy(pds_handle *h) {
  if (!h) return PDS_OK;
  DeviceGuard guard(h->cfg.device);
  if (h->slab) (void)hipFree(h->slab);
  if (h->lat_buf) (void)hipFree(h->lat_buf);
  if (h->d_stamps) (void)hipFree(h->d_stamps);
  if (h->eval_sink) (void)hipFree(h->eval_sink);
  delete h;
  return PDS_OK;
}

extern "C" int pds_obs_dim(const pds_handle *h) { return h ? h->obs_dim : PDS_EINVAL; }
extern "C" int64_t pds_num_envs(const pds_handle *h) { return h ? h->cfg.num_envs : PDS_EINVAL; }
extern "C" uint64_t pds_tick(const pds_handle *h) { return h ? h->tick : 0; }
extern "C" int pds_latency_steps(const pds_handle *h) { return h ? h->k.lat_steps : PDS_EINVAL; }
extern "C" const char *pds_last_error(const pds_handle *h) { return h ? h->err : g_create_err; }

extern "C" uint64_t pds_sync_tick(pds_handle *h, void *stream) {
  if (!h) return 0;
  DeviceGuard guard(h->cfg.device);
  WaveClock c;
  if (hipStreamSynchronize((hipStream_t)stream) == hipSuccess &&
      hipMemcpy(&c, h->st.clk, sizeof(c), hipMemcpyDeviceToHost) == hipSuccess)
    h->tick = ((uint64_t)c.y << 32) | c.x;
  return h->tick;
}

extern "C" int pds_set_tick(pds_handle *h, uint64_t tick) {
  if (!h) return PDS_EINVAL;
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  PDS_HIP(h, hipDeviceSynchronize());  // no stream argument: order behind everything in flight
  if (const int rc = materialize_kept_obs(h, 0)) return rc;  // (regenerated from the OLD tick's blocks)
  if (const int rc = materialize_state(h, 0)) return rc;     // (the new tick may change the phase of the state store)
  const long long ntiles = (h->cfg.num_envs + kWave - 1) / kWave;
  hipLaunchKernelGGL(clock_fill_kernel, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, 0, h->st.clk, ntiles,
                     (unsigned long long)tick, 1);
  PDS_HIP(h, hipGetLastError());
  PDS_HIP(h, hipDeviceSynchronize());
  h->tick = tick;
  return PDS_OK;
}

// CrazyFlieAgent.set_latency, envs/agents.py:388-404
extern "C" int pds_set_latency(pds_handle *h, double latency) {
  if (!h) return PDS_EINVAL;
  if (h->flags.ge && h->flags.ctrl != 0) return fail(h, PDS_EUNSUPPORTED, "use_latency with the ground-effect extension: control_mode PWM only");
  int steps = 0;
  if (!(latency < h->cfg.time_step)) {
    steps = (int)(latency / h->cfg.time_step);  // int(self.latency / self.TIME_STEP)
    if (steps < 1) return fail(h, PDS_EINVAL, "latency %g: buf_size 0 (the reference asserts buf_size > 0)", latency);
    if (steps > kMaxLatSteps) return fail(h, PDS_EUNSUPPORTED, "latency %g s = %d steps (limit %d)", latency, steps, kMaxLatSteps);
  }
  // every check and the allocation come BEFORE the handle is touched: a refused call leaves it as it was
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  PDS_HIP(h, hipDeviceSynchronize());
  if (steps > 0) {
    const int rc = ensure_latency_buffer(h);
    if (rc != PDS_OK) return rc;
  }
  if (const int rc = materialize_state(h, 0)) return rc;  // (the latency variants do not know kCtrBehindBit)
  h->cfg.latency = latency;
  h->cfg.use_latency = steps > 0;
  h->flags.lat = steps > 0;
  set_latency_consts(h->k, steps, h->cfg.aggregate_phy_steps);
  if (steps > 0) {
    const long long n = h->cfg.num_envs;
    hipLaunchKernelGGL(latency_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, h->st, n, kMaxLatSteps);
    PDS_HIP(h, hipGetLastError());
    PDS_HIP(h, hipDeviceSynchronize());
  }
  return PDS_OK;
}

// buf_size of a sim-opt candidate: CrazyFlieAgent.set_latency's float64 form (envs/agents.py:397-401)
extern "C" int pds_simopt_latency_steps(const pds_handle *h, double latency) {
  if (!h) return PDS_EINVAL;
  if (latency < h->cfg.time_step) return 0;  // (a NaN falls through like in the reference and gives 0 below)
  const double steps = latency / h->cfg.time_step;
  return steps >= 1.0 ? (steps > 1e6 ? 1000000 : (int)steps) : 0;
}

// ObjectiveFunctionPyBullet.evaluate for P candidates in one launch (csrc/pds_simopt.hip).  Reads the handle's configuration,
// changes nothing in it: every check comes first, then two launches on the caller's stream.
extern "C" int pds_simopt_evaluate(pds_handle *h, int64_t P, const float *d_params, const int32_t *d_lat_steps, int max_lat_steps,
                                   int64_t M, int T, int pre_steps, double gamma, const float *d_actions, const float *d_obs,
                                   const float *d_pre_inputs, float *d_loss, float *d_score, float *d_sim_obs, void *stream) {
  if (!h) return PDS_EINVAL;
  const LaunchFlags &f = h->flags;
  if (f.tn || f.on || f.dr || f.ge || f.hold || f.ctrl != 0)
    return fail(h, PDS_EUNSUPPORTED,
                "pds_simopt_evaluate is built for the deterministic objective: control_mode PWM, motor_thrust_noise <= 0, "
                "observation_noise <= 0, domain_randomization <= 0, no ground effect (this handle:%s%s%s%s%s)",
                f.ctrl != 0 ? " PID control mode" : "", f.tn ? " thrust noise" : "", f.on ? " observation noise" : "",
                f.dr ? " domain randomisation" : "", f.ge ? " ground effect" : "");
  if (max_lat_steps > kMaxLatSteps)
    return fail(h, PDS_EUNSUPPORTED, "a candidate's latency is %d time steps (limit %d): nothing was evaluated", max_lat_steps,
                kMaxLatSteps);
  if (P < 1 || M < 1 || T < 2 || pre_steps < 0 || max_lat_steps < 0)
    return fail(h, PDS_EINVAL, "pds_simopt_evaluate: P %lld, M %lld, T %d, pre_steps %d, max_lat_steps %d", (long long)P,
                (long long)M, T, pre_steps, max_lat_steps);
  if (M > (1 << 24) || P > (1 << 24) || P * ((M + kWave - 1) / kWave) > (int64_t)1 << 32)
    return fail(h, PDS_EINVAL, "pds_simopt_evaluate: P %lld x M %lld is beyond one launch: shard the candidates", (long long)P,
                (long long)M);
  if (!d_params || !d_lat_steps || !d_actions || !d_obs || !d_loss || !d_score || (pre_steps > 0 && !d_pre_inputs))
    return fail(h, PDS_EINVAL, "pds_simopt_evaluate: null pointer");
  if (((uintptr_t)d_actions | (uintptr_t)d_obs | (uintptr_t)d_pre_inputs) & 15u)
    return fail(h, PDS_EINVAL, "pds_simopt_evaluate: the data set arrays must be 16-byte aligned");
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  if (const int rc = materialize_state(h, (hipStream_t)stream)) return rc;
  SimoptArgs a;
  a.k = h->k;
  a.time_step = h->cfg.time_step;
  a.G = 9.81;  // envs/agents.py:150
  a.gamma = gamma;
  a.params = d_params;
  a.lat_steps = d_lat_steps;
  a.acts = reinterpret_cast<const float4 *>(d_actions);
  a.obs = reinterpret_cast<const float4 *>(d_obs);
  a.pre = reinterpret_cast<const float4 *>(d_pre_inputs);
  a.P = (int)P; a.M = (int)M; a.T = T; a.pre_steps = pre_steps;
  a.loss = d_loss; a.score = d_score; a.sim_obs = d_sim_obs;
  launch_simopt(a, (hipStream_t)stream);
  PDS_HIP(h, hipGetLastError());
  return PDS_OK;
}

// read action 16 + dyn state 48 + action history 32 + counter 4; write dyn state 48
// + newest history slot 16 + counter 4 + reward 4 + cost 4 + terminated 1 + truncated 1; obs 4*D;
// DR params +24; motor PT1: x R+W 32 (+ A, K 32 when randomised); OU state R+W 32; gyro bias +
// low-pass R+W 48; kept noisy observation (10 floats) R+W 80 only with the Kalman hold (obs_rate > 1) -- otherwise it is
// regenerated from the previous tick's Philox blocks, not kept (csrc/pds_reset.h regen_kept_obs; pds_step_with_variates
// and the first step after an explicit reset still move those 80 B); latency ring: one row R+W per physics
// sub-step.  (The per-tile clock word adds 0.5 B per env-step and is not counted.)
extern "C" int pds_bytes_per_env_step(const pds_handle *h) {
  if (!h) return PDS_EINVAL;
  int b = 100 + 78 + 4 * h->obs_dim;
  const LaunchFlags &f = h->flags;
  if (f.dr) b += 24;
  if (f.motor) b += 32;
  if (f.motor && f.dr) b += 32;
  if (f.tn) b += 32;
  if (f.on) b += 48 + (f.hold ? 80 : 0);
  if (f.ctrl >= 1) b += 48;  // rate-PID integral + last error, R+W
  if (f.ctrl == 2) b += 48;  // attitude-PID integral + last error, R+W
  if (f.lat) b += 32 * h->cfg.aggregate_phy_steps;
  return b;
}

// Whether pds_step_k is ONE launch for this handle (a step_k_kernel exists: step_k_rule, csrc/pds_types.h) or a loop of
// pds_step.  The single statement of that rule for pds_step_k, pds_bytes_per_env_step_k and the tests.
extern "C" int pds_step_k_fused(const pds_handle *h) {
  if (!h) return PDS_EINVAL;
  return step_k_supported(h->flags) ? 1 : 0;
}

// Algorithmic bytes per env-step of pds_step_k: the env state is read and written once per launch.
extern "C" int pds_bytes_per_env_step_k(const pds_handle *h, int k_steps) {
  if (!h || k_steps < 1) return PDS_EINVAL;
  const LaunchFlags &f = h->flags;
  const int full = pds_bytes_per_env_step(h);
  // where pds_step_k loops over pds_step (pds_step_k_fused: a PID mode with the ground effect or the Kalman hold) every step
  // moves the single-step kernel's bytes (rounds 2-5 priced those rows with the K-step formula: 0.26-0.36 "of their own
  // roofline" for what is pds_step at 0.57-0.86).  Elsewhere the PID integrals and previous errors (inside `full`) amortise
  // with the rest of the state.
  if (!pds_step_k_fused(h)) return full;
  const int stream = 16 + 4 * h->obs_dim + 10 + (f.lat ? 32 * h->cfg.aggregate_phy_steps : 0);
  // once per launch: the state read + written, both ring slots and the randomised parameters written back
  // (+ the kept noisy observation, which the K-step kernel reads from and leaves in oh0-2: materialize_oh_kernel)
  const int state = full - stream + 16 + (f.dr ? 24 : 0) + (f.dr && f.motor ? 32 : 0) + ((f.on && !f.hold) ? 80 : 0);
  return stream + (state + k_steps - 1) / k_steps;
}

static void base_args(pds_handle *h, StepArgs &a) {
  memset(&a, 0, sizeof(a));
  a.st = h->st;
  a.k = h->k;
  a.n = h->cfg.num_envs;
  a.env_id_base = (unsigned long long)h->cfg.env_id_base;
  a.seed_lo = (uint32_t)h->cfg.seed; a.seed_hi = (uint32_t)(h->cfg.seed >> 32);
  a.auto_reset = h->cfg.auto_reset;
  a.k_steps = 1;
  a.stamps = h->d_stamps;
}

static void launch_family(pds_handle *h, int kind, const LaunchFlags &lf, dim3 grid, hipStream_t s, const StepArgs &a) {
  const int task = h->cfg.task;
  const bool reset_kind = kind == kLaunchReset;
  if (lf.hold && !reset_kind) {  // (a reset observes at iteration 0: always a fresh observation)
    if (task == PDS_TASK_HOVER) launch_hover_hold(kind, lf, grid, s, a);
    else if (task == PDS_TASK_CIRCLE) launch_circle_hold(kind, lf, grid, s, a);
    else launch_takeoff_hold(kind, lf, grid, s, a);
  } else if (lf.lat) {
    if (task == PDS_TASK_HOVER) launch_hover_lat(kind, lf, grid, s, a);
    else if (task == PDS_TASK_CIRCLE) launch_circle_lat(kind, lf, grid, s, a);
    else launch_takeoff_lat(kind, lf, grid, s, a);
  } else if (lf.ctrl != 0 && !reset_kind) {
    if (lf.ge) {
      if (task == PDS_TASK_HOVER) launch_hover_pid_ge(kind, lf, grid, s, a);
      else launch_circle_pid_ge(kind, lf, grid, s, a);
    } else if (task == PDS_TASK_HOVER) launch_hover_pid(kind, lf, grid, s, a);
    else launch_circle_pid(kind, lf, grid, s, a);
  } else {
    if (task == PDS_TASK_HOVER) launch_hover(kind, lf, grid, s, a);
    else if (task == PDS_TASK_CIRCLE) launch_circle(kind, lf, grid, s, a);
    else launch_takeoff(kind, lf, grid, s, a);
  }
}

static int do_reset(pds_handle *h, const uint8_t *d_mask, const float *d_samples, float *d_obs, void *stream) {
  if (!h) return PDS_EINVAL;
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  // the envs outside a mask would keep what pds_evaluate_policies left: tiles that stopped at different steps
  if (d_mask != nullptr && h->after_evaluate)
    return fail(h, PDS_EINVAL, "pds_reset with a mask after pds_evaluate_policies: reset every env first (d_mask = NULL)");
  StepArgs a;
  base_args(h, a);
  a.mask = d_mask; a.samples = d_samples; a.obs = d_obs;
  const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock));
  if (d_mask != nullptr) {  // (the envs outside the mask keep their episode: see materialize_kept_obs, materialize_state)
    if (const int rc = materialize_kept_obs(h, (hipStream_t)stream)) return rc;
    if (const int rc = materialize_state(h, (hipStream_t)stream)) return rc;
  }
  launch_family(h, kLaunchReset, h->flags, grid, (hipStream_t)stream, a);
  PDS_HIP(h, hipGetLastError());
  h->tick += 1;
  h->was_reset = true;
  h->after_evaluate = false;
  if (d_mask == nullptr) h->state_maybe_behind = false;  // (every env's state and counter word are fresh)
  return PDS_OK;
}

extern "C" int pds_reset(pds_handle *h, const uint8_t *d_mask, float *d_obs, void *stream) {
  return do_reset(h, d_mask, nullptr, d_obs, stream);
}

extern "C" int pds_reset_from_samples(pds_handle *h, const uint8_t *d_mask, const float *d_samples,
                                      float *d_obs, void *stream) {
  if (h && !d_samples) return fail(h, PDS_EINVAL, "pds_reset_from_samples: d_samples is NULL");
  return do_reset(h, d_mask, d_samples, d_obs, stream);
}

static int check_step_pointers(pds_handle *h, const float *d_actions, float *d_obs, float *d_reward, uint8_t *d_terminated,
                               uint8_t *d_truncated, float *d_cost) {
  if (!d_actions || !d_obs || !d_reward || !d_terminated || !d_truncated || !d_cost)
    return fail(h, PDS_EINVAL, "pds_step: NULL tensor pointer");
  if (((uintptr_t)d_actions) & 15u) return fail(h, PDS_EINVAL, "pds_step: d_actions must be 16-byte aligned");
  if (((uintptr_t)d_obs) & 3u) return fail(h, PDS_EINVAL, "pds_step: d_obs must be 4-byte aligned (16 for full speed)");
  if (!h->was_reset) return fail(h, PDS_EINVAL, "pds_step before pds_reset");
  return PDS_OK;
}

extern "C" int pds_step_with_variates(pds_handle *h, const float *d_actions, const float *d_variates,
                                      float *d_obs, float *d_reward, uint8_t *d_terminated,
                                      uint8_t *d_truncated, float *d_cost, float *d_final_obs, void *stream) {
  if (!h) return PDS_EINVAL;
  if (const int rc = check_step_pointers(h, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_cost)) return rc;
  DeviceGuard guard(h->cfg.device);  // (no hipSetDevice when the caller is already on the device)
  PDS_HIP(h, guard.err);
  StepArgs a;
  base_args(h, a);
  a.actions = reinterpret_cast<const float4 *>(d_actions);
  a.obs = d_obs; a.reward = d_reward; a.term = d_terminated; a.trunc = d_truncated; a.cost = d_cost;
  a.final_obs = d_final_obs;
  a.noise = d_variates;
  // one 256-env block per 4 tiles
  const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock));
  // half observation tile (4 resident blocks per CU instead of 3) while the grid is between one and
  // about 2.7 rounds of the full-tile residency; see pds_types.h kHalfTileRows
  LaunchFlags lf = h->flags;
  // (variants that reset in registers on the full tile -- pds_step.h merged_reset_variant -- gain less
  // from the half tile: it wins up to 5 blocks per CU there, up to 8 for the others; profiles/r01_tile_rows.txt)
  const bool merged = !lf.on && !lf.lat && !(lf.motor && lf.dr) && h->cfg.task != PDS_TASK_TAKEOFF && h->cfg.auto_reset;
  const unsigned cus = (unsigned)h->num_cus;
  lf.half_tile = grid.x > (unsigned)kFullTileBlocksPerCU * cus * (256 / kBlock) && grid.x <= (merged ? 5u : 8u) * cus * (256 / kBlock);
  if (h->force_tile) lf.half_tile = h->force_tile == 1;
  if (lf.on || lf.lat) lf.half_tile = false;  // (no half-tile instantiation)
  launch_family(h, h->store_every_step ? kLaunchStepStoreAll : kLaunchStep, lf, grid, (hipStream_t)stream, a);
  PDS_HIP(h, hipGetLastError());
  if (skips_state(h)) {  // (see materialize_state)
    h->state_maybe_behind = true;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) (void)hipGetLastError();
    else if (cs != hipStreamCaptureStatusNone) h->step_captured = true;
  }
  h->tick += 1;
  return PDS_OK;
}

extern "C" int pds_step(pds_handle *h, const float *d_actions, float *d_obs, float *d_reward,
                        uint8_t *d_terminated, uint8_t *d_truncated, float *d_cost, float *d_final_obs,
                        void *stream) {
  return pds_step_with_variates(h, d_actions, nullptr, d_obs, d_reward, d_terminated, d_truncated, d_cost,
                                d_final_obs, stream);
}

extern "C" int pds_step_k(pds_handle *h, int k_steps, const float *d_actions, float *d_obs, float *d_reward,
                          uint8_t *d_terminated, uint8_t *d_truncated, float *d_cost, float *d_final_obs, void *stream) {
  if (!h) return PDS_EINVAL;
  if (k_steps < 1) return fail(h, PDS_EINVAL, "pds_step_k: k_steps %d", k_steps);
  if (const int rc = check_step_pointers(h, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_cost)) return rc;
  const long long n = h->cfg.num_envs;
  const int D = h->obs_dim;
  if (!pds_step_k_fused(h)) {
    // a PID mode with the ground effect or the Kalman hold (no K-step kernel): K single-step launches, same results
    for (int s = 0; s < k_steps; ++s) {
      const long long o1 = (long long)s * n;
      const int rc = pds_step(h, d_actions + o1 * 4, d_obs + o1 * D, d_reward + o1, d_terminated + o1, d_truncated + o1,
                              d_cost + o1, d_final_obs ? d_final_obs + o1 * D : nullptr, stream);
      if (rc != PDS_OK) return rc;
    }
    return PDS_OK;
  }
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  StepArgs a;
  base_args(h, a);
  a.actions = reinterpret_cast<const float4 *>(d_actions);
  a.obs = d_obs; a.reward = d_reward; a.term = d_terminated; a.trunc = d_truncated; a.cost = d_cost;
  a.final_obs = d_final_obs;
  a.k_steps = k_steps;
  const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock));
  LaunchFlags lf = h->flags;
  lf.half_tile = false;
  if (const int rc = materialize_kept_obs(h, (hipStream_t)stream)) return rc;  // (the K-step kernel reads oh0-2: StoredOh)
  if (const int rc = materialize_state(h, (hipStream_t)stream)) return rc;
  launch_family(h, kLaunchStepK, lf, grid, (hipStream_t)stream, a);
  PDS_HIP(h, hipGetLastError());
  h->tick += (uint64_t)k_steps;
  return PDS_OK;
}

extern "C" int pds_field_width(int field) {
  switch (field) {
    case PDS_F_POS: case PDS_F_RPY: case PDS_F_VEL: case PDS_F_OMEGA: case PDS_F_GYRO_BIAS: case PDS_F_GYRO_LPF: return 3;
    case PDS_F_QUAT: case PDS_F_MOTOR_X: case PDS_F_LAST_ACTION: case PDS_F_PREV_ACTION: case PDS_F_MOTOR_A:
    case PDS_F_MOTOR_K: case PDS_F_OU: return 4;
    case PDS_F_STEP_COUNT: case PDS_F_QUAT_SIGN: case PDS_F_REF_OFFSET: case PDS_F_ACTION_IDX: return 1;
    case PDS_F_PARAMS: return 6;
    case PDS_F_NOISY_OBS: return 10;
    case PDS_F_PID: return 12;
    case PDS_F_ACTION_BUFFER: return 4 * kMaxLatSteps;
    default: return PDS_EINVAL;
  }
}

// ---- the one-launch rollouts: pds_rollout (csrc/pds_rollout.h) and pds_rollout_history (csrc/pds_rollout_hist.h) ----
// What both validate about the call and the handle (`any_null`: one of the entry point's required pointers is NULL).
static int check_rollout_call(pds_handle *h, const char *fn, bool any_null, const float *d_mean, const float *d_std) {
  if (any_null) return fail(h, PDS_EINVAL, "%s: NULL pointer", fn);
  if ((d_mean == nullptr) != (d_std == nullptr)) return fail(h, PDS_EINVAL, "%s: mean and std come together", fn);
  if (!h->was_reset) return fail(h, PDS_EINVAL, "%s before pds_reset", fn);
  // the rollout bootstraps finished episodes from V(final_obs) and restarts them in place (roll_out of the reference
  // calls env.reset() itself, algs/iwpg/iwpg.py:382-385): without auto-reset there is no final observation to evaluate
  if (!h->cfg.auto_reset) return fail(h, PDS_EUNSUPPORTED, "%s needs a handle created with auto_reset = 1", fn);
  return PDS_OK;
}
// a network the rollout kernels can stage: d_in inputs, hidden layers <= 64, all six tensors there
static bool rollout_net_ok(const pds_mlp *m, int d_in) {
  return m->d_in == d_in && m->h1 >= 1 && m->h1 <= 64 && m->h2 >= 1 && m->h2 <= 64 && (m->activation == 0 || m->activation == 1) &&
         m->w1 && m->b1 && m->w2 && m->b2 && m->w3 && m->b3;
}
static bool rollout_buffers_aligned(const float *d_act_buf, const float *d_obs_buf) {
  return !((((uintptr_t)d_act_buf) & 15u) || (((uintptr_t)d_obs_buf) & 3u));
}
// The StepArgs head and the fields RolloutArgs, RolloutHistArgs and RolloutDeepArgs share (csrc/pds_types.h,
// csrc/pds_rollout_deep_args.h); reward / term / trunc / cost point at the [T, N] rollout buffers.  s.obs and what only one of the
// structs has are the caller's.  Net: the struct's actor, struct pds_mlp or struct pds_mlp_deep.
template <class RA, class Net>
static void fill_rollout_args(pds_handle *h, RA &ra, int T, const Net *pi, const float *d_mean, const float *d_std, float eps,
                              const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset,
                              int deterministic, float *d_act_buf, float *d_logp_buf, float *d_rew_buf, uint8_t *d_term_buf,
                              uint8_t *d_trunc_buf, float *d_cost_buf, float *d_ep_ret, float *d_ep_len, float *d_stats) {
  memset(&ra, 0, sizeof(ra));
  base_args(h, ra.s);
  ra.s.actions = reinterpret_cast<const float4 *>(d_act_buf);  // (load_env's action slot: valid memory, value unused)
  ra.s.reward = d_rew_buf; ra.s.term = d_term_buf; ra.s.trunc = d_trunc_buf; ra.s.cost = d_cost_buf;
  ra.s.final_obs = nullptr;                                     // (the finished rows stay in LDS)
  ra.s.k_steps = T;
  ra.pi = *pi;
  ra.mean = d_mean; ra.stdv = d_std; ra.eps = eps; ra.log_std = d_log_std;
  ra.seed = seed; ra.call_base = reinterpret_cast<const unsigned long long *>(d_call_base); ra.call_offset = call_offset;
  ra.deterministic = deterministic; ra.T = T;
  ra.act_buf = d_act_buf; ra.logp_buf = d_logp_buf;
  ra.ep_ret = d_ep_ret; ra.ep_len = d_ep_len; ra.stats = d_stats;
}
// The launch: `launch(grid, stream)` is the entry point's dispatch by task, grid.x the number of 64-env tiles; T ticks
// further.  Both entry points decide support BEFORE they get here: a refused call leaves the handle as it was.
template <class Launch>
static int launch_rollout(pds_handle *h, const char *fn, int T, void *stream, Launch launch) {
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  // the env waves read the kept noisy observation from oh0-2 (StoredOh, like the K-step kernel)
  if (const int rc = materialize_kept_obs(h, (hipStream_t)stream)) return rc;
  if (const int rc = materialize_state(h, (hipStream_t)stream)) return rc;
  const dim3 grid((unsigned)((h->cfg.num_envs + kWave - 1) / kWave));
  if (!launch(grid, (hipStream_t)stream)) return fail(h, PDS_EHIP, "%s: its _supported() rule and the launchers disagree", fn);
  PDS_HIP(h, hipGetLastError());
  h->tick += (uint64_t)T;
  return PDS_OK;
}

// One launch per rollout: csrc/pds_rollout.h (the caller's roll_out, algs/iwpg/iwpg.py:350-385).
extern "C" int pds_rollout(pds_handle *h, int T, const pds_mlp *pi, const pds_mlp *vf, const float *d_mean, const float *d_std,
                           float eps, const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset,
                           int deterministic, float *d_obs_buf, float *d_act_buf, float *d_logp_buf, float *d_val_buf,
                           float *d_rew_buf, uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fval_buf,
                           float *d_last_val, float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream) {
  if (!h) return PDS_EINVAL;
  if (T < 1) return fail(h, PDS_EINVAL, "pds_rollout: T %d", T);
  const bool any_null = !pi || !vf || !d_log_std || !d_obs_buf || !d_act_buf || !d_logp_buf || !d_val_buf || !d_rew_buf ||
                        !d_term_buf || !d_trunc_buf || !d_cost_buf || !d_fval_buf || !d_last_val || !d_ep_ret || !d_ep_len || !d_stats;
  if (const int rc = check_rollout_call(h, "pds_rollout", any_null, d_mean, d_std)) return rc;
  const int D = h->obs_dim;
  if (!rollout_net_ok(pi, D) || !rollout_net_ok(vf, D))
    return fail(h, PDS_EINVAL, "pds_rollout: network shape (d_in must be the observation width %d, hidden <= 64)", D);
  if (pi->d_out != 4 || vf->d_out != 1) return fail(h, PDS_EINVAL, "pds_rollout: actor d_out 4, critic d_out 1");
  if (!rollout_buffers_aligned(d_act_buf, d_obs_buf)) return fail(h, PDS_EINVAL, "pds_rollout: alignment");
  if (!rollout_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "pds_rollout: no kernel for this env configuration (not built: the ground effect except on TakeOff with control_mode PWM; the Kalman hold or "
                                     "partial noise settings together with a PID mode or the latency ring; TakeOff with motor dynamics "
                                     "without the latency ring) -- the per-step kernels give the same bits");
  RolloutArgs ra;
  fill_rollout_args(h, ra, T, pi, d_mean, d_std, eps, d_log_std, seed, d_call_base, call_offset, deterministic, d_act_buf, d_logp_buf,
                    d_rew_buf, d_term_buf, d_trunc_buf, d_cost_buf, d_ep_ret, d_ep_len, d_stats);
  ra.s.obs = d_obs_buf + (long long)h->cfg.num_envs * D;  // step t writes o(t + 1) into row t + 1
  ra.vf = *vf;
  ra.obs0 = d_obs_buf;
  ra.val_buf = d_val_buf; ra.fval_buf = d_fval_buf; ra.last_val = d_last_val;
  // (grid.x = the number of tiles: the launchers pick one or two tiles per block, csrc/pds_rollout.h)
  return launch_rollout(h, "pds_rollout", T, stream, [&](dim3 grid, hipStream_t s) {
    if (h->cfg.task == PDS_TASK_HOVER) return launch_rollout_hover(h->flags, grid, s, ra);
    if (h->cfg.task == PDS_TASK_CIRCLE) return launch_rollout_circle(h->flags, grid, s, ra);
    return launch_rollout_takeoff(h->flags, grid, s, ra);
  });
}

// One launch per rollout for observation histories other than 2: csrc/pds_rollout_hist.h.  ONE body for pds_rollout_history and
// pds_rollout_history_latency (include/pds_history_latency.h): the checks, the argument block and the launch; `latency`: the entry
// point that flies the latency ring (its own support rule and launchers) -- pds_rollout_history answers a latency handle as before.
static int rollout_history_call(pds_handle *h, const char *fn, bool latency, int T, int history, const pds_mlp *pi, const float *d_mean,
                                const float *d_std, float eps, const float *d_log_std, uint64_t seed, const uint64_t *d_call_base,
                                uint64_t call_offset, int deterministic, float *d_obs_buf, float *d_act_buf, float *d_logp_buf,
                                float *d_rew_buf, uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows,
                                int32_t *d_fin_step, int slots, float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream);
extern "C" int pds_rollout_history(pds_handle *h, int T, int history, const pds_mlp *pi, const float *d_mean, const float *d_std,
                                   float eps, const float *d_log_std, uint64_t seed, const uint64_t *d_call_base,
                                   uint64_t call_offset, int deterministic, float *d_obs_buf, float *d_act_buf,
                                   float *d_logp_buf, float *d_rew_buf, uint8_t *d_term_buf, uint8_t *d_trunc_buf,
                                   float *d_cost_buf, float *d_fin_rows, int32_t *d_fin_step, int slots, float *d_ep_ret,
                                   float *d_ep_len, float *d_stats, void *stream) {
  return rollout_history_call(h, "pds_rollout_history", false, T, history, pi, d_mean, d_std, eps, d_log_std, seed, d_call_base,
                              call_offset, deterministic, d_obs_buf, d_act_buf, d_logp_buf, d_rew_buf, d_term_buf, d_trunc_buf,
                              d_cost_buf, d_fin_rows, d_fin_step, slots, d_ep_ret, d_ep_len, d_stats, stream);
}
extern "C" int pds_rollout_history_latency_supported(const pds_handle *h, int history) {
  if (!h) return PDS_EINVAL;
  return h->cfg.auto_reset && rollout_hist_latency_supported(h->cfg.task, h->flags) && history >= 1 &&
                 (long long)history * (h->obs_dim / 2) <= 192 ? 1 : 0;
}
extern "C" int pds_rollout_history_latency(pds_handle *h, int T, int history, const pds_mlp *pi, const float *d_mean,
                                           const float *d_std, float eps, const float *d_log_std, uint64_t seed,
                                           const uint64_t *d_call_base, uint64_t call_offset, int deterministic, float *d_obs_buf,
                                           float *d_act_buf, float *d_logp_buf, float *d_rew_buf, uint8_t *d_term_buf,
                                           uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows, int32_t *d_fin_step, int slots,
                                           float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream) {
  return rollout_history_call(h, "pds_rollout_history_latency", true, T, history, pi, d_mean, d_std, eps, d_log_std, seed, d_call_base,
                              call_offset, deterministic, d_obs_buf, d_act_buf, d_logp_buf, d_rew_buf, d_term_buf, d_trunc_buf,
                              d_cost_buf, d_fin_rows, d_fin_step, slots, d_ep_ret, d_ep_len, d_stats, stream);
}
static int rollout_history_call(pds_handle *h, const char *fn, bool latency, int T, int history, const pds_mlp *pi, const float *d_mean,
                                const float *d_std, float eps, const float *d_log_std, uint64_t seed, const uint64_t *d_call_base,
                                uint64_t call_offset, int deterministic, float *d_obs_buf, float *d_act_buf, float *d_logp_buf,
                                float *d_rew_buf, uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows,
                                int32_t *d_fin_step, int slots, float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream) {
  if (!h) return PDS_EINVAL;
  if (T < 1 || history < 1 || slots < 1) return fail(h, PDS_EINVAL, "%s: T %d, history %d, slots %d", fn, T, history, slots);
  const bool any_null = !pi || !d_log_std || !d_obs_buf || !d_act_buf || !d_logp_buf || !d_rew_buf || !d_term_buf || !d_trunc_buf ||
                        !d_cost_buf || !d_fin_rows || !d_fin_step || !d_ep_ret || !d_ep_len || !d_stats;
  if (const int rc = check_rollout_call(h, fn, any_null, d_mean, d_std)) return rc;
  const int half = h->obs_dim / 2, HS = history * half;
  if (HS > 192) return fail(h, PDS_EUNSUPPORTED, "%s: %d x %d = %d network inputs (<= 192)", fn, history, half, HS);
  if (!rollout_net_ok(pi, HS) || pi->d_out != 4)
    return fail(h, PDS_EINVAL, "%s: actor shape (d_in must be history x half = %d, hidden <= 64, d_out 4)", fn, HS);
  // max_episode_steps bounds how often the TimeLimit can cut one env within T steps; + the rollout's last step
  if (slots < T / h->cfg.max_episode_steps + 2)
    return fail(h, PDS_EINVAL, "%s: slots %d < T / max_episode_steps + 2 = %d", fn, slots, T / h->cfg.max_episode_steps + 2);
  if (!rollout_buffers_aligned(d_act_buf, d_obs_buf)) return fail(h, PDS_EINVAL, "%s: alignment", fn);
  if (latency && !rollout_hist_latency_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "pds_rollout_history_latency: no kernel for this env configuration (built: Hover and Circle on the "
                                     "latency ring in every control mode, noise off or the reference's default; not TakeOff, the Kalman hold "
                                     "or the ground effect) -- the per-step kernels give the same bits");
  if (!latency && !rollout_hist_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "pds_rollout_history: no kernel for this env configuration (built: every control mode without latency ring, "
                                     "Kalman hold or ground effect; noise off or the reference's default; TakeOff without motor dynamics) "
                                     "-- the per-step kernels give the same bits");
  RolloutHistArgs ra;
  fill_rollout_args(h, ra, T, pi, d_mean, d_std, eps, d_log_std, seed, d_call_base, call_offset, deterministic, d_act_buf, d_logp_buf,
                    d_rew_buf, d_term_buf, d_trunc_buf, d_cost_buf, d_ep_ret, d_ep_len, d_stats);
  ra.s.obs = nullptr;  // (the kernel's own [o(k), o(k + 1)] row stays in LDS)
  ra.H = history; ra.half = half; ra.slots = slots;
  ra.obs_buf = d_obs_buf;
  ra.fin_rows = d_fin_rows; ra.fin_step = d_fin_step;
  const int hn = rollout_hist_tiles(HS);
  return launch_rollout(h, fn, T, stream, [&](dim3 grid, hipStream_t s) {
    if (latency) {  // (Hover or Circle: rollout_hist_latency_supported)
      const bool hover = h->cfg.task == PDS_TASK_HOVER;
      if (h->flags.ctrl != 0) return hover ? launch_rollout_hist_hover_pid_lat(h->flags, hn, grid, s, ra) : launch_rollout_hist_circle_pid_lat(h->flags, hn, grid, s, ra);
      return hover ? launch_rollout_hist_hover_lat(h->flags, hn, grid, s, ra) : launch_rollout_hist_circle_lat(h->flags, hn, grid, s, ra);
    }
    if (h->flags.ctrl != 0) {  // (TakeOff fixes control_mode PWM)
      if (h->cfg.task == PDS_TASK_HOVER) return launch_rollout_hist_hover_pid(h->flags, hn, grid, s, ra);
      return h->cfg.task == PDS_TASK_CIRCLE && launch_rollout_hist_circle_pid(h->flags, hn, grid, s, ra);
    }
    if (h->cfg.task == PDS_TASK_HOVER) return launch_rollout_hist_hover(h->flags, hn, grid, s, ra);
    if (h->cfg.task == PDS_TASK_CIRCLE) return launch_rollout_hist_circle(h->flags, hn, grid, s, ra);
    return launch_rollout_hist_takeoff(h->flags, hn, grid, s, ra);
  });
}

// The per-step streams of a kernel that keeps every step's outcome in registers (pds_evaluate_policies, pds_collect): step_once
// (csrc/pds_step.h) streams reward / cost / term / trunc out whatever its caller does with them, and those kernels point all four
// at one [N] sink row of the handle that every step overwrites.  16 N bytes, allocated by the first such call: load_env reads an
// action quad per env through StepArgs::actions (unused there); the outcome streams take 10 N of them.
static int point_at_step_sink(pds_handle *h, const char *fn, StepArgs &sa, void *stream) {
  const long long n = h->cfg.num_envs;
  if (!h->eval_sink) {
    if (hipMalloc(&h->eval_sink, (size_t)n * 16) != hipSuccess) {
      h->eval_sink = nullptr;
      (void)hipGetLastError();
      return fail(h, PDS_ENOMEM, "%s: %lld bytes for the per-step sink row", fn, n * 16);
    }
    PDS_HIP(h, hipMemsetAsync(h->eval_sink, 0, (size_t)n * 16, (hipStream_t)stream));  // (no uninitialised read in load_env)
  }
  sa.actions = reinterpret_cast<const float4 *>(h->eval_sink);  // (load_env's action slot: valid memory, value unused)
  sa.reward = reinterpret_cast<float *>(h->eval_sink);
  sa.cost = sa.reward + n;
  sa.term = reinterpret_cast<uint8_t *>(sa.cost + n);
  sa.trunc = sa.term + n;
  return PDS_OK;
}

// whether pds_evaluate_policies has a kernel for this handle (the two PDS_EUNSUPPORTED conditions of check_rollout_call and below)
extern "C" int pds_evaluate_supported(const pds_handle *h) {
  if (!h) return PDS_EINVAL;
  return h->cfg.auto_reset && rollout_supported(h->cfg.task, h->flags) ? 1 : 0;
}

// P policies x E episodes in one launch: csrc/pds_evaluate.h (the caller's evaluation loop, utils/evaluation.py:52-107).
// What every population evaluation validates about the call, in front of anything that touches the handle (`any_null`: one of the
// entry point's required pointers is NULL; `d_in`: the inputs the handle's observation gives the actors; d_metrics: checked where
// given).  The env configuration is the entry point's own question, behind these.
// (check_evaluate_population: everything but the network's shape -- pds_evaluate_policies_deep brings a struct pds_mlp_deep)
static int check_evaluate_population(pds_handle *h, const char *fn, bool any_null, int64_t P, int64_t episodes_per_policy,
                                     const float *d_mean, const float *d_std, int max_steps, const float *d_metrics) {
  if (max_steps < 1) return fail(h, PDS_EINVAL, "%s: max_steps %d", fn, max_steps);
  if (const int rc = check_rollout_call(h, fn, any_null, d_mean, d_std)) return rc;
  if (((uintptr_t)d_metrics) & 15u) return fail(h, PDS_EINVAL, "%s: d_metrics must be 16-byte aligned", fn);
  const long long n = h->cfg.num_envs;
  if (P < 1 || episodes_per_policy < 1 || episodes_per_policy > n || P > n || P * episodes_per_policy != n)
    return fail(h, PDS_EINVAL, "%s: P %lld x episodes_per_policy %lld is not the handle's %lld envs", fn, (long long)P,
                (long long)episodes_per_policy, n);
  if (episodes_per_policy % kWave != 0)
    return fail(h, PDS_EINVAL, "%s: episodes_per_policy %lld is not a multiple of %d (one tile)", fn, (long long)episodes_per_policy, kWave);
  return PDS_OK;
}
static int check_evaluate_call(pds_handle *h, const char *fn, bool any_null, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                               int d_in, const float *d_mean, const float *d_std, int max_steps, const float *d_metrics) {
  if (const int rc = check_evaluate_population(h, fn, any_null, P, episodes_per_policy, d_mean, d_std, max_steps, d_metrics)) return rc;
  if (shape->d_in != d_in || shape->h1 < 1 || shape->h1 > 64 || shape->h2 < 1 || shape->h2 > 64 || shape->d_out != 4 ||
      (shape->activation != 0 && shape->activation != 1))
    return fail(h, PDS_EINVAL, "%s: network shape (d_in must be the observation width %d, hidden <= 64, d_out 4, activation 0 or 1)", fn, d_in);
  return PDS_OK;
}
// the EvalArgs every form of the evaluation launches with; the per-step streams point at the handle's sink row
// (fill_evaluate_population_args: everything but the network's shape and its parameter count, as check_evaluate_population)
static int fill_evaluate_population_args(pds_handle *h, const char *fn, EvalArgs &ea, int64_t episodes_per_policy,
                                         const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                         const float *d_obs0, float *d_ret, float *d_len, float *d_cost, void *stream) {
  base_args(h, ea.s);
  if (const int rc = point_at_step_sink(h, fn, ea.s, stream)) return rc;
  ea.s.k_steps = max_steps;
  ea.params = d_params;
  ea.mean = d_mean; ea.stdv = d_std; ea.eps = eps;
  ea.tiles_per_policy = (int)(episodes_per_policy / kWave);
  ea.T = max_steps;
  ea.obs0 = d_obs0;
  ea.ret = d_ret; ea.len = d_len; ea.cost = d_cost;
  return PDS_OK;
}
static int fill_evaluate_args(pds_handle *h, const char *fn, EvalArgs &ea, int64_t episodes_per_policy, const pds_mlp *shape,
                              const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                              const float *d_obs0, float *d_ret, float *d_len, float *d_cost, void *stream) {
  if (const int rc = fill_evaluate_population_args(h, fn, ea, episodes_per_policy, d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret,
                                                   d_len, d_cost, stream))
    return rc;
  ea.shape = *shape;
  ea.param_count = pds_mlp_param_count(shape);
  return PDS_OK;
}
// ONE body for the four forms of pds_evaluate_policies (EvalForm, csrc/pds_evaluate_args.h): the checks, the argument block and the
// handle's state afterwards are stated once.  EvalFormCall holds what the forms add to the plain call; a form leaves what it does
// not take NULL / 0.  Metrics and Stats ask for d_metrics, Stats for d_obs_sums; the Record form's checks come first and its
// d_metrics is optional.
struct EvalFormCall {
  float *d_metrics, *d_obs_sums;
  int64_t record_per_policy;
  float *d_flight, *d_obs_rec;
};
// what a recording call validates about its record, in front of everything else (pds_evaluate_policies_record and
// pds_evaluate_policies_history_record)
static int check_record_call(pds_handle *h, const char *fn, const EvalFormCall &x, int64_t episodes_per_policy) {
  if (x.record_per_policy < kWave || x.record_per_policy % kWave != 0 || x.record_per_policy > episodes_per_policy)
    return fail(h, PDS_EINVAL, "%s: record_per_policy %lld is not a positive multiple of %d up to episodes_per_policy %lld", fn,
                (long long)x.record_per_policy, kWave, (long long)episodes_per_policy);
  if (!x.d_flight || (((uintptr_t)x.d_flight) & 15u)) return fail(h, PDS_EINVAL, "%s: d_flight must be given and 16-byte aligned", fn);
  if (((uintptr_t)x.d_obs_rec) & 3u) return fail(h, PDS_EINVAL, "%s: d_obs_rec must be 4-byte aligned", fn);
  return PDS_OK;
}
// ... and its part of the argument block
static void fill_record_args(EvalRecordArgs &ra, const EvalFormCall &x) {
  ra.flight = reinterpret_cast<float4 *>(x.d_flight);
  ra.obs_rec = x.d_obs_rec;
  ra.rec_tiles = (int)(x.record_per_policy / kWave);
}
template <EvalForm F>
static int evaluate_policies_call(pds_handle *h, const char *fn, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                  const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                  const float *d_obs0, float *d_ret, float *d_len, float *d_cost, const EvalFormCall &x, void *stream) {
  constexpr bool STATS = F == EvalForm::Stats, RECORD = F == EvalForm::Record;
  if (!h) return PDS_EINVAL;
  if constexpr (RECORD) {  // (decided before the handle is looked at)
    if (const int rc = check_record_call(h, fn, x, episodes_per_policy)) return rc;
  }
  const bool any_null = !shape || !d_params || !d_obs0 || !d_ret || !d_len || !d_cost ||
                        (eval_sums_metrics(F) && !RECORD && !x.d_metrics) || (STATS && !x.d_obs_sums);
  if (const int rc = check_evaluate_call(h, fn, any_null, P, episodes_per_policy, shape, h->obs_dim, d_mean, d_std, max_steps, x.d_metrics))
    return rc;
  if (STATS && (((uintptr_t)x.d_obs_sums) & 15u)) return fail(h, PDS_EINVAL, "%s: d_obs_sums must be 16-byte aligned", fn);
  if (!rollout_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: what pds_rollout is built for) -- "
                                     "pds_mlp_forward + pds_step give the same bits", fn);
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  EvalKernelArgs<F> ka;
  memset(&ka, 0, sizeof(ka));
  if constexpr (F == EvalForm::Metrics) ka.metrics = x.d_metrics;
  else if constexpr (eval_sums_metrics(F)) ka.m.metrics = x.d_metrics;
  if constexpr (STATS) ka.obs_sums = x.d_obs_sums;
  if constexpr (RECORD) fill_record_args(ka, x);
  if (const int rc = fill_evaluate_args(h, fn, eval_head(ka), episodes_per_policy, shape, d_params, d_mean, d_std, eps, max_steps, d_obs0,
                                        d_ret, d_len, d_cost, stream))
    return rc;
  const int rc = launch_rollout(h, fn, max_steps, stream, [&](dim3 grid, hipStream_t s) {
    if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hover<F>(h->flags, grid, s, ka);
    if (h->cfg.task == PDS_TASK_CIRCLE) return launch_evaluate_circle<F>(h->flags, grid, s, ka);
    return launch_evaluate_takeoff<F>(h->flags, grid, s, ka);
  });
  // tiles stopped at different steps: not a state to continue from -- every stepping entry point asks for pds_reset first
  if (rc == PDS_OK) { h->was_reset = false; h->after_evaluate = true; }
  return rc;
}
extern "C" int pds_evaluate_policies(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                     const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                     const float *d_obs0, float *d_ret, float *d_len, float *d_cost, void *stream) {
  return evaluate_policies_call<EvalForm::Plain>(h, "pds_evaluate_policies", P, episodes_per_policy, shape, d_params, d_mean, d_std, eps,
                                                 max_steps, d_obs0, d_ret, d_len, d_cost, {}, stream);
}
// the same launch with the PDS_EM_* flight metrics of every first episode in d_metrics [N, PDS_EVAL_METRICS]
extern "C" int pds_evaluate_policies_metrics(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                             const float *d_params, const float *d_mean, const float *d_std, float eps,
                                             int max_steps, const float *d_obs0, float *d_ret, float *d_len, float *d_cost,
                                             float *d_metrics, void *stream) {
  return evaluate_policies_call<EvalForm::Metrics>(h, "pds_evaluate_policies_metrics", P, episodes_per_policy, shape, d_params, d_mean,
                                                   d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost, {d_metrics}, stream);
}
// the metrics launch with the per-wave observation sums of every tile in d_obs_sums [tiles, 4, 2, 64] (include/pds.h)
extern "C" int pds_evaluate_policies_stats(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                           const float *d_params, const float *d_mean, const float *d_std, float eps,
                                           int max_steps, const float *d_obs0, float *d_ret, float *d_len, float *d_cost,
                                           float *d_metrics, float *d_obs_sums, void *stream) {
  return evaluate_policies_call<EvalForm::Stats>(h, "pds_evaluate_policies_stats", P, episodes_per_policy, shape, d_params, d_mean,
                                                 d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost, {d_metrics, d_obs_sums}, stream);
}
// the metrics launch (d_metrics optional) that also records the flights of the first record_per_policy envs of every policy:
// d_flight [T, 4, N_rec, 4] and, where given, d_obs_rec [T, N_rec, D] (include/pds.h; csrc/pds_evaluate.h, the record)
extern "C" int pds_evaluate_policies_record(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                            const float *d_params, const float *d_mean, const float *d_std, float eps,
                                            int max_steps, const float *d_obs0, float *d_ret, float *d_len, float *d_cost,
                                            float *d_metrics, int64_t record_per_policy, float *d_flight, float *d_obs_rec,
                                            void *stream) {
  return evaluate_policies_call<EvalForm::Record>(h, "pds_evaluate_policies_record", P, episodes_per_policy, shape, d_params, d_mean, d_std,
                                                  eps, max_steps, d_obs0, d_ret, d_len, d_cost,
                                                  {d_metrics, nullptr, record_per_policy, d_flight, d_obs_rec}, stream);
}

// ---- the population evaluation for actors with three or four hidden layers: csrc/pds_evaluate_deep.h ----
// a shape evaluate_deep_kernel can stage for a handle that observes d_in features; the struct's pointers are not looked at
static bool evaluate_deep_shape_ok(const pds_mlp_deep *m, int d_in) {
  if (m->n_hidden < 3 || m->n_hidden > PDS_MLP_DEEP_MAX_HIDDEN || m->d_in != d_in || d_in < 1 || d_in > 64 || m->d_out != 4 ||
      (m->activation != 0 && m->activation != 1))
    return false;
  for (int l = 0; l < m->n_hidden; ++l)
    if (m->hidden[l] < 1 || m->hidden[l] > 64) return false;
  return true;
}
// floats of one policy's row: W1 b1 .. W(L+1) b(L+1) (pds_mlp_deep_param_count, which also asks for the struct's pointers)
static int evaluate_deep_param_count(const pds_mlp_deep *m) {
  int total = 0, in = m->d_in;
  for (int l = 0; l <= m->n_hidden; ++l) {
    const int out = l < m->n_hidden ? m->hidden[l] : m->d_out;
    total += out * in + out;
    in = out;
  }
  return total;
}
// whether pds_evaluate_policies_deep has a kernel for this handle and this shape (include/pds_evaluate_deep.h)
extern "C" int pds_evaluate_deep_supported(const pds_handle *h, const pds_mlp_deep *shape) {
  if (!h || !shape) return PDS_EINVAL;
  const bool built = h->cfg.auto_reset && evaluate_deep_family(h->cfg.task, h->flags) && evaluate_deep_shape_ok(shape, h->obs_dim) &&
                     evaluate_deep_variant_built(h->cfg.task, h->flags, shape->n_hidden);
  return built ? 1 : 0;
}
// P policies x E episodes in one launch, the actors with three or four hidden layers: ONE body for the three forms of
// evaluate_deep_kernel (csrc/pds_evaluate_deep.h), as evaluate_policies_call is for evaluate_kernel's.  The checks and the handle's
// state afterwards are those of the form's two-hidden-layer entry point -- the record's own checks first, d_obs_sums given and
// aligned --; d_metrics is optional in every form (summed either way); the struct and the family are this kernel's questions.
template <EvalForm F>
static int evaluate_policies_deep_call(pds_handle *h, const char *fn, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                                       const float *d_params, const float *d_mean, const float *d_std, float eps, int32_t max_steps,
                                       const float *d_obs0, float *d_ret, float *d_len, float *d_cost, const EvalFormCall &x, void *stream) {
  constexpr bool STATS = F == EvalForm::Stats, RECORD = F == EvalForm::Record;
  if (!h) return PDS_EINVAL;
  if constexpr (RECORD) {  // (decided before the handle is looked at)
    if (const int rc = check_record_call(h, fn, x, episodes_per_policy)) return rc;
  }
  const bool any_null = !shape || !d_params || !d_obs0 || !d_ret || !d_len || !d_cost || (STATS && !x.d_obs_sums);
  if (const int rc = check_evaluate_population(h, fn, any_null, P, episodes_per_policy, d_mean, d_std, max_steps, x.d_metrics)) return rc;
  if (STATS && (((uintptr_t)x.d_obs_sums) & 15u)) return fail(h, PDS_EINVAL, "%s: d_obs_sums must be 16-byte aligned", fn);
  if (!evaluate_deep_shape_ok(shape, h->obs_dim))
    return fail(h, PDS_EINVAL, "%s: network shape (n_hidden 3 or 4, d_in must be the observation width %d, hidden 1..64, d_out 4, "
                               "activation 0 or 1)", fn, h->obs_dim);
  const bool built = F == EvalForm::Metrics ? evaluate_deep_variant_built(h->cfg.task, h->flags, shape->n_hidden)
                                            : evaluate_deep_forms_variant_built(h->cfg.task, h->flags, shape->n_hidden, F);
  if (!evaluate_deep_family(h->cfg.task, h->flags) || !built)
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: control_mode PWM without latency ring or Kalman "
                                     "hold, every noise setting; motor dynamics on Hover and Circle, the ground effect on TakeOff) -- "
                                     "pds_mlp_deep_forward + pds_step give the same bits", fn);
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  EvalDeepKernelArgs<F> ka;
  memset(&ka, 0, sizeof(ka));
  EvalMetricsArgs &head = eval_deep_head(ka);
  head.metrics = x.d_metrics;
  if constexpr (STATS) ka.st.obs_sums = x.d_obs_sums;
  if constexpr (RECORD) fill_record_args(ka.r, x);
  ka.deep = *shape;
  for (int l = 0; l <= PDS_MLP_DEEP_MAX_HIDDEN; ++l) ka.deep.w[l] = ka.deep.b[l] = nullptr;  // (the kernel lays them out per policy)
  ka.deep_param_count = evaluate_deep_param_count(shape);
  if (const int rc = fill_evaluate_population_args(h, fn, head.e, episodes_per_policy, d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret,
                                                   d_len, d_cost, stream))
    return rc;
  const bool l3 = shape->n_hidden == 3;
  const int task = h->cfg.task;
  const int rc = launch_rollout(h, fn, max_steps, stream, [&](dim3 grid, hipStream_t s) {
    if constexpr (STATS) {
      if (task == PDS_TASK_HOVER) return l3 ? launch_evaluate_stats_deep_hover_l3(h->flags, grid, s, ka) : launch_evaluate_stats_deep_hover_l4(h->flags, grid, s, ka);
      if (task == PDS_TASK_CIRCLE) return l3 ? launch_evaluate_stats_deep_circle_l3(h->flags, grid, s, ka) : launch_evaluate_stats_deep_circle_l4(h->flags, grid, s, ka);
      return l3 ? launch_evaluate_stats_deep_takeoff_l3(h->flags, grid, s, ka) : launch_evaluate_stats_deep_takeoff_l4(h->flags, grid, s, ka);
    } else if constexpr (RECORD) {
      if (task == PDS_TASK_HOVER) return l3 ? launch_evaluate_record_deep_hover_l3(h->flags, grid, s, ka) : launch_evaluate_record_deep_hover_l4(h->flags, grid, s, ka);
      if (task == PDS_TASK_CIRCLE) return l3 ? launch_evaluate_record_deep_circle_l3(h->flags, grid, s, ka) : launch_evaluate_record_deep_circle_l4(h->flags, grid, s, ka);
      return l3 ? launch_evaluate_record_deep_takeoff_l3(h->flags, grid, s, ka) : launch_evaluate_record_deep_takeoff_l4(h->flags, grid, s, ka);
    } else {
      if (task == PDS_TASK_HOVER) return l3 ? launch_evaluate_deep_hover_l3(h->flags, grid, s, ka) : launch_evaluate_deep_hover_l4(h->flags, grid, s, ka);
      if (task == PDS_TASK_CIRCLE) return l3 ? launch_evaluate_deep_circle_l3(h->flags, grid, s, ka) : launch_evaluate_deep_circle_l4(h->flags, grid, s, ka);
      return l3 ? launch_evaluate_deep_takeoff_l3(h->flags, grid, s, ka) : launch_evaluate_deep_takeoff_l4(h->flags, grid, s, ka);
    }
  });
  if (rc == PDS_OK) { h->was_reset = false; h->after_evaluate = true; }  // (tiles stopped at different steps: pds_evaluate_policies)
  return rc;
}
extern "C" int pds_evaluate_policies_deep(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                                          const float *d_params, const float *d_mean, const float *d_std, float eps, int32_t max_steps,
                                          const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                          void *stream) {
  return evaluate_policies_deep_call<EvalForm::Metrics>(h, "pds_evaluate_policies_deep", P, episodes_per_policy, shape, d_params, d_mean, d_std,
                                                        eps, max_steps, d_obs0, d_ret, d_len, d_cost, {d_metrics}, stream);
}
// ---- its stats and record forms: include/pds_evaluate_deep_forms.h ----
extern "C" int pds_evaluate_deep_forms_supported(const pds_handle *h, const pds_mlp_deep *shape, int32_t form) {
  if (!h || !shape || (form != PDS_EVALUATE_DEEP_FORM_STATS && form != PDS_EVALUATE_DEEP_FORM_RECORD)) return PDS_EINVAL;
  const bool built = h->cfg.auto_reset && evaluate_deep_family(h->cfg.task, h->flags) && evaluate_deep_shape_ok(shape, h->obs_dim) &&
                     evaluate_deep_forms_variant_built(h->cfg.task, h->flags, shape->n_hidden,
                                                       form == PDS_EVALUATE_DEEP_FORM_STATS ? EvalForm::Stats : EvalForm::Record);
  return built ? 1 : 0;
}
extern "C" int pds_evaluate_policies_deep_stats(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                                                const float *d_params, const float *d_mean, const float *d_std, float eps,
                                                int32_t max_steps, const float *d_obs0, float *d_ret, float *d_len, float *d_cost,
                                                float *d_metrics, float *d_obs_sums, void *stream) {
  return evaluate_policies_deep_call<EvalForm::Stats>(h, "pds_evaluate_policies_deep_stats", P, episodes_per_policy, shape, d_params, d_mean,
                                                      d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost, {d_metrics, d_obs_sums}, stream);
}
extern "C" int pds_evaluate_policies_deep_record(pds_handle *h, int64_t P, int64_t episodes_per_policy, const pds_mlp_deep *shape,
                                                 const float *d_params, const float *d_mean, const float *d_std, float eps,
                                                 int32_t max_steps, const float *d_obs0, float *d_ret, float *d_len, float *d_cost,
                                                 float *d_metrics, int64_t record_per_policy, float *d_flight, float *d_obs_rec,
                                                 void *stream) {
  return evaluate_policies_deep_call<EvalForm::Record>(h, "pds_evaluate_policies_deep_record", P, episodes_per_policy, shape, d_params, d_mean,
                                                       d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost,
                                                       {d_metrics, nullptr, record_per_policy, d_flight, d_obs_rec}, stream);
}

// ---- the one-launch rollout for actors with three or four hidden layers: csrc/pds_rollout_deep.h ----
// (an actor rollout_deep_kernel can stage is a shape evaluate_deep_kernel can: evaluate_deep_shape_ok)
// whether pds_rollout_deep has a kernel for this handle and this actor (include/pds_rollout_deep.h)
extern "C" int pds_rollout_deep_supported(const pds_handle *h, const pds_mlp_deep *pi) {
  if (!h || !pi) return PDS_EINVAL;
  const bool built = h->cfg.auto_reset && rollout_deep_family(h->cfg.task, h->flags) && evaluate_deep_shape_ok(pi, h->obs_dim) &&
                     rollout_deep_variant_built(h->cfg.task, h->flags, pi->n_hidden);
  return built ? 1 : 0;
}
// One launch per rollout, the actor with three or four hidden layers and the critic outside.  The checks are pds_rollout_history's.
extern "C" int pds_rollout_deep(pds_handle *h, int T, const pds_mlp_deep *pi, const float *d_mean, const float *d_std, float eps,
                                const float *d_log_std, uint64_t seed, const uint64_t *d_call_base, uint64_t call_offset,
                                int deterministic, float *d_obs_buf, float *d_act_buf, float *d_logp_buf, float *d_rew_buf,
                                uint8_t *d_term_buf, uint8_t *d_trunc_buf, float *d_cost_buf, float *d_fin_rows, int32_t *d_fin_step,
                                int slots, float *d_ep_ret, float *d_ep_len, float *d_stats, void *stream) {
  const char *fn = "pds_rollout_deep";
  if (!h) return PDS_EINVAL;
  if (T < 1 || slots < 1) return fail(h, PDS_EINVAL, "%s: T %d, slots %d", fn, T, slots);
  const bool any_null = !pi || !d_log_std || !d_obs_buf || !d_act_buf || !d_logp_buf || !d_rew_buf || !d_term_buf || !d_trunc_buf ||
                        !d_cost_buf || !d_fin_rows || !d_fin_step || !d_ep_ret || !d_ep_len || !d_stats;
  if (const int rc = check_rollout_call(h, fn, any_null, d_mean, d_std)) return rc;
  const int D = h->obs_dim;
  bool tensors = true;
  for (int l = 0; l <= pi->n_hidden && l <= PDS_MLP_DEEP_MAX_HIDDEN; ++l) tensors = tensors && pi->w[l] && pi->b[l];
  if (!evaluate_deep_shape_ok(pi, D) || !tensors)
    return fail(h, PDS_EINVAL, "%s: actor shape (n_hidden 3 or 4, d_in must be the observation width %d, hidden 1..64, d_out 4, "
                               "activation 0 or 1, all 2 (n_hidden + 1) tensors)", fn, D);
  // max_episode_steps bounds how often the TimeLimit can cut one env within T steps; + the rollout's last step
  if (slots < T / h->cfg.max_episode_steps + 2)
    return fail(h, PDS_EINVAL, "%s: slots %d < T / max_episode_steps + 2 = %d", fn, slots, T / h->cfg.max_episode_steps + 2);
  if (!rollout_buffers_aligned(d_act_buf, d_obs_buf)) return fail(h, PDS_EINVAL, "%s: alignment", fn);
  if (!rollout_deep_family(h->cfg.task, h->flags) || !rollout_deep_variant_built(h->cfg.task, h->flags, pi->n_hidden))
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: control_mode PWM without latency ring or Kalman "
                                     "hold, every noise setting; motor dynamics on Hover and Circle, the ground effect on TakeOff) -- "
                                     "the per-step kernels give the same bits", fn);
  RolloutDeepArgs ra;
  fill_rollout_args(h, ra, T, pi, d_mean, d_std, eps, d_log_std, seed, d_call_base, call_offset, deterministic, d_act_buf, d_logp_buf,
                    d_rew_buf, d_term_buf, d_trunc_buf, d_cost_buf, d_ep_ret, d_ep_len, d_stats);
  ra.s.obs = d_obs_buf + (long long)h->cfg.num_envs * D;  // step t writes o(t + 1) into row t + 1
  ra.obs0 = d_obs_buf;
  ra.slots = slots;
  ra.fin_rows = d_fin_rows; ra.fin_step = d_fin_step;
  const bool l3 = pi->n_hidden == 3;
  return launch_rollout(h, fn, T, stream, [&](dim3 grid, hipStream_t s) {
    if (h->cfg.task == PDS_TASK_HOVER) return l3 ? launch_rollout_deep_hover_l3(h->flags, grid, s, ra) : launch_rollout_deep_hover_l4(h->flags, grid, s, ra);
    if (h->cfg.task == PDS_TASK_CIRCLE) return l3 ? launch_rollout_deep_circle_l3(h->flags, grid, s, ra) : launch_rollout_deep_circle_l4(h->flags, grid, s, ra);
    return l3 ? launch_rollout_deep_takeoff_l3(h->flags, grid, s, ra) : launch_rollout_deep_takeoff_l4(h->flags, grid, s, ra);
  });
}

// ---- the population evaluation for observation histories: csrc/pds_evaluate_hist.h ----
// whether pds_evaluate_policies_history and pds_evaluate_policies_history_record (the same variant set) have a kernel for this
// handle and this observation_history_size
extern "C" int pds_evaluate_history_supported(const pds_handle *h, int history) {
  if (!h) return PDS_EINVAL;
  return h->cfg.auto_reset && rollout_hist_supported(h->cfg.task, h->flags) && history >= 1 && (long long)history * (h->obs_dim / 2) <= 192 ? 1 : 0;
}
// ... and whether pds_evaluate_policies_history_stats has: the same question, and the stats form built for the input width
extern "C" int pds_evaluate_history_stats_supported(const pds_handle *h, int history) {
  const int rc = pds_evaluate_history_supported(h, history);
  if (rc != 1) return rc;
  return eval_hist_stats_width_built(rollout_hist_tiles(history * (h->obs_dim / 2))) ? 1 : 0;
}
// P policies x E episodes in one launch, the actors reading the last `history` halves of the handle's row.  The checks and the
// handle's state afterwards are pds_evaluate_policies'; d_metrics is optional.  ONE body for the three forms of the kernel
// (EvalHistForm, csrc/pds_evaluate_hist.h): the record form's checks come first, as in evaluate_policies_call, the stats form's
// behind those of the plain call, and `x` holds what a form adds.  `latency`: the entry points of
// include/pds_history_latency_evaluate.h, which fly the latency ring (their own support rule and launchers, as in
// rollout_history_call) -- the others answer a ring handle as before.
template <EvalHistForm F>
static int evaluate_history_call(pds_handle *h, const char *fn, bool latency, int history, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                 const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                 const float *d_obs0, float *d_ret, float *d_len, float *d_cost, const EvalFormCall &x, void *stream) {
  constexpr bool REC = F == EvalHistForm::Record, STATS = F == EvalHistForm::Stats;
  float *const d_metrics = x.d_metrics;
  if (!h) return PDS_EINVAL;
  if constexpr (REC) {  // (decided before the handle is looked at)
    if (const int rc = check_record_call(h, fn, x, episodes_per_policy)) return rc;
  }
  if (history < 1) return fail(h, PDS_EINVAL, "%s: history %d", fn, history);
  const bool any_null = !shape || !d_params || !d_obs0 || !d_ret || !d_len || !d_cost;
  const int half = h->obs_dim / 2;
  const long long HS = (long long)history * half;
  if (HS > 192) return fail(h, PDS_EUNSUPPORTED, "%s: %d x %d = %lld network inputs (<= 192)", fn, history, half, HS);
  if (const int rc = check_evaluate_call(h, fn, any_null, P, episodes_per_policy, shape, (int)HS, d_mean, d_std, max_steps, d_metrics))
    return rc;
  if (latency && !rollout_hist_latency_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: what pds_rollout_history_latency is built for) -- "
                                     "pds_mlp_forward + pds_step + pds_history_advance_latency give the same bits", fn);
  if (!latency && !rollout_hist_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: what pds_rollout_history is built for) -- "
                                     "pds_mlp_forward + pds_step + pds_history_advance give the same bits", fn);
  const int hn = rollout_hist_tiles((int)HS);
  if constexpr (STATS) {
    if (!x.d_obs_sums || (((uintptr_t)x.d_obs_sums) & 15u)) return fail(h, PDS_EINVAL, "%s: d_obs_sums must be given and 16-byte aligned", fn);
    if (!eval_hist_stats_width_built(hn))
      return fail(h, PDS_EUNSUPPORTED, "%s: the stats form is not built for %lld network inputs (%d input tiles) -- "
                                       "pds_mlp_forward + pds_step + pds_history_advance give the same bits", fn, HS, hn);
  }
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  EvalHistKernelArgs<F> ka;
  memset(&ka, 0, sizeof(ka));
  if constexpr (REC) {
    ka.r.m.metrics = d_metrics;
    fill_record_args(ka.r, x);
  } else if constexpr (STATS) {
    ka.st.m.metrics = d_metrics;
    ka.st.obs_sums = x.d_obs_sums;
  } else {
    ka.m.metrics = d_metrics;
  }
  ka.H = history;
  if (const int rc = fill_evaluate_args(h, fn, eval_head(ka), episodes_per_policy, shape, d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret,
                                        d_len, d_cost, stream))
    return rc;
  const int rc = launch_rollout(h, fn, max_steps, stream, [&](dim3 grid, hipStream_t s) {
    if (latency) {  // (Hover or Circle: rollout_hist_latency_supported)
      const bool hover = h->cfg.task == PDS_TASK_HOVER, pid = h->flags.ctrl != 0;
      if constexpr (STATS) {
        if (pid) return hover ? launch_evaluate_hist_stats_hover_pid_lat(h->flags, hn, grid, s, ka) : launch_evaluate_hist_stats_circle_pid_lat(h->flags, hn, grid, s, ka);
        return hover ? launch_evaluate_hist_stats_hover_lat(h->flags, hn, grid, s, ka) : launch_evaluate_hist_stats_circle_lat(h->flags, hn, grid, s, ka);
      } else if constexpr (REC) {
        if (pid) return hover ? launch_evaluate_hist_record_hover_pid_lat(h->flags, hn, grid, s, ka) : launch_evaluate_hist_record_circle_pid_lat(h->flags, hn, grid, s, ka);
        return hover ? launch_evaluate_hist_record_hover_lat(h->flags, hn, grid, s, ka) : launch_evaluate_hist_record_circle_lat(h->flags, hn, grid, s, ka);
      } else {
        if (pid) return hover ? launch_evaluate_hist_hover_pid_lat(h->flags, hn, grid, s, ka) : launch_evaluate_hist_circle_pid_lat(h->flags, hn, grid, s, ka);
        return hover ? launch_evaluate_hist_hover_lat(h->flags, hn, grid, s, ka) : launch_evaluate_hist_circle_lat(h->flags, hn, grid, s, ka);
      }
    }
    if constexpr (STATS) {
      if (h->flags.ctrl != 0) {  // (TakeOff fixes control_mode PWM)
        if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hist_stats_hover_pid(h->flags, hn, grid, s, ka);
        return h->cfg.task == PDS_TASK_CIRCLE && launch_evaluate_hist_stats_circle_pid(h->flags, hn, grid, s, ka);
      }
      if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hist_stats_hover(h->flags, hn, grid, s, ka);
      if (h->cfg.task == PDS_TASK_CIRCLE) return launch_evaluate_hist_stats_circle(h->flags, hn, grid, s, ka);
      return launch_evaluate_hist_stats_takeoff(h->flags, hn, grid, s, ka);
    } else if constexpr (REC) {
      if (h->flags.ctrl != 0) {  // (TakeOff fixes control_mode PWM)
        if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hist_record_hover_pid(h->flags, hn, grid, s, ka);
        return h->cfg.task == PDS_TASK_CIRCLE && launch_evaluate_hist_record_circle_pid(h->flags, hn, grid, s, ka);
      }
      if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hist_record_hover(h->flags, hn, grid, s, ka);
      if (h->cfg.task == PDS_TASK_CIRCLE) return launch_evaluate_hist_record_circle(h->flags, hn, grid, s, ka);
      return launch_evaluate_hist_record_takeoff(h->flags, hn, grid, s, ka);
    } else {
      if (h->flags.ctrl != 0) {  // (TakeOff fixes control_mode PWM)
        if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hist_hover_pid(h->flags, hn, grid, s, ka);
        return h->cfg.task == PDS_TASK_CIRCLE && launch_evaluate_hist_circle_pid(h->flags, hn, grid, s, ka);
      }
      if (h->cfg.task == PDS_TASK_HOVER) return launch_evaluate_hist_hover(h->flags, hn, grid, s, ka);
      if (h->cfg.task == PDS_TASK_CIRCLE) return launch_evaluate_hist_circle(h->flags, hn, grid, s, ka);
      return launch_evaluate_hist_takeoff(h->flags, hn, grid, s, ka);
    }
  });
  if (rc == PDS_OK) { h->was_reset = false; h->after_evaluate = true; }  // (tiles stopped at different steps: pds_evaluate_policies)
  return rc;
}
extern "C" int pds_evaluate_policies_history(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy, const pds_mlp *shape,
                                             const float *d_params, const float *d_mean, const float *d_std, float eps, int max_steps,
                                             const float *d_obs0, float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                             void *stream) {
  return evaluate_history_call<EvalHistForm::Metrics>(h, "pds_evaluate_policies_history", false, history, P, episodes_per_policy, shape, d_params, d_mean,
                                      d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost, {d_metrics}, stream);
}
// the same launch that also records the flights of the first record_per_policy envs of every policy: d_flight [T, 4, N_rec, 4] and,
// where given, d_obs_rec [T, N_rec, history x half] (include/pds_history_record.h; csrc/pds_evaluate_hist.h, the record)
extern "C" int pds_evaluate_policies_history_record(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                    const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                    const float *d_std, float eps, int max_steps, const float *d_obs0, float *d_ret,
                                                    float *d_len, float *d_cost, float *d_metrics, int64_t record_per_policy,
                                                    float *d_flight, float *d_obs_rec, void *stream) {
  return evaluate_history_call<EvalHistForm::Record>(h, "pds_evaluate_policies_history_record", false, history, P, episodes_per_policy, shape, d_params,
                                     d_mean, d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost,
                                     {d_metrics, nullptr, record_per_policy, d_flight, d_obs_rec}, stream);
}
// the same launch that also sums the histories the policies acted on: d_obs_sums [tiles, 4, 2, 16 hn] (include/pds_history_stats.h;
// csrc/pds_evaluate_hist.h, the observation sums)
extern "C" int pds_evaluate_policies_history_stats(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                   const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                   const float *d_std, float eps, int max_steps, const float *d_obs0, float *d_ret,
                                                   float *d_len, float *d_cost, float *d_metrics, float *d_obs_sums, void *stream) {
  return evaluate_history_call<EvalHistForm::Stats>(h, "pds_evaluate_policies_history_stats", false, history, P, episodes_per_policy, shape,
                                                    d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost,
                                                    {d_metrics, d_obs_sums}, stream);
}
// ... and on the latency ring (include/pds_history_latency_evaluate.h): the same three calls with `latency` set
extern "C" int pds_evaluate_history_latency_supported(const pds_handle *h, int history) {
  if (!h) return PDS_EINVAL;
  return h->cfg.auto_reset && rollout_hist_latency_supported(h->cfg.task, h->flags) && history >= 1 &&
                 (long long)history * (h->obs_dim / 2) <= 192 ? 1 : 0;
}
extern "C" int pds_evaluate_history_latency_stats_supported(const pds_handle *h, int history) {
  const int rc = pds_evaluate_history_latency_supported(h, history);
  if (rc != 1) return rc;
  return eval_hist_stats_width_built(rollout_hist_tiles(history * (h->obs_dim / 2))) ? 1 : 0;
}
extern "C" int pds_evaluate_policies_history_latency(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                     const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                     const float *d_std, float eps, int max_steps, const float *d_obs0, float *d_ret,
                                                     float *d_len, float *d_cost, float *d_metrics, void *stream) {
  return evaluate_history_call<EvalHistForm::Metrics>(h, "pds_evaluate_policies_history_latency", true, history, P, episodes_per_policy, shape,
                                                      d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost, {d_metrics}, stream);
}
extern "C" int pds_evaluate_policies_history_latency_record(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                            const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                            const float *d_std, float eps, int max_steps, const float *d_obs0,
                                                            float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                                            int64_t record_per_policy, float *d_flight, float *d_obs_rec, void *stream) {
  return evaluate_history_call<EvalHistForm::Record>(h, "pds_evaluate_policies_history_latency_record", true, history, P, episodes_per_policy,
                                                     shape, d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost,
                                                     {d_metrics, nullptr, record_per_policy, d_flight, d_obs_rec}, stream);
}
extern "C" int pds_evaluate_policies_history_latency_stats(pds_handle *h, int history, int64_t P, int64_t episodes_per_policy,
                                                           const pds_mlp *shape, const float *d_params, const float *d_mean,
                                                           const float *d_std, float eps, int max_steps, const float *d_obs0,
                                                           float *d_ret, float *d_len, float *d_cost, float *d_metrics,
                                                           float *d_obs_sums, void *stream) {
  return evaluate_history_call<EvalHistForm::Stats>(h, "pds_evaluate_policies_history_latency_stats", true, history, P, episodes_per_policy,
                                                    shape, d_params, d_mean, d_std, eps, max_steps, d_obs0, d_ret, d_len, d_cost,
                                                    {d_metrics, d_obs_sums}, stream);
}

// ---- the fused off-policy collection: csrc/pds_collect.h (OffPolicyTrainer.step_env + the bookkeeping of learn_one_epoch) ----
// what pds_collect refuses with PDS_EUNSUPPORTED, as a question: the handle (auto_reset, collect_env_supported) and the actor's shape
static bool collect_shape_ok(const pds_handle *h, const pds_mlp *pi) {
  return pi->d_in == h->obs_dim && h->obs_dim <= 64 && pi->h1 >= 1 && pi->h1 <= 64 && pi->h2 >= 1 && pi->h2 <= 64 &&
         (pi->activation == 0 || pi->activation == 1);
}
extern "C" int pds_collect_supported(const pds_handle *h, const pds_mlp *pi, int mode) {
  if (!h || !pi) return PDS_EINVAL;
  if (mode != kCollectDdpg && mode != kCollectSac) return 0;
  return h->cfg.auto_reset && collect_env_supported(h->cfg.task, h->flags) && collect_shape_ok(h, pi) &&
                 pi->d_out == (mode == kCollectSac ? 8 : 4) ? 1 : 0;
}

// what pds_collect_control flies: what pds_collect flies, and the PID control modes / the latency ring on Hover and Circle
static bool collect_control_handle_ok(const pds_handle *h) {
  return collect_env_supported(h->cfg.task, h->flags) || collect_control_env_supported(h->cfg.task, h->flags);
}
extern "C" int pds_collect_control_supported(const pds_handle *h, const pds_mlp *pi, int mode) {
  if (!h || !pi) return PDS_EINVAL;
  if (mode != kCollectDdpg && mode != kCollectSac) return 0;
  return h->cfg.auto_reset && collect_control_handle_ok(h) && collect_shape_ok(h, pi) &&
                 pi->d_out == (mode == kCollectSac ? 8 : 4) ? 1 : 0;
}

// ONE body for pds_collect and pds_collect_control (include/pds_collect_control.h): the checks, the argument block and the handle's
// state afterwards are stated once; `control` admits the env configurations of collect_control_env_supported beside pds_collect's.
static int collect_call(pds_handle *h, const char *fn, bool control, int K, int mode, const pds_mlp *pi, float act_limit,
                        const float *d_log_std, uint64_t seed, uint64_t first_call, float *d_oa, float *d_obs2, float *d_rew,
                        float *d_done, int64_t capacity, int64_t ptr, float *d_obs, float *d_ep_ret, float *d_ep_len,
                        float *d_tile_stats, void *stream) {
  if (!h) return PDS_EINVAL;
  if (K < 1) return fail(h, PDS_EINVAL, "%s: K %d", fn, K);
  if (mode != kCollectDdpg && mode != kCollectSac) return fail(h, PDS_EINVAL, "%s: mode %d (0 DDPG, 1 SAC)", fn, mode);
  const bool any_null = !pi || (mode == kCollectDdpg && !d_log_std) || !d_oa || !d_obs2 || !d_rew || !d_done || !d_obs || !d_ep_ret ||
                        !d_ep_len || !d_tile_stats;
  if (const int rc = check_rollout_call(h, fn, any_null, nullptr, nullptr)) return rc;
  const bool plain = collect_env_supported(h->cfg.task, h->flags);
  if (!plain && !control)
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: control_mode PWM without latency ring, Kalman hold "
                                     "or ground effect; noise off or the reference's default; TakeOff without motor dynamics) -- the "
                                     "per-step entry points give the same bits", fn);
  if (!plain && !collect_control_env_supported(h->cfg.task, h->flags))
    return fail(h, PDS_EUNSUPPORTED, "%s: no kernel for this env configuration (built: what pds_collect flies, and Hover and Circle under "
                                     "AttitudeRate / Attitude and / or with the latency ring; not built: Kalman hold, ground effect, "
                                     "noise settings other than off or the reference's default, TakeOff with the latency ring or "
                                     "motor dynamics) -- the per-step entry points give the same bits", fn);
  const int D = h->obs_dim;
  if (!collect_shape_ok(h, pi))
    return fail(h, PDS_EUNSUPPORTED, "%s: actor shape (d_in must be the observation width %d <= 64, hidden <= 64, relu or tanh)", fn, D);
  if (!pi->w1 || !pi->b1 || !pi->w2 || !pi->b2 || !pi->w3 || !pi->b3) return fail(h, PDS_EINVAL, "%s: NULL pointer in the actor", fn);
  if (pi->d_out != (mode == kCollectSac ? 8 : 4))
    return fail(h, PDS_EINVAL, "%s: actor d_out %d in mode %d (DDPG 4, SAC 8)", fn, pi->d_out, mode);
  if (!(act_limit > 0.f) || !std::isfinite(act_limit)) return fail(h, PDS_EINVAL, "%s: act_limit %g", fn, (double)act_limit);
  const long long n = h->cfg.num_envs;
  if (capacity < n || capacity % n != 0 || ptr < 0 || ptr >= capacity || ptr % n != 0)
    return fail(h, PDS_EINVAL, "%s: capacity %lld and ptr %lld must be multiples of the handle's %lld envs, 0 <= ptr < capacity", fn,
                (long long)capacity, (long long)ptr, n);
  // the id packing of PDS_GAUSSIAN_PHILOX holds sample ids below 2^56
  if ((unsigned long long)n > (1ull << 56)) return fail(h, PDS_EINVAL, "%s: sample ids beyond 2^56", fn);
  if (!rollout_buffers_aligned(d_oa, d_obs) || (((uintptr_t)d_obs2) & 15u) || (((uintptr_t)d_rew | (uintptr_t)d_done |
      (uintptr_t)d_ep_ret | (uintptr_t)d_ep_len | (uintptr_t)d_tile_stats) & 3u))
    return fail(h, PDS_EINVAL, "%s: alignment (d_oa, d_obs2: 16 bytes; the others: 4)", fn);
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  CollectArgs ca;
  memset(&ca, 0, sizeof(ca));
  base_args(h, ca.s);
  if (const int rc = point_at_step_sink(h, fn, ca.s, stream)) return rc;
  ca.s.k_steps = K;
  ca.pi = *pi;
  ca.mode = mode; ca.K = K; ca.act_limit = act_limit; ca.log_std = d_log_std;
  ca.seed = seed; ca.first_call = first_call;
  ca.oa = d_oa; ca.obs2 = d_obs2; ca.rew = d_rew; ca.done = d_done;
  ca.capacity = capacity; ca.ptr = ptr;
  ca.obs = d_obs; ca.ep_ret = d_ep_ret; ca.ep_len = d_ep_len; ca.tile_stats = d_tile_stats;
  return launch_rollout(h, fn, K, stream, [&](dim3 grid, hipStream_t s) {
    const LaunchFlags &f = h->flags;
    const bool hover = h->cfg.task == PDS_TASK_HOVER;
    if (!plain) {  // (Hover or Circle: collect_control_env_supported)
      if (!f.lat) return hover ? launch_collect_hover_pid(f, grid, s, ca) : launch_collect_circle_pid(f, grid, s, ca);
      if (f.ctrl == 0) return hover ? launch_collect_hover_lat(f, grid, s, ca) : launch_collect_circle_lat(f, grid, s, ca);
      return hover ? launch_collect_hover_pid_lat(f, grid, s, ca) : launch_collect_circle_pid_lat(f, grid, s, ca);
    }
    if (hover) return launch_collect_hover(f, grid, s, ca);
    if (h->cfg.task == PDS_TASK_CIRCLE) return launch_collect_circle(f, grid, s, ca);
    return launch_collect_takeoff(f, grid, s, ca);
  });
}
extern "C" int pds_collect(pds_handle *h, int K, int mode, const pds_mlp *pi, float act_limit, const float *d_log_std, uint64_t seed,
                           uint64_t first_call, float *d_oa, float *d_obs2, float *d_rew, float *d_done, int64_t capacity,
                           int64_t ptr, float *d_obs, float *d_ep_ret, float *d_ep_len, float *d_tile_stats, void *stream) {
  return collect_call(h, "pds_collect", false, K, mode, pi, act_limit, d_log_std, seed, first_call, d_oa, d_obs2, d_rew, d_done, capacity,
                      ptr, d_obs, d_ep_ret, d_ep_len, d_tile_stats, stream);
}
// the same call that also takes the PID control modes and the latency ring (include/pds_collect_control.h)
extern "C" int pds_collect_control(pds_handle *h, int K, int mode, const pds_mlp *pi, float act_limit, const float *d_log_std,
                                   uint64_t seed, uint64_t first_call, float *d_oa, float *d_obs2, float *d_rew, float *d_done,
                                   int64_t capacity, int64_t ptr, float *d_obs, float *d_ep_ret, float *d_ep_len, float *d_tile_stats,
                                   void *stream) {
  return collect_call(h, "pds_collect_control", true, K, mode, pi, act_limit, d_log_std, seed, first_call, d_oa, d_obs2, d_rew, d_done,
                      capacity, ptr, d_obs, d_ep_ret, d_ep_len, d_tile_stats, stream);
}

// number of envs whose dynamic state holds a NaN or an Inf (diagnostic, see pds_count_nonfinite)
__global__ __launch_bounds__(256) void nonfinite_kernel(DevState st, long long n, unsigned long long *count) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const float4 a = st.s0[i], b = st.s1[i], c = st.s2[i];
    const float s = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w));
    bad = !(fabsf(s) <= 3.4e38f);  // NaN or Inf anywhere poisons the sum (Inf - Inf = NaN included)
  }
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(count, (unsigned long long)__popcll(m));
}

static int do_field(pds_handle *h, int field, void *d_ptr, int set, void *stream) {
  if (!h) return PDS_EINVAL;
  if (!d_ptr || pds_field_width(field) < 0) return fail(h, PDS_EINVAL, "bad field %d or NULL pointer", field);
  if (set && field == PDS_F_QUAT) return fail(h, PDS_EINVAL, "PDS_F_QUAT is derived (set PDS_F_RPY / PDS_F_QUAT_SIGN)");
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  FieldArgs a;
  memset(&a, 0, sizeof(a));
  a.st = h->st; a.k = h->k; a.user = d_ptr; a.n = h->cfg.num_envs; a.field = field; a.task = h->cfg.task; a.set = set;
  a.has_motor = h->flags.motor; a.has_dr = h->flags.dr; a.has_tn = h->flags.tn; a.has_on = h->flags.on; a.ctrl = h->flags.ctrl;
  a.regen_obs = h->flags.on && !h->flags.hold;
  // an edit of the state / step counter does not change what the env has OBSERVED: the kept observation is regenerated from the
  // unedited state first and stays in oh0-2 (the reference's history keeps the row that was returned, envs/base.py:303-319)
  if (set && field != PDS_F_NOISY_OBS)
    if (const int rc = materialize_kept_obs(h, (hipStream_t)stream)) return rc;
  if (const int rc = materialize_state(h, (hipStream_t)stream)) return rc;  // (reads too; an edit of the counter word drops kCtrBehindBit)
  a.env_id_base = (unsigned long long)h->cfg.env_id_base;
  a.seed_lo = (uint32_t)h->cfg.seed; a.seed_hi = (uint32_t)(h->cfg.seed >> 32);
  const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(field_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  PDS_HIP(h, hipGetLastError());
  if (set && !h->after_evaluate) h->was_reset = true;  // (an edit does not mend what an evaluation left: only a reset does)
  return PDS_OK;
}

extern "C" int pds_count_nonfinite(pds_handle *h, int64_t *count, void *stream) {
  if (!h || !count) return PDS_EINVAL;
  DeviceGuard guard(h->cfg.device);
  PDS_HIP(h, guard.err);
  hipStream_t s = (hipStream_t)stream;
  if (const int rc = materialize_state(h, s)) return rc;
  PDS_HIP(h, hipMemsetAsync(h->d_count, 0, sizeof(*h->d_count), s));  // handle-owned word: nothing to free
  const long long n = h->cfg.num_envs;
  hipLaunchKernelGGL(nonfinite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->st, n, h->d_count);
  PDS_HIP(h, hipGetLastError());
  unsigned long long host = 0;
  PDS_HIP(h, hipMemcpyAsync(&host, h->d_count, sizeof(host), hipMemcpyDeviceToHost, s));
  PDS_HIP(h, hipStreamSynchronize(s));
  *count = (int64_t)host;
  return PDS_OK;
}

extern "C" int pds_get_state(pds_handle *h, int field, void *d_out, void *stream) { return do_field(h, field, d_out, 0, stream); }
extern "C" int pds_set_state(pds_handle *h, int field, const void *d_in, void *stream) { return do_field(h, field, const_cast<void *>(d_in), 1, stream); }

template <int ROUNDS>
__global__ __launch_bounds__(256) void philox_kernel(const uint32_t *ctr, const uint32_t *key, long long n, uint32_t *out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U4 r = philox4x32<ROUNDS>(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1]);
  out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
}

__global__ __launch_bounds__(256) void noise_normals_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t tick_lo, uint32_t tick_hi,
                                                            uint32_t block, unsigned long long id_base, long long n, float *out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U4 r = philox4x32_7((uint32_t)(id_base + (unsigned long long)i), tick_lo, tick_hi, block, seed_lo, seed_hi);
  float z[8];
  box_muller_word(r.x, z[0], z[1]);
  box_muller_word(r.y, z[2], z[3]);
  box_muller_word(r.z, z[4], z[5]);
  box_muller_word(r.w, z[6], z[7]);
  float4 *o = reinterpret_cast<float4 *>(out + 8 * i);
  o[0] = make_float4(z[0], z[1], z[2], z[3]);
  o[1] = make_float4(z[4], z[5], z[6], z[7]);
}

extern "C" int pds_noise_normals(uint64_t seed, uint64_t tick, uint32_t block, uint64_t env_id_base, int64_t n, float *d_out,
                                 void *stream) {
  if (!d_out || n < 0 || (((uintptr_t)d_out) & 15u)) return PDS_EINVAL;
  if (n == 0) return PDS_OK;
  hipLaunchKernelGGL(noise_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)tick, (uint32_t)(tick >> 32), block, (unsigned long long)env_id_base,
                     (long long)n, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

// the two-word Box-Muller of the Gaussian policy sampler and the ES noise (pds_device.h box_muller), one word pair per lane
__global__ __launch_bounds__(256) void box_muller_kernel(const uint32_t *words, long long n, float *out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float z0, z1;
  box_muller(words[2 * i], words[2 * i + 1], z0, z1);
  out[2 * i] = z0; out[2 * i + 1] = z1;
}

extern "C" int pds_box_muller(const uint32_t *d_words, int64_t n, float *d_out, void *stream) {
  if (!d_words || !d_out || n < 1) return PDS_EINVAL;
  hipLaunchKernelGGL(box_muller_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_words,
                     (long long)n, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_philox4x32(const uint32_t *d_ctr, const uint32_t *d_key, int rounds, int64_t n, uint32_t *d_out, void *stream) {
  if (!d_ctr || !d_key || !d_out || n < 0 || (rounds != 7 && rounds != 10)) return PDS_EINVAL;
  if (n == 0) return PDS_OK;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (rounds == 10) hipLaunchKernelGGL(philox_kernel<10>, grid, dim3(256), 0, (hipStream_t)stream, d_ctr, d_key, (long long)n, d_out);
  else hipLaunchKernelGGL(philox_kernel<7>, grid, dim3(256), 0, (hipStream_t)stream, d_ctr, d_key, (long long)n, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

// Diagnostic builds (-DPDS_STAMPS): per-wave s_memtime stamps of the step kernel's phases, kStampSlots
// words per 64-env tile; NULL / 0 in regular builds.  Not part of include/pds.h.
extern "C" int pds_debug_stamps(pds_handle *h, unsigned long long *host_out, long long max_words) {
#ifdef PDS_STAMPS
  if (!h) return PDS_EINVAL;
  DeviceGuard guard(h->cfg.device);
  const long long ntiles = (h->cfg.num_envs + kWave - 1) / kWave;
  const long long words = ntiles * kStampSlots;
  if (!h->d_stamps) {
    PDS_HIP(h, hipMalloc((void **)&h->d_stamps, (size_t)words * 8));
    PDS_HIP(h, hipMemset(h->d_stamps, 0, (size_t)words * 8));
    return 0;
  }
  PDS_HIP(h, hipDeviceSynchronize());
  const long long w = words < max_words ? words : max_words;
  if (host_out && w > 0) PDS_HIP(h, hipMemcpy(host_out, h->d_stamps, (size_t)w * 8, hipMemcpyDeviceToHost));
  return (int)(w / kStampSlots);
#else
  (void)h; (void)host_out; (void)max_words;
  return PDS_EUNSUPPORTED;
#endif
}
