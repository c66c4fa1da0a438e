// pds_evaluate_hist.h -- ONE launch evaluates a POPULATION of observation-HISTORY policies (gfx950): P policies fly E episodes
// each, the actor reading the last H [o, u] halves of its env (observation_history_size = H, envs/base.py:44, 303-319, 417-431;
// H x half <= 192 inputs).  It joins two kernels that are pinned bit for bit against the per-step path:
//   * from rollout_hist_kernel (csrc/pds_rollout_hist.h): one block per 64-env tile -- the LDS leaves room for one team --, the
//     actor's wide image (W1 [64][16 HN + 4], stage_net_wide), the history tile [64][16 HN + 4] that is the network input
//     (gather_hist -> forward16_wide, the code path of pds_mlp_forward with more than 64 inputs: same bits) and the env wave's
//     in-place update of its own history row behind every step (pds_history_advance, csrc/pds_history.hip: same values);
//   * from evaluate_kernel (csrc/pds_evaluate.h): the policy per TILE (tile t flies policy t / tiles_per_policy: its six tensors
//     from row p of the flat [P, param_count] block, its standardisation from row p of the [P, H half] mean / std), return,
//     length and cost frozen at an env's first `terminated | truncated`, the cost read back from the sink row behind the post,
//     the counted loop a stopped tile falls through (the parity behind the loop is parity(entry) ^ (T & 1) in EVERY tile), the
//     eight PDS_EM_* flight metrics through em_lds, and the two counters with the kEvalStop protocol.
// Not here: action noise, log-probability and action buffer; an obs_buf store, the `fin` image and the fin_rows list (a finished
// env's history restarts from its reset row, and nobody reads the history it had -- the newest half the per-step path takes from
// final_obs lands in a row the restart overwrites whole); the stats form (it stays on the composed path for history envs).
//
// Hand-over (rollout_wait_ge / rollout_post of csrc/pds_rollout.h, eval_wait_ge / eval_post of csrc/pds_evaluate.h; all five waves
// of the block are resident together):
//   act_ready: +1 per network wave and step, after the wave has read its 16 history rows of step s and written their actions.  The
//              env wave waits for 4 (s + 1) in front of step s.
//   obs_ready: posted ONCE by the env wave at the end of every iteration s it runs, after the histories of step s + 1 are in LDS:
//              +1 when it will run step s + 1, + kEvalStop when it will not (no lane in its first episode, or s + 1 == T).  After
//              iteration s the counter is either s + 1 or >= kEvalStop, never anything else.
//   A network wave waits for obs_ready >= s in front of step s and looks at the value that ended its wait: s (the env wave will
//   wait for this step's actions: compute and post them) or >= kEvalStop (it will not: leave).  So every wait has its post on
//   every path: the env wave only waits for actions of a step it announced with +1 (step 0: the counter's initial 0 announces it),
//   a network wave only waits for the end of an iteration the env wave has started -- and the env wave ends EVERY iteration it
//   starts with a post, the last one with the stop.  How the team drains: the env wave never waits behind its stop (the
//   iterations that remain are the `stopped` fall-through, without a wait), it stores its results and returns; each network wave
//   sees >= kEvalStop at its next wait, whichever step it is at, and returns.  Blocks share no counter.
//   LDS images: the history tile and the kernel's own [o(k), o(k + 1)] row tile are written by the env wave between its
//   act_ready wait and its obs_ready post; the network waves read the history tile between their obs_ready wait and their
//   act_ready post, and never touch the row tile; the action slots go the other way round.  em_lds belongs to the env wave.
//
// METRICS: the env wave always sums the eight PDS_EM_* values, exactly as evaluate_kernel<.., METRICS = true> does -- seven words
// per lane in LDS, read and written back behind the act_ready wait, one rounded instruction per product and sum -- and stores the
// [N, 8] row where d_metrics is non-NULL: one code object per variant instead of a plain and a metrics form.
#pragma once
#include "pds_evaluate.h"
#include "pds_evaluate_hist_args.h"
#include "pds_rollout_hist.h"

namespace pds {

// pds_history_advance for this lane's own row of the history tile (the statements of rollout_hist_kernel, which keeps its own
// copy: its code objects stay the ones they were): shift by one half, append the newest half -- the second half of the step's row
// `krow`; where the env finished (`dn`), the restart from the reset row `krow` holds then: H - 1 copies of its first half, then
// its second half (envs/base.py:417-431).  Reads in blocks, then the block's writes (csrc/pds_rollout_hist.h says why).
template <int HALF>
PDS_DEV void eval_hist_advance_row(float *hrow, const float *krow, int H, bool dn) {
  const int keep = H * HALF - HALF;
  const float *newest = krow + HALF;
  if constexpr (HALF % 4 == 0) {  // 16-byte aligned halves: b128 moves
    for (int j0 = 0; j0 < keep; j0 += 32) {
      float4 buf[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) buf[u] = (j0 + 4 * u < keep) ? *reinterpret_cast<const float4 *>(hrow + j0 + 4 * u + HALF) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 8; ++u) if (j0 + 4 * u < keep) *reinterpret_cast<float4 *>(hrow + j0 + 4 * u) = buf[u];
    }
    float4 nb[HALF / 4];
#pragma unroll
    for (int c = 0; c < HALF / 4; ++c) nb[c] = *reinterpret_cast<const float4 *>(newest + 4 * c);
#pragma unroll
    for (int c = 0; c < HALF / 4; ++c) *reinterpret_cast<float4 *>(hrow + keep + 4 * c) = nb[c];
  } else {
    for (int j0 = 0; j0 < keep; j0 += 16) {
      float buf[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) buf[u] = (j0 + u < keep) ? hrow[j0 + u + HALF] : 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) if (j0 + u < keep) hrow[j0 + u] = buf[u];
    }
    float nb[HALF];
#pragma unroll
    for (int c = 0; c < HALF; ++c) nb[c] = newest[c];
#pragma unroll
    for (int c = 0; c < HALF; ++c) hrow[keep + c] = nb[c];
  }
  if (dn) {
    float k0[HALF], k1[HALF];
#pragma unroll
    for (int c = 0; c < HALF; ++c) { k0[c] = krow[c]; k1[c] = krow[HALF + c]; }
    for (int j = 0; j < H - 1; ++j)
#pragma unroll
      for (int c = 0; c < HALF; ++c) hrow[j * HALF + c] = k0[c];
#pragma unroll
    for (int c = 0; c < HALF; ++c) hrow[keep + c] = k1[c];
  }
}

template <class V_, int HN>
__global__ __launch_bounds__(kRolloutThreads, 1) void evaluate_hist_kernel(const EvalHistArgs ka) {
  using namespace pds_mlpf;
  const EvalArgs &ea = ka.m.e;
  using V = std::conditional_t<regen_obs_variant<V_>(), StoredOh<V_>, V_>;
  constexpr int D = V::D;                    // the kernel's own row: two halves
  constexpr int HALF = D / 2;
  constexpr int TS = tile_stride<D>();
  constexpr int S1 = kTW * HN + 4;           // row stride of the history tile and of W1's image
  constexpr int RM = merged_reset_variant<V>() ? RM_MERGED : RM_INLINE;
  constexpr int kScratchU4_ = (RM == RM_MERGED) ? kMergedScratchU4 : (inline_coop_variant<V>() ? inline_envs<V, false>() * scratch_stride<V>() : 0);
  __shared__ __attribute__((aligned(16))) float net_pi[net_floats_wide<HN>()];
  __shared__ __attribute__((aligned(16))) float mus[kTW * HN], iss[kTW * HN];
  __shared__ __attribute__((aligned(16))) float hist[kWave * S1];
  __shared__ __attribute__((aligned(16))) float tile[kWave * TS];
  __shared__ __attribute__((aligned(16))) float4 act_all[kWave];
  __shared__ uint32_t queue[kQueueCap];
  __shared__ U4 scratch[kScratchU4_ > 0 ? kScratchU4_ : 1];
  __shared__ int obs_ready, act_ready;
#ifdef PDS_STAMPS
  unsigned long long stamp_[kStampSlots];
#endif
  prefetch_kernargs();
  const StepArgs &a = ea.s;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_env = wave >= kRolloutMlpWaves;
  const int n16 = lane & 15, g = lane >> 4;
  const NetLds wpi = net_lds_wide<HN>(net_pi);
  const long long t = blockIdx.x;  // this block's 64-env tile (N = P x E, E a multiple of 64: every tile is full)
  const int T = ea.T, H = ka.H;
  const int HS = H * HALF;         // floats per history row (= the actors' d_in <= 16 HN)

  // ---- prologue: policy p's actor and statistics and the tile's histories into LDS ------------------------------------
  {
    const long long p = t / ea.tiles_per_policy;
    pds_mlp m = ea.shape;
    const float *row = ea.params + p * ea.param_count;  // W1 b1 W2 b2 W3 b3, torch order (pds_mlp_param_count)
    m.w1 = row;
    m.b1 = m.w1 + m.h1 * m.d_in;
    m.w2 = m.b1 + m.h1;
    m.b2 = m.w2 + m.h2 * m.h1;
    m.w3 = m.b2 + m.h2;
    m.b3 = m.w3 + m.d_out * m.h2;
    stage_net_wide<HN>(m, wpi, tid, kRolloutThreads);
    for (int i = tid; i < kTW * HN; i += kRolloutThreads) {
      const bool on = ea.mean != nullptr && i < HS;
      mus[i] = on ? ea.mean[p * HS + i] : 0.f;
      iss[i] = on ? 1.0f / (ea.stdv[p * HS + i] + ea.eps) : 1.f;
    }
    for (int i = tid; i < kWave * S1; i += kRolloutThreads) {
      const int r = i / S1, c = i - r * S1;
      hist[i] = (c < HS) ? ea.obs0[(t * kWave + r) * HS + c] : 0.f;
    }
  }
  if (tid == 0) { obs_ready = 0; act_ready = 0; }
  __syncthreads();  // (the only block barrier: from here on the roles meet through the counters)

  if (is_env) {
    // ================================ env wave: the tile's 64 envs in registers =================================
#if PDS_ROLLOUT_ENV_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ENV_PRIO);
#endif
    const long long wave_base = t * kWave;
    const bool active = true;
    const Idx<V> ix{wave_base, (uint32_t)lane};
    PDS_ENV_WAVE_BEGIN
    float ep_ret = 0.f, ep_len = 0.f, ep_cost = 0.f;
    bool alive = true;          // this lane's env is in its first episode
    float c_step = 0.f;         // the last step's cost, on its way back from the sink row ...
    bool c_counts = false;      // ... and whether it belongs to the first episode
    int qcount = 0;
    bool stopped = false;  // wave-uniform: this tile has posted its stop
    float *hrow = hist + lane * S1;
    // the metrics' seven words per lane (csrc/pds_evaluate.h em_lds): zero sums; the signs of x(0)'s roll and pitch rate
    float4 *em = em_lds<1>();
    em[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    em[kWave + lane] = make_float4(0.f, __int_as_float((S.e.wx < 0.f ? 1 : 0) | (S.e.wy < 0.f ? 2 : 0)), __int_as_float(0), 0.f);
    for (int s = 0; s < T; ++s) {
      const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<311, true>(ea.s, s));
      // (a stopped tile falls through its remaining iterations; the parity of the state ring goes on toggling: csrc/pds_evaluate.h)
      if (stopped) { parity ^= 1; continue; }
      rollout_wait_ge(&act_ready, kRolloutMlpWaves * (s + 1));  // the network waves have read the histories and written a(s)
      ep_cost += c_counts ? c_step : 0.f;
      RngKey rks = rk;  // (opaque per-iteration copies: see step_k_kernel)
      int lane_s = lane;
      asm volatile("" : "+s"(rks.seed_lo), "+s"(rks.seed_hi), "+v"(lane_s));
      long long o1 = 0;  // every step's outputs go to the SAME sink row: offset 0, but opaque (csrc/pds_evaluate.h)
      asm volatile("" : "+s"(o1));
      const float4 act = act_all[lane_s];
      {  // x(s), the state the policy acted in, and a(s), raw, against u(k - 1) = the last action before the step
        const float4 sums = em[lane_s], rest = em[kWave + lane_s];
        float m_roll = sums.x, m_pitch = sums.y, m_rate = sums.z, m_act = sums.w, m_tilt = rest.x;
        int m_sat = __float_as_int(rest.y), m_cross = __float_as_int(rest.z);
        const EnvRegs &e = S.e;
        m_roll = __fadd_rn(m_roll, alive ? __fmul_rn(e.roll, e.roll) : 0.f);
        m_pitch = __fadd_rn(m_pitch, alive ? __fmul_rn(e.pitch, e.pitch) : 0.f);
        const float w2 = __fadd_rn(__fadd_rn(__fmul_rn(e.wx, e.wx), __fmul_rn(e.wy, e.wy)), __fmul_rn(e.wz, e.wz));
        m_rate = __fadd_rn(m_rate, alive ? w2 : 0.f);
        const float ar = fabsf(e.roll), ap = fabsf(e.pitch);  // (one compare each: a NaN angle is passed over, whichever it is)
        m_tilt = (alive && ar > m_tilt) ? ar : m_tilt;
        m_tilt = (alive && ap > m_tilt) ? ap : m_tilt;
        const int neg = (e.wx < 0.f ? 1 : 0) | (e.wy < 0.f ? 2 : 0);
        const int crossed = alive ? ((neg ^ m_sat) & 3) : 0;
        m_cross += (crossed & 1) | ((crossed & 2) << 15);
        m_sat = (m_sat & ~3) | neg;
        const float d0 = __fsub_rn(act.x, S.h1.x), d1 = __fsub_rn(act.y, S.h1.y), d2 = __fsub_rn(act.z, S.h1.z), d3 = __fsub_rn(act.w, S.h1.w);
        const float dd = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)), __fmul_rn(d3, d3));
        m_act = __fadd_rn(m_act, alive ? dd : 0.f);
        const bool sat = fabsf(act.x) > 1.f || fabsf(act.y) > 1.f || fabsf(act.z) > 1.f || fabsf(act.w) > 1.f;
        m_sat += (alive && sat) ? 4 : 0;
        em[lane_s] = make_float4(m_roll, m_pitch, m_rate, m_act);
        em[kWave + lane_s] = make_float4(m_tilt, __int_as_float(m_sat), __int_as_float(m_cross), 0.f);
      }
      StepOut so;
      step_once<V, kWave, RM, false>(el.s, o1, rks, parity, nullptr, tile, nullptr, queue, scratch, lane_s, wave_base, ix, active, act, S,
                                     qcount, nullptr, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      // the accumulator updates of evaluation.evaluate, in its order and its form (x + 0 for an env that has finished)
      ep_ret += alive ? so.reward : 0.f;
      ep_len += alive ? 1.f : 0.f;
      c_counts = alive;
      const bool dn = so.done || so.trunc;
      alive = alive && !dn;
      // the history of step s + 1, this lane's own row (the env goes on behind its first episode: auto-reset in place)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // (step_once's wave-cooperative writes of `tile` are complete)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      eval_hist_advance_row<HALF>(hrow, tile + lane * TS, H, dn);
      const unsigned long long still = __ballot(alive);
      const bool more = still != 0ull && s + 1 < T;  // wave-uniform
      eval_post(&obs_ready, lane, more ? 1 : kEvalStop);  // the histories of step s + 1 are in LDS / the env wave has left
      c_step = *at(el.s.cost, ix);  // (behind the post: csrc/pds_evaluate.h)
      stopped = !more;
    }
    ep_cost += c_counts ? c_step : 0.f;
    // The state as the tile left it and the clock T ticks on, whichever step the tile stopped at: the caller resets before it
    // steps again (pds_evaluate_policies_history leaves the handle "not reset").
    const EvalHistArgs &kl = *reinterpret_cast<const EvalHistArgs *>(&reload_args<312, true>(ea.s, T));
    const EvalArgs &el = kl.m.e;
    store_state<V>(el.s, ix, parity, S, true);
    advance_clock(el.s.st.clk, t, rk0, parity, (uint32_t)T, lane);
    *at(el.ret, ix) = ep_ret;
    *at(el.len, ix) = ep_len;
    *at(el.cost, ix) = ep_cost;
    if (kl.m.metrics != nullptr) {  // row `env` of [N, 8] as two 16-byte pieces (every tile is full: env < N)
      float4 *row = reinterpret_cast<float4 *>(kl.m.metrics) + 2 * (wave_base + lane);
      const float4 rest = em[kWave + lane];
      const int m_sat = __float_as_int(rest.y), m_cross = __float_as_int(rest.z);
      row[0] = em[lane];
      row[1] = make_float4(rest.x, (float)(m_sat >> 2), (float)(m_cross & 0xFFFF), (float)((unsigned)m_cross >> 16));
    }
    return;
  }

  // ================================ network waves: the actor for 16 rows of the tile each ========================
  const int own = wave * 16 + n16;  // this lane's sample row
  for (int s = 0;; ++s) {
    const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<313, true>(ea.s, s));
    if (eval_wait_ge(&obs_ready, s) >= kEvalStop) break;  // the histories of step s are in LDS, or the env wave has left
#if PDS_ROLLOUT_ACTOR_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ACTOR_PRIO);
#endif
    f32x4 x_own[HN];
    gather_hist<HN>(hist + own * S1, HS, mus, iss, g, x_own);
    const bool kh2 = el.shape.h1 == el.shape.h2 && last_tile_steps(el.shape.h1, kNT) == 2;
    f32x4 mu;
    if (el.shape.activation == 0) mu = kh2 ? forward16_wide<0, HN, S1, 2>(wpi, x_own, n16, g) : forward16_wide<0, HN, S1, 4>(wpi, x_own, n16, g);
    else mu = kh2 ? forward16_wide<1, HN, S1, 2>(wpi, x_own, n16, g) : forward16_wide<1, HN, S1, 4>(wpi, x_own, n16, g);
    if (g == 0) act_all[own] = make_float4(mu[0], mu[1], mu[2], mu[3]);  // lane n16 owns sample `own`: the actor's four outputs
    rollout_post(&act_ready, lane);  // this wave is done with the histories of step s
  }
}

template <class RV_>
inline void launch_evaluate_hist_variant(int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka) {
  if (hn == 4) hipLaunchKernelGGL((evaluate_hist_kernel<RV_, 4>), grid, dim3(kRolloutThreads), 0, s, ka);
  else if (hn == 6) hipLaunchKernelGGL((evaluate_hist_kernel<RV_, 6>), grid, dim3(kRolloutThreads), 0, s, ka);
  else if (hn == 8) hipLaunchKernelGGL((evaluate_hist_kernel<RV_, 8>), grid, dim3(kRolloutThreads), 0, s, ka);
  else hipLaunchKernelGGL((evaluate_hist_kernel<RV_, 12>), grid, dim3(kRolloutThreads), 0, s, ka);
}
// The variants of launch_rollout_hist_task (csrc/pds_rollout_hist.h): {lean, reference-default noise} x {with, without motor
// dynamics; TakeOff: without}; CTRL 0: control_mode PWM (csrc/pds_evaluate_hist_<task>.hip), 1 / 2: AttitudeRate / Attitude
// (csrc/pds_evaluate_hist_<task>_pid.hip).
template <int TASK, int CTRL = 0>
inline bool launch_evaluate_hist_task(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka) {
  static_assert(CTRL == 0 || TASK != PDS_TASK_TAKEOFF, "TakeOff fixes control_mode PWM (envs/takeoff.py:225)");
  if (!rollout_hist_supported(TASK, f) || f.ctrl != CTRL) return false;
  const bool full = f.on;
  if constexpr (TASK != PDS_TASK_TAKEOFF) {
    if (f.motor) {
      if (full) launch_evaluate_hist_variant<Variant<TASK, true, true, false, true, true, CTRL, false, false>>(hn, grid, s, ka);
      else launch_evaluate_hist_variant<Variant<TASK, true, false, false, false, false, CTRL, false, false>>(hn, grid, s, ka);
      return true;
    }
  }
  if (full) launch_evaluate_hist_variant<Variant<TASK, false, true, false, true, true, CTRL, false, false>>(hn, grid, s, ka);
  else launch_evaluate_hist_variant<Variant<TASK, false, false, false, false, false, CTRL, false, false>>(hn, grid, s, ka);
  return true;
}
template <int TASK>
inline bool launch_evaluate_hist_pid(const LaunchFlags &f, int hn, dim3 grid, hipStream_t s, const EvalHistArgs &ka) {
  if (f.ctrl == 1) return launch_evaluate_hist_task<TASK, 1>(f, hn, grid, s, ka);
  return launch_evaluate_hist_task<TASK, 2>(f, hn, grid, s, ka);
}

}  // namespace pds
