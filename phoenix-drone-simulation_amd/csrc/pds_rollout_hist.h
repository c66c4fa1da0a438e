// pds_rollout_hist.h -- ONE launch per rollout for observation histories other than 2 (observation_history_size = H,
// envs/base.py:44, 303-319, 417-431; the reference's experiments/04_history_of_state_action_inputs trains H = 1, 2, 4, 6, 8):
// the actor reads the last H [o, u] halves of every env, H x half <= 192 floats.
//
// Rounds 2-5 ran such a rollout as 8 launches per step (critic, actor, sample, env step, pds_history_advance, V(final_obs),
// record, + copies); csrc/pds_rollout.h -- the one-launch form for H = 2 -- keeps both networks' weights and the observation
// tile in LDS, which at 160 inputs would take 233 KB.  Here:
//   * the ACTOR, the sampling (PDS_DRAW_ACTION_NOISE / PDS_EMIT_ACTION of csrc/pds_rollout.h), the env step (step_once inside the
//     prologue PDS_ENV_WAVE_BEGIN of csrc/pds_rollout.h), the history update of pds_history_advance
//     (csrc/pds_history.hip, same values) and the episode bookkeeping (PDS_RECORD_STEP of csrc/pds_rollout.h) run in the kernel: one
//     block per 64-env tile, four network waves (16 rows each, csrc/pds_mlp_fwd.h forward16_wide: the code path of
//     pds_mlp_forward, same bits) + one env wave, hand-over through LDS counters as in csrc/pds_rollout.h;
//   * the CRITIC does not: V(o(t)) for all t is one pds_mlp_forward over obs_buf after the kernel (it is off the step's
//     critical path; at H = 2 the in-kernel critic measured 6 % ahead of this, csrc/pds_rollout.h header), and the final
//     histories of the envs the TimeLimit cut (or that finished on the rollout's last step: algs/iwpg/iwpg.py:374-379) go to a
//     small per-env slot list `fin_rows` / `fin_step` that the caller evaluates the same way;
//   * LDS: the actor's image (W1 [64][16 HN + 4]), the history tile [64][16 HN + 4] (the network input, shifted in place by
//     the env wave), the kernel's own [o(k), o(k + 1)] row tile and the finished envs' last rows: 152 KB at HN = 12.
// obs_buf [T + 1, N, H half]: row 0 = the histories on entry (the env's current observation), row t + 1 written by step t.
#pragma once
#include "pds_rollout.h"

namespace pds {

// network input of this lane from a history row: features 16 kt + 4 g + q (one b128 read per input tile)
template <int NIN>
PDS_DEV void gather_hist(const float *row, int d_in, const float *mus, const float *iss, int g, pds_mlpf::f32x4 (&xin)[NIN]) {
#pragma unroll
  for (int kt = 0; kt < NIN; ++kt) {
    const int k0 = kt * 16 + 4 * g;
    const pds_mlpf::f32x4 v = pds_mlpf::lds4(row + k0), mu = pds_mlpf::lds4(mus + k0), is = pds_mlpf::lds4(iss + k0);
#pragma unroll
    for (int q = 0; q < 4; ++q) xin[kt][q] = ((k0 + q < d_in ? v[q] : mu[q]) - mu[q]) * is[q];
  }
}

// ---- pds_history_advance (csrc/pds_history.hip, same values) for the env wave's own row `hrow` of the history tile, for both
// history kernels.  Statement macros over a constant HALF in scope, like PDS_ENV_WAVE_BEGIN of csrc/pds_rollout.h and for its
// reason: rollout_hist_kernel expands them in its loop, with its fin_rows copy between the two -- called as forced-inline template
// functions they change every TakeOff rollout_hist_kernel (16-18 instructions fewer, another schedule).  evaluate_hist_kernel
// (csrc/pds_evaluate_hist.h) was built on such a function and loses 5-6 instructions per kernel with the statements in its
// loop, so its function stays, with these two macros as its body
// (profiles/fused_refactor_identity.txt). ----
// Shift by one half (`keep` = H HALF - HALF floats stay) and append the HALF floats at `newest`.  Blocks of reads, then the block's
// writes: a read-then-write loop over one array serialises on the LDS latency of every element -- the compiler must assume the two
// alias --, ~130 cycles x 51 moves for Hover H = 4: 18.7 -> 13 us per step.  16-byte aligned halves: b128 moves (8 consecutive
// lanes cover all banks).
#define PDS_HIST_SHIFT_APPEND(hrow, newest, keep)                                                                                                               \
  if constexpr (HALF % 4 == 0) {                                                                                                                                \
    for (int j0 = 0; j0 < keep; j0 += 32) {                                                                                                                     \
      float4 buf[8];                                                                                                                                            \
      _Pragma("unroll")                                                                                                                                         \
      for (int u = 0; u < 8; ++u) buf[u] = (j0 + 4 * u < keep) ? *reinterpret_cast<const float4 *>(hrow + j0 + 4 * u + HALF) : make_float4(0.f, 0.f, 0.f, 0.f); \
      _Pragma("unroll")                                                                                                                                         \
      for (int u = 0; u < 8; ++u) if (j0 + 4 * u < keep) *reinterpret_cast<float4 *>(hrow + j0 + 4 * u) = buf[u];                                               \
    }                                                                                                                                                           \
    float4 nb[HALF / 4];                                                                                                                                        \
    _Pragma("unroll")                                                                                                                                           \
    for (int c = 0; c < HALF / 4; ++c) nb[c] = *reinterpret_cast<const float4 *>(newest + 4 * c);                                                               \
    _Pragma("unroll")                                                                                                                                           \
    for (int c = 0; c < HALF / 4; ++c) *reinterpret_cast<float4 *>(hrow + keep + 4 * c) = nb[c];                                                                \
  } else {                                                                                                                                                      \
    for (int j0 = 0; j0 < keep; j0 += 16) {                                                                                                                     \
      float buf[16];                                                                                                                                            \
      _Pragma("unroll")                                                                                                                                         \
      for (int u = 0; u < 16; ++u) buf[u] = (j0 + u < keep) ? hrow[j0 + u + HALF] : 0.f;                                                                        \
      _Pragma("unroll")                                                                                                                                         \
      for (int u = 0; u < 16; ++u) if (j0 + u < keep) hrow[j0 + u] = buf[u];                                                                                    \
    }                                                                                                                                                           \
    float nb[HALF];                                                                                                                                             \
    _Pragma("unroll")                                                                                                                                           \
    for (int c = 0; c < HALF; ++c) nb[c] = newest[c];                                                                                                           \
    _Pragma("unroll")                                                                                                                                           \
    for (int c = 0; c < HALF; ++c) hrow[keep + c] = nb[c];                                                                                                      \
  }
// The restart of a finished env from its reset row `krow` (the step's row of the kernel's own tile): H - 1 copies of its first
// half, then its second half (envs/base.py:417-431).
#define PDS_HIST_RESTART(hrow, krow, H, keep)                                 \
  float k0[HALF], k1[HALF];                                                   \
  _Pragma("unroll")                                                           \
  for (int c = 0; c < HALF; ++c) { k0[c] = krow[c]; k1[c] = krow[HALF + c]; } \
  for (int j = 0; j < H - 1; ++j)                                             \
    _Pragma("unroll")                                                         \
    for (int c = 0; c < HALF; ++c) hrow[j * HALF + c] = k0[c];                \
  _Pragma("unroll")                                                           \
  for (int c = 0; c < HALF; ++c) hrow[keep + c] = k1[c];

// The actor's pass for this lane's 16 rows, both history kernels: forward16_wide (csrc/pds_mlp_fwd.h) with the tile steps of
// pds_mlp_forward's dispatch.  `m`: the actor's shape; reads wpi, x_own, n16, g; declares kh2 and the output `mu`.  (As a
// forced-inline function it left every rollout_hist_kernel alone and moved the HN = 12 forms of evaluate_hist_kernel.)
#define PDS_FORWARD16_WIDE(m, mu)                                                                                                         \
  const bool kh2 = m.h1 == m.h2 && last_tile_steps(m.h1, kNT) == 2;                                                                       \
  f32x4 mu;                                                                                                                               \
  if (m.activation == 0) mu = kh2 ? forward16_wide<0, HN, S1, 2>(wpi, x_own, n16, g) : forward16_wide<0, HN, S1, 4>(wpi, x_own, n16, g);  \
  else mu = kh2 ? forward16_wide<1, HN, S1, 2>(wpi, x_own, n16, g) : forward16_wide<1, HN, S1, 4>(wpi, x_own, n16, g);

template <class V_, int HN>
__global__ __launch_bounds__(kRolloutThreads, 1) void rollout_hist_kernel(const RolloutHistArgs ra) {
  using namespace pds_mlpf;
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
  __shared__ __attribute__((aligned(16))) float fin[kWave * D];
  __shared__ __attribute__((aligned(16))) float4 act_all[kWave];
  __shared__ uint32_t queue[kQueueCap];
  __shared__ U4 scratch[kScratchU4_ > 0 ? kScratchU4_ : 1];
  __shared__ int obs_ready, act_ready;
#ifdef PDS_STAMPS
  unsigned long long stamp_[kStampSlots];
#endif
  prefetch_kernargs();
  const StepArgs &a = ra.s;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_env = wave >= kRolloutMlpWaves;
  const int n16 = lane & 15, g = lane >> 4;
  const NetLds wpi = net_lds_wide<HN>(net_pi);
  const long long t = blockIdx.x;  // this block's 64-env tile
  const int T = ra.T, H = ra.H;
  const int HS = H * HALF;         // floats per history row (= the actor's d_in)
  const int d_out = ra.pi.d_out;
  const long long rem0 = a.n - t * kWave;
  const int rows = rem0 >= kWave ? kWave : (int)rem0;

  // ---- prologue: the actor, the statistics and the histories into LDS; env state into the env wave's registers ----
  stage_net_wide<HN>(ra.pi, wpi, tid, kRolloutThreads);
  for (int i = tid; i < kTW * HN; i += kRolloutThreads) {
    const bool on = ra.mean != nullptr && i < HS;
    mus[i] = on ? ra.mean[i] : 0.f;
    iss[i] = on ? 1.0f / (ra.stdv[i] + ra.eps) : 1.f;
  }
  for (int i = tid; i < kWave * S1; i += kRolloutThreads) {
    const int r = i / S1, c = i - r * S1;
    hist[i] = (r < rows && c < HS) ? ra.obs_buf[(t * kWave + r) * HS + c] : 0.f;
  }
  if (tid == 0) { obs_ready = 0; act_ready = 0; }
  unsigned long long call0 = ra.call_offset;
  if (ra.call_base != nullptr) call0 += *ra.call_base;
  __syncthreads();  // (the only block barrier: from here on the roles meet through the counters)

  if (is_env) {
    // ================================ env wave: the tile's 64 envs in registers =================================
#if PDS_ROLLOUT_ENV_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ENV_PRIO);
#endif
    const long long wave_base = t * kWave;
    const bool active = rem0 >= kWave || lane < (int)rem0;
    const Idx<V> ix{wave_base, active ? (uint32_t)lane : (uint32_t)rem0 - 1u};
    PDS_ENV_WAVE_BEGIN
    float ep_ret = *at(ra.ep_ret, ix), ep_len = *at(ra.ep_len, ix), st0 = 0.f, st1 = 0.f, st2 = 0.f;
    int qcount = 0, nfin = 0;
    float *hrow = hist + lane * S1;
    for (int s = 0; s < T; ++s) {
      const RolloutHistArgs &rl = *reinterpret_cast<const RolloutHistArgs *>(&reload_args<211, true>(ra.s, s));
      const long long o1 = (long long)s * rl.s.n;
      rollout_wait_ge(&act_ready, kRolloutMlpWaves * (s + 1));  // the network waves have read the histories and written a(s)
      PDS_OPAQUE_STEP_COPIES
      const float4 act = act_all[lane_s];
      [[maybe_unused]] int ep_step = 0;  // LAT: env.step()s of this env since its last reset, in front of this one
      if constexpr (V::LAT) ep_step = (int)ctr_step(S.ctr);
      StepOut so;
      step_once<V, kWave, RM, false>(rl.s, o1, rks, parity, nullptr, tile, nullptr, queue, scratch, lane_s, wave_base, ix, active, act, S,
                                     qcount, fin, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      PDS_RECORD_STEP(so)
      // pds_history_advance (csrc/pds_history.hip), this lane's own row: shift by one half, append the newest half -- of the
      // env's LAST observation where it finished (`fin`: the row that goes to final_obs), of the step's row otherwise
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // (step_once's wave-cooperative writes of `tile` and `fin` are complete)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const float *krow = tile + lane * TS;
      const float *newest = dn ? fin + lane * D + HALF : krow + HALF;
      const int keep = HS - HALF;
      PDS_HIST_SHIFT_APPEND(hrow, newest, keep)
      // the latency ring (pds_history_advance_latency, csrc/pds_history.hip, same values): at step j = ep_step + 1 <= H of an
      // episode the action columns of the slots 0 .. H - j are still the reference's VIEWS of action_buffer[-1]
      // (envs/agents.py:386, envs/base.py:424-429) and show the raw action when this step's apply_action calls rewrote that row,
      // floor(j agg / B) > floor((j - 1) agg / B) -- in the final history of an env that finishes here too, hence in front of
      // the fin_rows copy and the restart.  Divergent, but at most H four-float LDS writes, none after step H of an episode.
      if constexpr (V::LAT) {
        const int views = H - ep_step;  // slots 0 .. H - j
        if (views > 0) {
          const int B = rl.s.k.lat_steps, agg = rl.s.k.agg;
          if ((ep_step + 1) * agg / B > ep_step * agg / B) {
            for (int j = 0; j < views; ++j) {
              float *u = hrow + j * HALF + (HALF - 4);
              u[0] = act.x; u[1] = act.y; u[2] = act.z; u[3] = act.w;
            }
          }
        }
      }
      // the final history of an env the TimeLimit cut bootstraps its path with V (also when it terminated on that step, and
      // for every env that finished on the rollout's last step: algs/iwpg/iwpg.py:374-379; the rule behind done_all[] of
      // rollout_kernel, where the reason for the two wordings is) -> the caller's slot list
      const bool want = dn && (so.trunc || s == T - 1);
      unsigned long long wm = __ballot(want);
      if (wm != 0ull) {  // wave-uniform, rare
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        while (wm != 0ull) {
          const int src = __builtin_ctzll(wm);
          wm &= wm - 1ull;
          const int slot = __builtin_amdgcn_readlane(nfin, src);
          if (slot < rl.slots) {
            float *dst = rl.fin_rows + ((long long)slot * rl.s.n + wave_base + src) * HS;
            for (int c = lane; c < HS; c += kWave) dst[c] = hist[src * S1 + c];
            if (lane == 0) rl.fin_step[(long long)slot * rl.s.n + wave_base + src] = s;
          }
        }
        if (want) ++nfin;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (the rows are overwritten below)
      }
      if (dn) {
        PDS_HIST_RESTART(hrow, krow, H, keep)
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // o(s + 1) -> obs_buf[s + 1]: the tile's rows are one contiguous piece of it (wave-cooperative, 256 B per pass)
      {
        float *dst = rl.obs_buf + ((long long)(s + 1) * rl.s.n + wave_base) * HS;
        const int total = rows * HS;
        // 16-byte stores where the rows allow it (H half a multiple of 4: Circle, TakeOff, Hover at H = 4 / 8; the piece of obs_buf
        // 16-byte aligned): the first form of this copy, 4 bytes per lane and store, was 68 store instructions per step at H = 4 --
        // the release fence behind them waits for every one of them
        if ((HS & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
          const int q4 = HS >> 2, total4 = total >> 2;  // float4 per row / in all
          int r = lane / q4, c4 = lane - r * q4;
          for (int idx0 = lane; idx0 < total4; idx0 += 4 * kWave) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              v[u] = (idx0 + u * kWave < total4) ? *reinterpret_cast<const float4 *>(hist + r * S1 + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
              c4 += kWave;
              while (c4 >= q4) { c4 -= q4; ++r; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (idx0 + u * kWave < total4) nt_store4(reinterpret_cast<float4 *>(dst) + idx0 + u * kWave, v[u]);
          }
        } else {
          int r = lane / HS, c = lane - r * HS;
          for (int idx0 = lane; idx0 < total; idx0 += 8 * kWave) {  // eight LDS reads in flight, then their stores
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              v[u] = (idx0 + u * kWave < total) ? hist[r * S1 + c] : 0.f;
              c += kWave;
              while (c >= HS) { c -= HS; ++r; }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (idx0 + u * kWave < total) nt_store(dst + idx0 + u * kWave, v[u]);
          }
        }
      }
      rollout_post(&obs_ready, lane);  // the histories of step s + 1 are in LDS
    }
    PDS_ENV_WAVE_END(RolloutHistArgs, 212)
    return;
  }

  // ================================ network waves: the actor for 16 rows of the tile each ========================
  const int own = wave * 16 + n16;  // this lane's sample row
  const bool own_ok = own < rows;
  const long long env_own = t * kWave + own;
  for (int s = 0; s < T; ++s) {
    const RolloutHistArgs &rl = *reinterpret_cast<const RolloutHistArgs *>(&reload_args<213, true>(ra.s, s));
    const long long o1 = (long long)s * rl.s.n;
    f32x4 x_own[HN];
    PDS_DRAW_ACTION_NOISE(rl, g == 0, call0 + (unsigned long long)s + 1ull, env_own, d_out)
    rollout_wait_ge(&obs_ready, s);  // the histories of step s are in LDS
    gather_hist<HN>(hist + own * S1, HS, mus, iss, g, x_own);
    PDS_FORWARD16_WIDE(rl.pi, mu)
    if (g == 0) PDS_EMIT_ACTION(rl, mu, d_out, act_all[own], o1 + env_own, own_ok);  // lane n16 owns sample `own`: outputs 0..3 of the actor
    rollout_post(&act_ready, lane);  // this wave is done with the histories of step s
  }
}

// ---- flags -> variant and input width, ONCE for both history kernels.  `l` is the kernel's launcher object (grid, s, args);
// `l.template run<Variant, HN>()` launches. ----
// hn = rollout_hist_tiles(H half): the input widths the kernels are instantiated for
template <class RV_, class L>
inline void hist_width(int hn, const L &l) {
  if (hn == 4) l.template run<RV_, 4>();
  else if (hn == 6) l.template run<RV_, 6>();
  else if (hn == 8) l.template run<RV_, 8>();
  else l.template run<RV_, 12>();
}
// {lean, reference-default noise} x {with, without motor dynamics; TakeOff: without}.  CTRL 0: control_mode PWM
// (csrc/pds_{rollout,evaluate}_hist_<task>.hip); 1 / 2: AttitudeRate / Attitude, the PID state in the env wave's registers like the
// rest of the env (csrc/pds_{rollout,evaluate}_hist_<task>_pid.hip, translation units of their own)
template <int TASK, int CTRL, class L>
inline bool hist_task(const LaunchFlags &f, int hn, const L &l) {
  static_assert(CTRL == 0 || TASK != PDS_TASK_TAKEOFF, "TakeOff fixes control_mode PWM (envs/takeoff.py:225)");
  if (!rollout_hist_supported(TASK, f) || f.ctrl != CTRL) return false;
  const bool full = f.on;
  if constexpr (TASK != PDS_TASK_TAKEOFF) {
    if (f.motor) {
      if (full) hist_width<Variant<TASK, true, true, false, true, true, CTRL, false, false>>(hn, l);
      else hist_width<Variant<TASK, true, false, false, false, false, CTRL, false, false>>(hn, l);
      return true;
    }
  }
  if (full) hist_width<Variant<TASK, false, true, false, true, true, CTRL, false, false>>(hn, l);
  else hist_width<Variant<TASK, false, false, false, false, false, CTRL, false, false>>(hn, l);
  return true;
}
template <int TASK, class L>
inline bool hist_pid(const LaunchFlags &f, int hn, const L &l) {
  if (f.ctrl == 1) return hist_task<TASK, 1>(f, hn, l);
  return hist_task<TASK, 2>(f, hn, l);
}
// ... and on the latency ring (LAT = true: rollout_hist_latency_supported; csrc/pds_rollout_hist_<task>[_pid]_lat.hip).  Hover and
// Circle only, both with motor dynamics in both noise settings.
template <int TASK, int CTRL, class L>
inline bool hist_lat_task(const LaunchFlags &f, int hn, const L &l) {
  static_assert(TASK != PDS_TASK_TAKEOFF, "TakeOff on the latency ring steps per step");
  if (!rollout_hist_latency_supported(TASK, f) || f.ctrl != CTRL) return false;
  if (f.motor) {
    if (f.on) hist_width<Variant<TASK, true, true, false, true, true, CTRL, true, false>>(hn, l);
    else hist_width<Variant<TASK, true, false, false, false, false, CTRL, true, false>>(hn, l);
  } else {
    if (f.on) hist_width<Variant<TASK, false, true, false, true, true, CTRL, true, false>>(hn, l);
    else hist_width<Variant<TASK, false, false, false, false, false, CTRL, true, false>>(hn, l);
  }
  return true;
}
template <int TASK, class L>
inline bool hist_lat_pid(const LaunchFlags &f, int hn, const L &l) {
  if (f.ctrl == 1) return hist_lat_task<TASK, 1>(f, hn, l);
  return hist_lat_task<TASK, 2>(f, hn, l);
}
struct RolloutHistLaunch {
  dim3 grid;  // one block per 64-env tile
  hipStream_t s;
  const RolloutHistArgs &args;
  template <class RV_, int HN>
  void run() const { hipLaunchKernelGGL((rollout_hist_kernel<RV_, HN>), grid, dim3(kRolloutThreads), 0, s, args); }
};

}  // namespace pds
