// pds_collect.h -- ONE launch collects K vector steps of an off-policy trainer into its replay ring (gfx950):
//     o -> actor -> exploration action -> env.step(a) -> (o, a, r, o', d) into the ring rows the update kernels read in place
// of OffPolicyTrainer.step_env + the episode bookkeeping of learn_one_epoch (ddpg.py; the reference's roll_out,
// algs/ddpg/ddpg.py:393-429, algs/sac/sac.py:402-437).  It is the off-policy counterpart of rollout_kernel (csrc/pds_rollout.h)
// and keeps its wave roles -- per 64-env tile four network waves on forward16_shape (csrc/pds_mlp_fwd.h: the code path of
// pds_mlp_forward, same bits) and one env wave on step_once (csrc/pds_step.h: the code path of pds_step, same bits) with the env
// state in registers, LDS counters between them -- without what collection does not need: no critic, no log-probability, no
// [T, N] buffers, no atomics.  Two exploration rules (csrc/pds_explore.h, the device functions of pds_ddpg_explore and
// pds_sac_sample): DDPG a = clamp(fma(exp(log_std), z, limit tanh(net)), +-limit), SAC the squashed-Gaussian sample of the
// head row [mu | log_std]; z of step s = the variates of pds_gaussian_sample for sample id = env row in call first_call + s.
//
// Who stores what.  Step s fills ring block b(s) = (ptr + s N) mod capacity (ptr, capacity multiples of N: no block straddles
// the wrap).  A tile's 64 rows are one contiguous piece of each array; network wave w owns rows 16 w .. 16 w + 15 of the tile:
//   oa [b(s) + i]   = [o_i(s) | a_i]     network wave: its 16 (D + 4) floats gathered from the tile and its own action slots
//                                        BEFORE it posts act_ready, stored behind the post -- 16 B per lane, consecutive lanes
//                                        consecutive addresses (scalar stores for a partial tile or an unaligned piece)
//   obs2[b(s) + i]  = fin_i or o_i(s+1)  network wave, one step later: in front of step s + 1 the tile holds o(s + 1), `fin` the
//                                        last rows of the envs that finished in step s and done_all says which; stored behind
//                                        the post of step s + 1 (the pass s == K only does this and writes o(K) to d_obs)
//   rew, done[b(s) + i]                  env wave, from its registers, behind its obs_ready post (done = terminated & ~truncated)
//   state, clock, ep_ret / ep_len, d_tile_stats[tile][0..7]   env wave, behind the loop (PDS_ENV_WAVE_STORE)
// The env wave is the critical path of a step (7-14 us against 2-3 us of network work): it gets no store but its own two
// 256-byte rows, and those behind its post.
//
// Hand-over (rollout_wait_ge / rollout_post of csrc/pds_rollout.h; all five waves of a team are resident together).  Both loops
// are COUNTED: the env wave runs s = 0 .. K - 1, a network wave s = 0 .. K, neither has a data-dependent exit.
//   act_ready: +1 per network wave and step s < K, after the wave has read o(s), the `fin` rows and flags of step s - 1 and written
//              its 16 actions of step s.  The env wave waits for 4 (s + 1) in front of step s.
//   obs_ready: +1 by the env wave at the end of EVERY iteration s < K, after o(s + 1), `fin` and the flags are in LDS.  A network
//              wave waits for obs_ready >= s in front of pass s (s = 0: no wait, the prologue staged o(0) behind the block barrier).
//   Pairing: the env wave's wait of step s <- the four network waves' posts of pass s, which they reach after a wait for
//   obs_ready >= s <- the env wave's post of iteration s - 1 (s >= 1; none needed for s = 0).  A network wave's wait of pass
//   s <= K <- the env wave's post of iteration s - 1 <= K - 1, which it reaches after its wait of step s - 1 <- the posts of pass
//   s - 1.  By induction over s every wait has its post on every path: a network wave posts in every pass s < K whether or not
//   its 16 rows exist (partial tile: rows < 16 w + 1 -- it still computes and posts, its stores are bounded by `rows`), the env
//   wave posts in every iteration whether or not an env finished.  Pass K posts nothing and nobody waits for it.  A team whose
//   tile lies beyond the last one (odd tile count, two-team form) leaves behind the prologue with all five waves: teams share no
//   counter.
//   LDS images: tile, fin and done_all are written by the env wave between its act_ready wait and its obs_ready post and read
//   by the network waves between their obs_ready wait and their act_ready post; the action slots the other way round.
#pragma once
#include "pds_collect_args.h"
#include "pds_explore.h"
#include "pds_rollout.h"

namespace pds {

// A network wave's piece of a [*, W] row-major array: its 16 rows = 16 W contiguous floats, 4 W float4, F4 of them per lane.
template <int W>
constexpr int collect_piece_f4() { return (4 * W + kWave - 1) / kWave; }
// element (r, c) of the piece for r < 16, c < W from `src(r, c)`, in the piece's linear order: lane holds float4 it * 64 + lane
template <int W, class Src>
PDS_DEV void collect_gather_piece(float (&v)[4 * collect_piece_f4<W>()], int lane, Src src) {
#pragma unroll
  for (int it = 0; it < collect_piece_f4<W>(); ++it) {
    const int i4 = it * kWave + lane;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = 4 * i4 + j, r = e / W, c = e - r * W;
      v[4 * it + j] = (i4 < 4 * W) ? src(r, c) : 0.f;
    }
  }
}
// ... and out to `dst` (the piece's first float): float4 per lane where the piece is whole and 16-byte aligned (wave-uniform)
template <int W>
PDS_DEV void collect_store_piece(float *dst, const float (&v)[4 * collect_piece_f4<W>()], int lane, int rows) {
  const bool fast = rows == 16 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
#pragma unroll
  for (int it = 0; it < collect_piece_f4<W>(); ++it) {
    const int i4 = it * kWave + lane;
    if (i4 < 4 * W) {
      if (fast) {
        reinterpret_cast<float4 *>(dst)[i4] = make_float4(v[4 * it], v[4 * it + 1], v[4 * it + 2], v[4 * it + 3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * i4 + j;
          if (e < rows * W) dst[e] = v[4 * it + j];
        }
      }
    }
  }
}

template <class V_, int TEAMS>
__global__ __launch_bounds__(kRolloutThreads * TEAMS, 1) void collect_kernel(const CollectArgs ra) {
  using namespace pds_mlpf;
  using V = std::conditional_t<regen_obs_variant<V_>(), StoredOh<V_>, V_>;
  constexpr int D = V::D;
  constexpr int TS = tile_stride<D>();
  constexpr int NIN = (D + 15) / 16;
  constexpr int RM = merged_reset_variant<V>() ? RM_MERGED : RM_INLINE;
  constexpr int kScratchU4_ = (RM == RM_MERGED) ? kMergedScratchU4 : (inline_coop_variant<V>() ? inline_envs<V, false>() * scratch_stride<V>() : 0);
  static_assert(D <= 64, "network input <= 64 features");
  __shared__ __attribute__((aligned(16))) float net_pi[kNetFloats];
  __shared__ __attribute__((aligned(16))) float mus[64], iss[64];  // no standardisation: 0 and 1 (gather_input: (v - 0) * 1 = v)
  __shared__ __attribute__((aligned(16))) float tile_all[TEAMS][kWave * TS];
  __shared__ __attribute__((aligned(16))) float fin_all[TEAMS][kWave * D];
  __shared__ __attribute__((aligned(16))) float4 act_all[TEAMS][kWave];
  __shared__ uint32_t done_all[TEAMS][kWave];
  __shared__ uint32_t queue_all[TEAMS][kQueueCap];
  __shared__ U4 scratch_all[TEAMS][kScratchU4_ > 0 ? kScratchU4_ : 1];
  __shared__ int obs_ready[TEAMS], act_ready[TEAMS];
#ifdef PDS_STAMPS
  unsigned long long stamp_[kStampSlots];
#endif
  prefetch_kernargs();
  const StepArgs &a = ra.s;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int team = __builtin_amdgcn_readfirstlane(tid / kRolloutThreads);                   // wave-uniform
  const int wave = __builtin_amdgcn_readfirstlane((tid - team * kRolloutThreads) >> 6);     // wave within its team
  const bool is_env = wave >= kRolloutMlpWaves;
  constexpr int kThreads = kRolloutThreads * TEAMS;
  const int n16 = lane & 15, g = lane >> 4;
  const NetLds wpi = net_lds(net_pi);
  const long long ntiles = (a.n + kWave - 1) / kWave;
  const long long tile0 = (long long)blockIdx.x * TEAMS;  // first 64-env tile of this block
  const int T = ra.K;
  auto tile_rows = [&](int j) -> int {  // envs of tile j of this block (0: the last block of an odd tile count)
    const long long tt = tile0 + j;
    if (tt >= ntiles) return 0;
    const long long rem = a.n - tt * kWave;
    return rem >= kWave ? kWave : (int)rem;
  };

  // ---- prologue: the actor and o(0) into LDS ---------------------------------------------------------------------------
  stage_net(ra.pi, wpi, tid, kThreads);
  if (tid < 64) { mus[tid] = 0.f; iss[tid] = 1.f; }
  if (tid < TEAMS) { obs_ready[tid] = 0; act_ready[tid] = 0; }
#pragma unroll
  for (int j = 0; j < TEAMS; ++j) {
    const int rows = tile_rows(j);
    for (int idx = tid; idx < kWave * D; idx += kThreads) {
      const int r = idx / D, c = idx - r * D;
      tile_all[j][r * TS + c] = (r < rows) ? ra.obs[((tile0 + j) * kWave + r) * D + c] : 0.f;
    }
    if (tid < kWave) done_all[j][tid] = 0u;
  }
  __syncthreads();  // (the only block barrier: from here on the roles meet through the counters)
  const long long t = tile0 + team;
  if (t >= ntiles) return;  // (all five waves of a team without a tile)

  if (is_env) {
    // ================================ env wave: the tile's 64 envs in registers =================================
#if PDS_ROLLOUT_ENV_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ENV_PRIO);  // the env wave's instructions before its SIMD-mates' (network waves)
#endif
    const long long wave_base = t * kWave;
    const long long rem_ = a.n - wave_base;
    const bool active = rem_ >= kWave || lane < (int)rem_;
    const Idx<V> ix{wave_base, active ? (uint32_t)lane : (uint32_t)rem_ - 1u};
    float *tile = tile_all[team], *fin = fin_all[team];
    PDS_ENV_WAVE_BEGIN
    float ep_ret = *at(ra.ep_ret, ix), ep_len = *at(ra.ep_len, ix);
    // the episodes that finished within the launch: learn_one_epoch's accumulators, per lane
    const float kInf = __builtin_inff();
    float c_n = 0.f, r_sum = 0.f, r_sq = 0.f, r_min = kInf, r_max = -kInf, l_sum = 0.f, l_min = kInf, l_max = -kInf;
    int qcount = 0;
    long long blk = ra.ptr;  // b(s), wave-uniform
    for (int s = 0; s < T; ++s) {
      const CollectArgs &rl = *reinterpret_cast<const CollectArgs *>(&reload_args<401, true>(ra.s, s));
      rollout_wait_ge(&act_ready[team], kRolloutMlpWaves * (s + 1));  // the network waves have read o(s) and written a(s)
      PDS_OPAQUE_STEP_COPIES
      PDS_SINK_ROW_OFFSET
      const float4 act = act_all[team][lane_s];
      StepOut so;
      step_once<V, kWave, RM, false>(rl.s, o1, rks, parity, nullptr, tile, nullptr, queue_all[team], scratch_all[team], lane_s,
                                     wave_base, ix, active, act, S, qcount, fin, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      // self.ep_ret += r; self.ep_len += 1; the accumulators; zero where done (learn_one_epoch, in its order)
      const bool dn = (so.done || so.trunc) && active;
      const float er = ep_ret + so.reward, el = ep_len + 1.f;
      if (dn) {
        c_n += 1.f; r_sum += er; r_sq += er * er; r_min = fminf(r_min, er); r_max = fmaxf(r_max, er);
        l_sum += el; l_min = fminf(l_min, el); l_max = fmaxf(l_max, el);
      }
      ep_ret = dn ? 0.f : er;
      ep_len = dn ? 0.f : el;
      done_all[team][lane] = dn ? 1u : 0u;  // obs2 of this step is the `fin` row
      rollout_post(&obs_ready[team], lane);  // o(s + 1) in the tile, the finished envs' last rows in `fin`, flags
      if (active) {
        *at(rl.rew + blk, ix) = so.reward;
        *at(rl.done + blk, ix) = (so.done && !so.trunc) ? 1.f : 0.f;
      }
      blk += rl.s.n;
      if (blk >= rl.capacity) blk -= rl.capacity;
    }
    PDS_ENV_WAVE_STORE(CollectArgs, 402)
    // the tile's eight statistics: butterfly over the lanes, a fixed order
    for (int d = 32; d >= 1; d >>= 1) {
      c_n += __shfl_xor(c_n, d); r_sum += __shfl_xor(r_sum, d); r_sq += __shfl_xor(r_sq, d); l_sum += __shfl_xor(l_sum, d);
      r_min = fminf(r_min, __shfl_xor(r_min, d)); r_max = fmaxf(r_max, __shfl_xor(r_max, d));
      l_min = fminf(l_min, __shfl_xor(l_min, d)); l_max = fmaxf(l_max, __shfl_xor(l_max, d));
    }
    if (lane == 0) {
      float *o = rl.tile_stats + t * kCollectStats;
      o[0] = c_n; o[1] = r_sum; o[2] = r_sq; o[3] = r_min; o[4] = r_max; o[5] = l_sum; o[6] = l_min; o[7] = l_max;
    }
    return;
  }

  // ================================ network waves: 16 rows of the tile each ====================================
  const int rows = tile_rows(team);
  const int own = wave * 16 + n16;  // this lane's sample row
  const int prows = rows - wave * 16 >= 16 ? 16 : (rows - wave * 16 > 0 ? rows - wave * 16 : 0);  // rows of this wave's pieces
  const long long row0 = t * kWave + wave * 16;  // first env row of this wave's pieces
  const long long env_own = t * kWave + own;
  const float *tile = tile_all[team], *fin = fin_all[team];
  const uint32_t *dflag = done_all[team];
  const float *acts = reinterpret_cast<const float *>(act_all[team]);
  long long blk = ra.ptr, blk_prev = ra.ptr;  // b(s), b(s - 1)
  for (int s = 0; s <= T; ++s) {  // s == T: only obs2 of the last step and o(K)
    const CollectArgs &rl = *reinterpret_cast<const CollectArgs *>(&reload_args<403, true>(ra.s, s));
    // the noise of step s depends on (env row, call) only: drawn while the env wave is still stepping
    f32x4 z = (f32x4)(0.f), lsd = (f32x4)(0.f);
    if (s < T && g == 0) {
      z = pds_explore::gaussian_draw4((unsigned long long)env_own, rl.first_call + (unsigned long long)s, rl.seed);
      if (rl.mode == kCollectDdpg) lsd = (f32x4){rl.log_std[0], rl.log_std[1], rl.log_std[2], rl.log_std[3]};
    }
    rollout_wait_ge(&obs_ready[team], s);  // o(s) and the outcome of step s - 1 are in LDS
    float v_o2[4 * collect_piece_f4<D>()], v_oa[4 * collect_piece_f4<D + 4>()], v_ob[4 * collect_piece_f4<D>()];
    if (s > 0 && prows > 0)
      collect_gather_piece<D>(v_o2, lane, [&](int r, int c) {
        const int rr = wave * 16 + r;
        return dflag[rr] != 0u ? fin[rr * D + c] : tile[rr * TS + c];
      });
    if (s == T && prows > 0) collect_gather_piece<D>(v_ob, lane, [&](int r, int c) { return tile[(wave * 16 + r) * TS + c]; });
    if (s < T) {
      f32x4 x_own[NIN];
      gather_input<NIN>(tile, TS, own, D, mus, iss, g, x_own);
      const f32x4 y = (rl.pi.activation == 0) ? forward16_shape<0, NIN>(wpi, rl.pi, x_own, n16, g) : forward16_shape<1, NIN>(wpi, rl.pi, x_own, n16, g);
      // lane group 0 holds outputs 0 .. 3 of sample `own`, group 1 outputs 4 .. 7 (SAC: log_std)
      f32x4 other;
#pragma unroll
      for (int q = 0; q < 4; ++q) other[q] = __shfl_xor(y[q], 16);
      if (g == 0) {
        f32x4 av;
        if (rl.mode == kCollectDdpg) {
          av = pds_explore::ddpg_explore(y, lsd, z, rl.act_limit);
        } else {
          const pds_explore::SacDraw d = pds_explore::sac_squash(y, other, z);
#pragma unroll
          for (int q = 0; q < 4; ++q) av[q] = rl.act_limit * d.th[q];
        }
        act_all[team][own] = make_float4(av[0], av[1], av[2], av[3]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // this wave's 16 action slots are written: its [o | a] rows are complete in LDS
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (prows > 0)
        collect_gather_piece<D + 4>(v_oa, lane, [&](int r, int c) {
          const int rr = wave * 16 + r;
          return c < D ? tile[rr * TS + c] : acts[rr * 4 + (c - D)];
        });
      rollout_post(&act_ready[team], lane);  // this wave is done with the tile, `fin` and the flags of step s - 1
      // ---- off the critical path: the env wave is stepping ----
      if (prows > 0) collect_store_piece<D + 4>(rl.oa + (blk + row0) * (D + 4), v_oa, lane, prows);
    }
    if (s > 0 && prows > 0) collect_store_piece<D>(rl.obs2 + (blk_prev + row0) * D, v_o2, lane, prows);
    if (s == T && prows > 0) collect_store_piece<D>(rl.obs + row0 * D, v_ob, lane, prows);
    blk_prev = blk;
    blk += rl.s.n;
    if (blk >= rl.capacity) blk -= rl.capacity;
  }
}

// grid.x = number of 64-env tiles; more tiles than CUs: two teams per block, where the two-team form of this variant fits
// (two_teams_fit, csrc/pds_rollout.h: read off the two code objects).
struct CollectLaunch {
  dim3 grid;
  hipStream_t s;
  const CollectArgs &args;
  template <class RV_>
  void run() const {
    if (grid.x > (unsigned)kRolloutTwoTeamsAbove && two_teams_fit<&collect_kernel<RV_, 1>, &collect_kernel<RV_, 2>>())
      hipLaunchKernelGGL((collect_kernel<RV_, 2>), dim3((grid.x + 1) / 2), dim3(2 * kRolloutThreads), 0, s, args);
    else
      hipLaunchKernelGGL((collect_kernel<RV_, 1>), grid, dim3(kRolloutThreads), 0, s, args);
  }
};

// flags -> variant: {lean, reference default} x {with, without motor dynamics; TakeOff: without} -- collect_env_supported().
// (Not fused_lean_or_full<TASK, 0, false> of csrc/pds_rollout.h, whose rows these are: that table decides on f.motor itself, so for
// TakeOff it would instantiate two motor-dynamics variants in both team forms that collect_env_supported() never admits.)
template <int TASK, bool MOTOR>
inline bool collect_lean_or_full(const LaunchFlags &f, const CollectLaunch &l) {
  if (f.dr && f.tn && f.on) l.template run<Variant<TASK, MOTOR, true, false, true, true, 0, false, false>>();
  else l.template run<Variant<TASK, MOTOR, false, false, false, false, 0, false, false>>();
  return true;
}
template <int TASK>
inline bool launch_collect_task(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) {
  if (!collect_env_supported(TASK, f)) return false;
  const CollectLaunch l{grid, s, ca};
  if constexpr (TASK != PDS_TASK_TAKEOFF) {
    if (f.motor) return collect_lean_or_full<TASK, true>(f, l);
  }
  return collect_lean_or_full<TASK, false>(f, l);
}

// ---- the PID control modes and the latency ring (pds_collect_control, include/pds_collect_control.h) ----
// The same kernel text: CTRL and LAT are parameters of the variant, and everything they add lives in the env wave.  The PID state
// (rate and attitude integrals and last errors) is part of EnvState: loaded once by PDS_ENV_WAVE_BEGIN, carried in registers over
// the K steps, zeroed in place where step_once resets a finished env (control.reset()), stored behind the loop by
// PDS_ENV_WAVE_STORE.  The delayed-action ring [lat_steps, N] float4 stays in memory as in every other kernel on step_once; what
// the env wave carries of it is its index (in the counter word).  Per sub-step it reads the row the index points at -- the PWM or
// the PID targets come from that delayed action -- and overwrites it with `act`, the exploration action the network waves handed
// over (after the rule's clamp); a finished env's rows are redrawn in place (lat_normals4).  Reward, the observation's action
// entries and `oa` take the action the policy chose, not the delayed one.  Rows of the table: fused_lean_or_full<TASK, CTRL, LAT>
// of csrc/pds_rollout.h ({lean, reference default} x {with, without motor dynamics}), Hover and Circle --
// collect_control_env_supported().  One translation unit per family keeps the build parallel.
template <int TASK>
inline bool launch_collect_pid(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) {  // a PID mode, no ring
  if (!collect_control_env_supported(TASK, f) || f.lat || f.ctrl == 0) return false;
  const CollectLaunch l{grid, s, ca};
  if (f.ctrl == 1) return fused_lean_or_full<TASK, 1, false>(f, l);
  return fused_lean_or_full<TASK, 2, false>(f, l);
}
template <int TASK>
inline bool launch_collect_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) {  // control_mode PWM on the ring
  if (!collect_control_env_supported(TASK, f) || !f.lat || f.ctrl != 0) return false;
  return fused_lean_or_full<TASK, 0, true>(f, CollectLaunch{grid, s, ca});
}
template <int TASK>
inline bool launch_collect_pid_lat(const LaunchFlags &f, dim3 grid, hipStream_t s, const CollectArgs &ca) {  // a PID mode on the ring
  if (!collect_control_env_supported(TASK, f) || !f.lat || f.ctrl == 0) return false;
  const CollectLaunch l{grid, s, ca};
  if (f.ctrl == 1) return fused_lean_or_full<TASK, 1, true>(f, l);
  return fused_lean_or_full<TASK, 2, true>(f, l);
}

}  // namespace pds
