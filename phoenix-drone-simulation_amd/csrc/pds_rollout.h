// pds_rollout.h -- ONE launch per rollout (gfx950): the T closed-loop steps
//     o -> standardise -> actor MLP -> a = mu + sigma z, log p -> critic V(o) -> env.step(a) -> buffers
// of the caller's roll_out (algs/iwpg/iwpg.py:350-385, ActorCritic.step algs/core.py:370-393), the env state in
// registers for the whole rollout (like pds_step_k), the observation tile in LDS between the env step and the
// networks, both networks' weights in LDS.
//
// Round 2 ran a rollout step as 7 launches (critic, actor, sample, env step, V(final_obs), record, + copies), replayed
// from a hipGraph: 63 us per step at 8 192 envs, i.e. launch-bound (the env step itself is 7 us).
// Round 3 gave every 64-env tile one 256-thread block whose four waves ran the networks, then WAITED while wave 0
// stepped the envs, then evaluated V(final_obs): 17 us per step, 7.5 of them one wave's env step with three waves idle
// at the barrier, and one tile per CU (101 KB of LDS, most of it the two weight images).
//
// Round 4 -- wave roles, no block barrier inside the loop.  320 threads per tile:
//   M0..M3 (network waves, rows 16 w .. 16 w + 15, v_mfma_f32_16x16x4_f32 through csrc/pds_mlp_fwd.h -- the code path of
//           pds_mlp_forward, same bits):   wait for o(t) -> read their rows into registers -> actor -> sample ->
//           action into LDS, SIGNAL; then, while the env wave steps: the critic V(o(t)) and V(final_obs) of the envs that
//           finished in step t - 1;
//   E      (wave 4: the 64 envs of the tile in registers, step_once of csrc/pds_step.h -- the code path of pds_step /
//           pds_step_k, same bits):  wait for the four action signals -> env.step -> o(t + 1), the finished
//           envs' last rows and flags into LDS, SIGNAL.
// Only the actor is on the critical path of a step (action -> env step -> next observation); the critic, the TimeLimit
// bootstrap V(final_obs) (algs/iwpg/iwpg.py:375-385), the action-noise draws of the NEXT step and all buffer writes of
// the network waves run while the env wave steps.  Measured and kept out: the critic as one pds_mlp_forward over
// obs_buf after the kernel (0.97 vs 0.91 ms at 8 192 x 64), the actor's weight operands resident in registers
// (a forward16 that keeps its 29 b128 weight operands in 116 registers: no change, 14.0 us per step either way -- the pass is a dependent chain of
// 110 MFMAs + epilogues, not LDS-bound).
// Waves w and w + 4 of a block share a SIMD (profiles/r03_mlp_microbench.txt), and a wave that
// streams MFMAs halves the vector-ALU rate of its SIMD-mate (a first version with two tiles per block, every env wave
// next to a busy network wave: 23 us per step against 17.7 for round 3's kernel), so M0 -- the env wave's mate -- only
// works while E waits: its rows' critic pass is taken by M1, their V(final_obs) by M2.
// Hand-over through monotonic counters in LDS (release / acquire, s_sleep loop; all five waves of a block are resident
// together, so the waits cannot deadlock); every LDS image has exactly one writer role, and every reader finishes with
// it before it posts the signal its writer waits for.
//
// Envs are independent, the policy is frozen during a rollout and the running observation statistics are only
// updated after it (ppo.py), so a tile needs nothing from another tile for all T steps.
#pragma once
#include "pds_mlp_fwd.h"
#include "pds_step.h"

namespace pds {

#ifndef PDS_ROLLOUT_TWO_TEAMS_ABOVE
#define PDS_ROLLOUT_TWO_TEAMS_ABOVE 256  // tiles (one per CU)
#endif
constexpr int kRolloutTwoTeamsAbove = PDS_ROLLOUT_TWO_TEAMS_ABOVE;
// Network wave 0 shares its SIMD with the env wave.  Where the env wave's step is long (observation noise: 20 k cycles per step,
// 14 k of them the in-place reset of the finished envs) wave 0 stays quiet while it runs and waves 1 / 2 take its critic
// passes; where it is short (lean variants: 8 k cycles) the network waves' shadow work is what bounds the step, and wave 0
// does its own share (same box, 8 192 x 64 lean: 0.91 -> 0.76 ms; default config 0.96 -> 1.05 the other way;
// profiles/r04_rollout_timing.txt).
#ifndef PDS_ROLLOUT_M0_QUIET
#define PDS_ROLLOUT_M0_QUIET (V::ON)
#endif
#ifndef PDS_ROLLOUT_ENV_PRIO
#define PDS_ROLLOUT_ENV_PRIO 3
#endif
#ifndef PDS_ROLLOUT_ACTOR_PRIO
#define PDS_ROLLOUT_ACTOR_PRIO 0
#endif
#ifndef PDS_ROLLOUT_SKIP
#define PDS_ROLLOUT_SKIP 0  // profiling builds only: 1 = no actor / critic passes, 2 = no env step, 4 = no V(final_obs)
#endif
constexpr int kRolloutMlpWaves = 4;               // network waves per block (16 rows of the tile each)
constexpr int kRolloutTeamWaves = kRolloutMlpWaves + 1;    // + the env wave: one TEAM per 64-env tile
constexpr int kRolloutThreads = kWave * kRolloutTeamWaves;  // threads per team

// network input of this lane: features 16 kt + 4 g + q of row `r` of an LDS image with row stride `stride`
template <int NIN>
PDS_DEV void gather_input(const float *img, int stride, int r, int d_in, const float *mus, const float *iss, int g,
                          pds_mlpf::f32x4 (&xin)[NIN]) {
#pragma unroll
  for (int kt = 0; kt < NIN; ++kt) {
    const int k0 = kt * 16 + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + q;
      const float mu = mus[k], is = iss[k];  // (16 NIN <= 64)
      const float v = (k < d_in) ? img[r * stride + k] : mu;
      xin[kt][q] = (v - mu) * is;  // (pds_mlp.hip: (v - mu) * (1 / (std + eps)); padding features 0)
    }
  }
}

// hand-over counters (LDS, monotonic)
PDS_DEV void rollout_wait_ge(int *flag, int need) {
  while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < need)
    __builtin_amdgcn_s_sleep(1);
}
PDS_DEV void rollout_post(int *flag, int lane) {  // +1, after every lane's LDS accesses of this phase
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0) __hip_atomic_fetch_add(flag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- the env wave's prologue, episode bookkeeping and epilogue, for both rollout kernels (PDS_NEXT_TICK: csrc/pds_step.h).  Macros
// that expand to the statements the kernels had, over the kernels' own locals (a, ra, ix, t, active, T, lane; ep_ret, ep_len: running
// return and length of this lane's env; st0-2: return, length and count of the episodes that finished): as forced-inline functions
// over a struct the bookkeeping cost two Circle rollout_hist_kernels a VGPR (profiles/rollout_refactor_resources.txt). ----
// The env state of tile `t` into registers, in front of the loop: declares cur, rk (the key of the current tick), parity, rk0 (the
// key of the first tick, for advance_clock behind the loop) and S.
#define PDS_ENV_WAVE_BEGIN                                                   \
  Loaded cur;                                                                \
  RngKey rk{a.seed_lo, a.seed_hi, 0u, 0u};                                   \
  load_env<V>(a, ix, t, cur);                                                \
  rk.tick_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.clk.x);     \
  rk.tick_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.clk.y);     \
  int parity = __builtin_amdgcn_readfirstlane((int)cur.clk.z) & 1;           \
  const RngKey rk0 = rk;                                                     \
  EnvState S;                                                                \
  unpack_state<V>(a.k, cur, parity, S);                                      \
  init_kept_obs<V>(a, rk, ix, S);
// pds_rollout_record (csrc/pds_train.hip record_kernel) for this lane's env; declares dn: the env finished in this step
#define PDS_RECORD_STEP(so)                                   \
  const bool dn = (so.done || so.trunc) && active;            \
  const float er = ep_ret + so.reward, el = ep_len + 1.f;     \
  if (dn) { st0 += er; st1 += el; st2 += 1.f; }               \
  ep_ret = dn ? 0.f : er;                                     \
  ep_len = dn ? 0.f : el;
// Behind the loop: state, running return / length and the tile's clock back to memory (PDS_ENV_WAVE_STORE: what every kernel
// with an env wave ends on, csrc/pds_collect.h too), the finished episodes' sums into stats[0..2] (one atomic triple per
// tile).  RA: the kernel's argument struct, ID: its reload_args tag.
#define PDS_ENV_WAVE_STORE(RA, ID)                                                                                            \
  const RA &rl = *reinterpret_cast<const RA *>(&reload_args<ID, true>(ra.s, T));                                              \
  if (active) {                                                                                                               \
    store_state<V>(rl.s, ix, parity, S, true);                                                                                \
    *at(rl.ep_ret, ix) = ep_ret;                                                                                              \
    *at(rl.ep_len, ix) = ep_len;                                                                                              \
  }                                                                                                                           \
  advance_clock(rl.s.st.clk, t, rk0, parity, (uint32_t)T, lane);
#define PDS_ENV_WAVE_END(RA, ID)                                                                                              \
  PDS_ENV_WAVE_STORE(RA, ID)                                                                                                  \
  for (int d = 32; d >= 1; d >>= 1) { st0 += __shfl_xor(st0, d); st1 += __shfl_xor(st1, d); st2 += __shfl_xor(st2, d); }      \
  if (lane == 0 && st2 != 0.f) {                                                                                              \
    atomicAdd(rl.stats + 0, st0);                                                                                             \
    atomicAdd(rl.stats + 1, st1);                                                                                             \
    atomicAdd(rl.stats + 2, st2);                                                                                             \
  }

// In front of step_once, every kernel with an env wave (csrc/pds_evaluate.h, pds_collect.h, both rollout kernels): opaque
// per-iteration copies of the seed and the lane index -- see step_k_kernel: their loop-invariant derivatives would otherwise be
// formed in the loop header and spilled.  Reads rk and lane; declares rks and lane_s.
#define PDS_OPAQUE_STEP_COPIES                                                             \
  RngKey rks = rk;                                                                         \
  int lane_s = lane;                                                                       \
  asm volatile("" : "+s"(rks.seed_lo), "+s"(rks.seed_hi), "+v"(lane_s));
// The kernels whose per-step streams all go to the SAME sink row (evaluation, collection): offset 0, but opaque -- step_once renews
// its late views of the kernel arguments per iteration by this offset (reload_args' tag); a constant would hoist them out of the
// loop, into registers.  Declares o1.
#define PDS_SINK_ROW_OFFSET \
  long long o1 = 0;         \
  asm volatile("" : "+s"(o1));

// ---- the network waves' sampling (both rollout kernels): ActorCritic.step's dist.sample() + log_prob().sum(-1), the
// values of pds_gaussian_sample (csrc/pds_train.hip sample_kernel; draw and log-probability term: csrc/pds_device.h) ----
// (Macros again: as forced-inline functions -- arrays by reference or a struct by value, either of the two alone -- they moved the
// register allocation of every TakeOff rollout_hist_kernel, profiles/rollout_refactor_resources.txt.)
// PDS_DRAW_ACTION_NOISE declares z[4] (standard normals; 0 where deterministic), lsd[4] = log_std and sig[4] = exp(log_std) of
// the lanes with `live`.  The noise of step s depends on (env, call) only: drawn while the env wave is still stepping.
#define PDS_DRAW_ACTION_NOISE(rl, live, call_, env, d_out)                                                    \
  float z[4] = {0.f, 0.f, 0.f, 0.f}, sig[4], lsd[4];                                                          \
  if (live) {                                                                                                 \
    if (!rl.deterministic) {                                                                                  \
      const unsigned long long gid = rl.s.env_id_base + (unsigned long long)env;                              \
      const unsigned long long call = call_;                                                                  \
      const U4 r = PDS_GAUSSIAN_PHILOX(gid, 0u, call, rl.seed);                                               \
      box_muller(r.x, r.y, z[0], z[1]);                                                                       \
      box_muller(r.z, r.w, z[2], z[3]);                                                                       \
    }                                                                                                         \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
      lsd[q] = (q < d_out) ? rl.log_std[q] : 0.f;                                                             \
      sig[q] = expf(lsd[q]);                                                                                  \
    }                                                                                                         \
  }
// a = mu + sigma z and its log-probability: the action into the env wave's LDS slot, both into row `row` of the buffers
#define PDS_EMIT_ACTION(rl, mu, d_out, slot, row, row_ok)                                                     \
  do {                                                                                                        \
    float av[4], lp = 0.f;                                                                                    \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
      av[q] = fmaf(sig[q], z[q], mu[q]);                                                                      \
      if (q < d_out) lp += PDS_GAUSSIAN_LOGP_TERM(z[q], lsd[q]);                                              \
    }                                                                                                         \
    slot = make_float4(av[0], av[1], av[2], av[3]);                                                           \
    if (row_ok) {                                                                                             \
      *reinterpret_cast<float4 *>(rl.act_buf + (row) * 4) = make_float4(av[0], av[1], av[2], av[3]);          \
      rl.logp_buf[row] = lp;                                                                                  \
    }                                                                                                         \
  } while (0)

// TEAMS: tiles (= teams of 4 network waves + 1 env wave) per block.  One team per block is the latency form (8 192 envs:
// 128 blocks on 256 CUs); with more tiles than CUs the network waves' idle time -- they work 5-9 of a step's 14 us -- is
// what a second team on the same CU fills: the two teams share nothing but the weight images (84 of the block's 124 KB
// of LDS) and the CU.  (Ten waves per CU = three per SIMD on two SIMDs: the 168-register cap, which the env wave only
// meets because it reads the kept noisy observation from memory, StoredOh, like the K-step kernel.)
template <class V_, int TEAMS>
__global__ __launch_bounds__(kRolloutThreads * TEAMS, 1) void rollout_kernel(const RolloutArgs ra) {
  using namespace pds_mlpf;
  using V = std::conditional_t<regen_obs_variant<V_>(), StoredOh<V_>, V_>;
  constexpr int D = V::D;
  constexpr int TS = tile_stride<D>();
  constexpr int NIN = (D + 15) / 16;
  constexpr int RM = merged_reset_variant<V>() ? RM_MERGED : RM_INLINE;
  constexpr int kScratchU4_ = (RM == RM_MERGED) ? kMergedScratchU4 : (inline_coop_variant<V>() ? inline_envs<V, false>() * scratch_stride<V>() : 0);
  static_assert(D <= 64, "network input <= 64 features");
  __shared__ __attribute__((aligned(16))) float net_pi[kNetFloats];
  __shared__ __attribute__((aligned(16))) float net_vf[kNetFloats];
  __shared__ __attribute__((aligned(16))) float mus[64], iss[64];
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
  const NetLds wpi = net_lds(net_pi), wvf = net_lds(net_vf);
  const long long ntiles = (a.n + kWave - 1) / kWave;
  const long long tile0 = (long long)blockIdx.x * TEAMS;  // first 64-env tile of this block
  const int T = ra.T;
  const int d_out = ra.pi.d_out;
  auto tile_rows = [&](int j) -> int {  // envs of tile j of this block (0: the last block of an odd tile count)
    const long long tt = tile0 + j;
    if (tt >= ntiles) return 0;
    const long long rem = a.n - tt * kWave;
    return rem >= kWave ? kWave : (int)rem;
  };

  // ---- prologue: networks, statistics and o(0) into LDS; env state into the env waves' registers --------------
  stage_net(ra.pi, wpi, tid, kThreads);
  stage_net(ra.vf, wvf, tid, kThreads);
  if (tid < 64) {
    const bool on = ra.mean != nullptr && tid < D;
    mus[tid] = on ? ra.mean[tid] : 0.f;
    iss[tid] = on ? 1.0f / (ra.stdv[tid] + ra.eps) : 1.f;
  }
  if (tid < TEAMS) { obs_ready[tid] = 0; act_ready[tid] = 0; }
#pragma unroll
  for (int j = 0; j < TEAMS; ++j) {
    const int rows = tile_rows(j);
    for (int idx = tid; idx < kWave * D; idx += kThreads) {
      const int r = idx / D, c = idx - r * D;
      tile_all[j][r * TS + c] = (r < rows) ? ra.obs0[((tile0 + j) * kWave + r) * D + c] : 0.f;
    }
    if (tid < kWave) done_all[j][tid] = 0u;
  }
  unsigned long long call0 = ra.call_offset;
  if (ra.call_base != nullptr) call0 += *ra.call_base;
  __syncthreads();  // (the only block barrier: from here on the roles meet through the counters)

  if (is_env) {
    // ================================ env wave: one tile's 64 envs in registers =================================
    const int grp = team;
#if PDS_ROLLOUT_ENV_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ENV_PRIO);  // the env wave's instructions before its SIMD-mates' (network waves)
#endif
    const long long t = tile0 + grp;
    if (t >= ntiles) return;
    const long long wave_base = t * kWave;
    const long long rem_ = a.n - wave_base;
    const bool active = rem_ >= kWave || lane < (int)rem_;
    const Idx<V> ix{wave_base, active ? (uint32_t)lane : (uint32_t)rem_ - 1u};
    float *tile = tile_all[grp], *fin = fin_all[grp];
    PDS_ENV_WAVE_BEGIN
    float ep_ret = *at(ra.ep_ret, ix), ep_len = *at(ra.ep_len, ix), st0 = 0.f, st1 = 0.f, st2 = 0.f;
    int qcount = 0;
#ifdef PDS_ROLLOUT_TIMING
    unsigned long long tw = 0, ts = 0, tp = 0, tph = 0, tout = 0, trst = 0, tfin = 0, tev = 0, tfill = 0, teval = 0;
#endif
    for (int s = 0; s < T; ++s) {
      const RolloutArgs &rl = *reinterpret_cast<const RolloutArgs *>(&reload_args<201, true>(ra.s, s));
      const long long o1 = (long long)s * rl.s.n;
#ifdef PDS_ROLLOUT_TIMING
      const unsigned long long q0 = __builtin_amdgcn_s_memtime();
#endif
      rollout_wait_ge(&act_ready[grp], kRolloutMlpWaves * (s + 1));  // the network waves have read o(s) and written a(s)
#ifdef PDS_ROLLOUT_TIMING
      const unsigned long long q1 = __builtin_amdgcn_s_memtime();
#endif
      if (!(PDS_ROLLOUT_SKIP & 2)) {
        PDS_OPAQUE_STEP_COPIES
        const float4 act = act_all[grp][lane_s];
        StepOut so;
#ifdef PDS_STAMPS_RESET
        stamp_[8] = 0; stamp_[9] = 0;
#endif
        step_once<V, kWave, RM, false>(rl.s, o1, rks, parity, nullptr, tile, nullptr, queue_all[grp], scratch_all[grp], lane_s,
                                       wave_base, ix, active, act, S, qcount, fin, &so PDS_STAMP_ARG);
        PDS_NEXT_TICK(rk, parity)
        PDS_RECORD_STEP(so)
        // V(final_obs) is the bootstrap of an episode the TimeLimit cut (algs/iwpg/iwpg.py:374-379: also when it terminated
        // on the same step); one that only terminated bootstraps with 0 and pds_gae never reads its fval entry: only the
        // truncated envs ask the network waves for a pass (a young policy ends ~5 % of its episodes per step, nearly all of
        // them by termination).  The LAST step of the rollout hands over every finished env: a caller that mirrors the
        // reference's epoch-end cut (`epoch_ended` takes V(o) for a terminated path too; ppo.py reset_each_rollout) reads it.
        // (`want` of rollout_hist_kernel is this rule, dn && (trunc || last step); each kernel keeps its wording: in the
        //  other's, 20 of 24 Hover latency-ring kernels here and 12 of 16 Circle kernels there change their SGPR spills.)
        done_all[grp][lane] = ((so.trunc || (so.done && s == T - 1)) && active) ? 1u : 0u;
      }
#ifdef PDS_ROLLOUT_TIMING
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const unsigned long long q2 = __builtin_amdgcn_s_memtime();
#endif
      rollout_post(&obs_ready[grp], lane);  // o(s + 1) in the tile, the finished envs' last rows in `fin`, flags
#ifdef PDS_ROLLOUT_TIMING
      const unsigned long long q3 = __builtin_amdgcn_s_memtime();
      tw += q1 - q0; ts += q2 - q1; tp += q3 - q2;
#ifdef PDS_STAMPS
      if (!(PDS_ROLLOUT_SKIP & 2)) { tph += stamp_[3] - q1; tout += stamp_[4] - stamp_[3]; trst += stamp_[5] - stamp_[4]; tfin += stamp_[6] - stamp_[4]; tev += stamp_[7] - stamp_[6]; }
#ifdef PDS_STAMPS_RESET
      tfill += stamp_[8]; teval += stamp_[9];
#endif
#endif
#endif
    }
#ifdef PDS_ROLLOUT_TIMING
    if (blockIdx.x == 0 && team == 0 && lane == 0) { ra.stats[8] = (float)tw / T; ra.stats[9] = (float)ts / T; ra.stats[10] = (float)tp / T;
      ra.stats[11] = (float)tph / T; ra.stats[12] = (float)tout / T; ra.stats[13] = (float)trst / T; ra.stats[14] = (float)tfin / T; ra.stats[15] = (float)tev / T; ra.stats[48] = (float)tfill / T; ra.stats[49] = (float)teval / T; }
#endif
    PDS_ENV_WAVE_END(RolloutArgs, 202)
    return;
  }

  // ================================ network waves: 16 rows of the tile each ====================================
  // rows 16 w .. 16 w + 15 are wave w's; the critic of wave 0's rows runs on wave 1 and their V(final_obs) on wave 2
  // (wave 0 shares its SIMD with the env wave: it only works while that one waits).
  const int j = team;
  const int rows = tile_rows(j);
  if (rows == 0) return;  // (the last block of an odd tile count: this team has no env wave to wait for)
  const int own = wave * 16 + n16;  // this lane's sample row
  const bool own_ok = own < rows, r0_ok = n16 < rows;
  const long long env_own = (tile0 + j) * kWave + own, env_r0 = (tile0 + j) * kWave + n16;
#ifdef PDS_ROLLOUT_TIMING
  unsigned long long mw = 0, mg = 0, ma = 0, mp = 0, mc = 0, mpre = 0;
#endif
  for (int s = 0; s <= T; ++s) {  // s == T: only V(o(T)) and the last step's V(final_obs)
#ifdef PDS_ROLLOUT_TIMING
    const unsigned long long r00 = __builtin_amdgcn_s_memtime();
#endif
    const RolloutArgs &rl = *reinterpret_cast<const RolloutArgs *>(&reload_args<203, true>(ra.s, s));
    const long long o1 = (long long)s * rl.s.n;
    f32x4 x_own[NIN], x_r0[NIN], f_own[NIN], f_r0[NIN];
    PDS_DRAW_ACTION_NOISE(rl, s < T && g == 0, call0 + (unsigned long long)s + 1ull, env_own, d_out)
#ifdef PDS_ROLLOUT_TIMING
    const unsigned long long r0 = __builtin_amdgcn_s_memtime();
#endif
    rollout_wait_ge(&obs_ready[j], s);  // o(s) and the outcome of step s - 1 are in LDS
#ifdef PDS_ROLLOUT_TIMING
    const unsigned long long r1 = __builtin_amdgcn_s_memtime();
#endif
#if PDS_ROLLOUT_ACTOR_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ACTOR_PRIO);  // the actor pass is on the step's critical path, the critic passes are not
#endif
    gather_input<NIN>(tile_all[j], TS, own, D, mus, iss, g, x_own);
    constexpr bool kQuiet = PDS_ROLLOUT_M0_QUIET;
    if (kQuiet && wave == 1) gather_input<NIN>(tile_all[j], TS, n16, D, mus, iss, g, x_r0);
    const bool skip_fin = (PDS_ROLLOUT_SKIP & 4) != 0;
    const bool dn_own = done_all[j][own] != 0u;                                   // (step s - 1; zeros before the first step)
    const bool any_own = (wave != 0 || !kQuiet) && __ballot(dn_own) != 0ull && !skip_fin;      // wave-uniform: one of these 16 envs finished
    const bool dn_r0 = done_all[j][n16] != 0u;
    const bool any_r0 = kQuiet && wave == 2 && __ballot(dn_r0) != 0ull && !skip_fin;
    if (any_own) gather_input<NIN>(fin_all[j], D, own, D, mus, iss, g, f_own);
    if (any_r0) gather_input<NIN>(fin_all[j], D, n16, D, mus, iss, g, f_r0);
#ifdef PDS_ROLLOUT_TIMING
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long r2 = __builtin_amdgcn_s_memtime();
    unsigned long long r3 = r2, r4 = r2;
#endif
    if (s < T) {
      if (!(PDS_ROLLOUT_SKIP & 1)) {
        const f32x4 mu = (rl.pi.activation == 0) ? forward16_shape<0, NIN>(wpi, rl.pi, x_own, n16, g) : forward16_shape<1, NIN>(wpi, rl.pi, x_own, n16, g);
        if (g == 0) PDS_EMIT_ACTION(rl, mu, d_out, act_all[j][own], o1 + env_own, own_ok);  // lane n16 owns sample `own`: outputs 0..3 of the actor
      }
#ifdef PDS_ROLLOUT_TIMING
      r3 = __builtin_amdgcn_s_memtime();
#endif
      rollout_post(&act_ready[j], lane);  // this wave is done with the tile, `fin` and the flags of step s - 1
#ifdef PDS_ROLLOUT_TIMING
      r4 = __builtin_amdgcn_s_memtime();
#endif
    }
#if PDS_ROLLOUT_ACTOR_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    // ---- off the critical path: the env wave is stepping (wave 0, its SIMD-mate, stays quiet) ------------------
    auto critic = [&](const f32x4 (&x)[NIN]) -> float {
      const f32x4 v = (rl.vf.activation == 0) ? forward16_shape<0, NIN>(wvf, rl.vf, x, n16, g) : forward16_shape<1, NIN>(wvf, rl.vf, x, n16, g);
      return v[0];
    };
    if ((wave != 0 || !kQuiet) && !(PDS_ROLLOUT_SKIP & 1)) {
      const float v = critic(x_own);
      if (g == 0 && own_ok) {
        if (s < T) rl.val_buf[o1 + env_own] = v;
        else rl.last_val[env_own] = v;
      }
    }
    if (kQuiet && wave == 1 && !(PDS_ROLLOUT_SKIP & 1)) {
      const float v = critic(x_r0);
      if (g == 0 && r0_ok) {
        if (s < T) rl.val_buf[o1 + env_r0] = v;
        else rl.last_val[env_r0] = v;
      }
    }
    // V(final_obs) where an env finished in step s - 1 (the other rows of fval_buf are never read: pds_gae)
    if (any_own) {
      const float v = critic(f_own);
      if (g == 0 && dn_own && own_ok) rl.fval_buf[o1 - rl.s.n + env_own] = v;
    }
    if (any_r0) {
      const float v = critic(f_r0);
      if (g == 0 && dn_r0 && r0_ok) rl.fval_buf[o1 - rl.s.n + env_r0] = v;
    }
#ifdef PDS_ROLLOUT_TIMING
    const unsigned long long r5 = __builtin_amdgcn_s_memtime();
    if (s > 0 && s < T) { mpre += r0 - r00; mw += r1 - r0; mg += r2 - r1; ma += r3 - r2; mp += r4 - r3; mc += r5 - r4; }
#endif
  }
#ifdef PDS_ROLLOUT_TIMING
  // (diagnostic builds: the caller's `stats` must have room for 64 floats -- profiles/tools/rollout_timing.py)
  if (blockIdx.x == 0 && team == 0 && lane == 0) {
    float *o = ra.stats + 16 + 8 * wave;
    o[0] = (float)mpre / (T - 1); o[1] = (float)mw / (T - 1); o[2] = (float)mg / (T - 1); o[3] = (float)ma / (T - 1); o[4] = (float)mp / (T - 1); o[5] = (float)mc / (T - 1);
  }
#endif
}

// The variants the fused rollout is built for (rollout_supported in csrc/pds_types.h states the same rule for the host):
//   control_mode PWM, no latency ring, no Kalman hold: every combination of domain randomisation / thrust noise /
//     observation noise (the reference's ctor arguments are independent: envs/base.py:26-48) x {with, without motor dynamics};
//   the PID control modes (what the reference's exp-07 trains: experiments/07_control_structure_hypothesis/
//     run_control_structures.py:53-61, envs/control.py:120-287) and the latency ring (envs/agents.py:267-276), also together:
//     {lean, reference default (DR + thrust noise + observation noise)} x {with, without motor dynamics};
//   the Kalman hold (observation_frequency < sim_freq, envs/hover.py:134-156) with control_mode PWM: observation noise with
//     {none, both} of DR + thrust noise x {with, without motor dynamics};
//   the ground effect: TakeOff with control_mode PWM, every noise setting (round 6); nowhere else.
// `grid.x` = number of 64-env tiles; more tiles than CUs: two teams per block.
struct RolloutLaunch {
  dim3 grid;
  hipStream_t s;
  const RolloutArgs &args;
  template <class RV_>
  void run() const {
    if (grid.x > (unsigned)kRolloutTwoTeamsAbove)
      hipLaunchKernelGGL((rollout_kernel<RV_, 2>), dim3((grid.x + 1) / 2), dim3(2 * kRolloutThreads), 0, s, args);
    else
      hipLaunchKernelGGL((rollout_kernel<RV_, 1>), grid, dim3(kRolloutThreads), 0, s, args);
  }
};
// The other launchers of the fused family (EvalLaunchT csrc/pds_evaluate.h, CollectLaunch csrc/pds_collect.h) take the two-team
// form above the same tile count -- unless the two-team form of this variant spills where the one-team form does not.  One launch
// bound covers every wave of a block, so the ten waves of two teams get the env wave's registers cut to 168 (three waves per SIMD)
// where one team's five leave it 256; the observation-noise variants of the evaluation need 190-250 there
// (profiles/evaluate_kernel_resources.txt).  The rule is read off the code objects instead of being listed by hand: the two-team
// form `Two` is launched where it needs no more scratch memory per lane than the one-team form `One`.
template <auto One, auto Two>
inline bool two_teams_fit() {
  static const bool fit = [] {
    hipFuncAttributes one, two;
    if (hipFuncGetAttributes(&one, reinterpret_cast<const void *>(One)) != hipSuccess ||
        hipFuncGetAttributes(&two, reinterpret_cast<const void *>(Two)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return two.localSizeBytes <= one.localSizeBytes;
  }();
  return fit;
}

// ---- flags -> variant, family by family, ONCE for every kernel of the fused family (rollout_kernel, evaluate_kernel in its three
// forms; collect_kernel takes fused_lean_or_full): the configurations rollout_supported() names.  `l` is the kernel's launcher
// object (grid, s, args; `l.template run<Variant>()` launches). ----
// motor dynamics x {lean, full}
template <int TASK, int CTRL, bool LAT, class L>
inline bool fused_lean_or_full(const LaunchFlags &f, const L &l) {
  const bool lean = !f.dr && !f.tn && !f.on, full = f.dr && f.tn && f.on;
  if (!lean && !full) return false;
  if (f.motor) {
    if (full) l.template run<Variant<TASK, true, true, false, true, true, CTRL, LAT, false>>();
    else l.template run<Variant<TASK, true, false, false, false, false, CTRL, LAT, false>>();
  } else {
    if (full) l.template run<Variant<TASK, false, true, false, true, true, CTRL, LAT, false>>();
    else l.template run<Variant<TASK, false, false, false, false, false, CTRL, LAT, false>>();
  }
  return true;
}
// control_mode PWM without latency / hold: all eight noise settings (GE: the ground-effect extension, TakeOff only)
template <int TASK, bool MOTOR, bool GE, class L>
inline void fused_pwm(const LaunchFlags &f, const L &l) {
#define PDS_FUSED_CASE(DR, TN, ON) \
  if (f.dr == DR && f.tn == TN && f.on == ON) return l.template run<Variant<TASK, MOTOR, DR, GE, TN, ON, 0, false, false>>()
  PDS_FUSED_CASE(false, false, false); PDS_FUSED_CASE(true, true, true);
  PDS_FUSED_CASE(true, false, false); PDS_FUSED_CASE(false, true, false); PDS_FUSED_CASE(false, false, true);
  PDS_FUSED_CASE(true, true, false); PDS_FUSED_CASE(true, false, true); PDS_FUSED_CASE(false, true, true);
#undef PDS_FUSED_CASE
}
template <int TASK, bool MOTOR, class L>
inline bool fused_hold(const LaunchFlags &f, const L &l) {
  if (!f.on || f.dr != f.tn) return false;
  if (f.dr) l.template run<Variant<TASK, MOTOR, true, false, true, true, 0, false, true>>();
  else l.template run<Variant<TASK, MOTOR, false, false, false, true, 0, false, true>>();
  return true;
}
// The families are instantiated in translation units of their own (csrc/pds_{rollout,evaluate,evaluate_metrics,evaluate_stats}_
// <task>[_pwm|_lat].hip: the build compiles them in parallel).
template <int TASK, class L>
inline bool fused_pwm_family(const LaunchFlags &f, const L &l) {
  constexpr bool kMotor = TASK != PDS_TASK_TAKEOFF;  // (TakeOff + motor dynamics: only with the latency ring)
  if (f.ge) {  // round 6: BasePhysics.calculate_ground_effect (envs/physics.py:27-58) on the task it matters for (BASELINE config 4)
    if constexpr (TASK == PDS_TASK_TAKEOFF) { fused_pwm<TASK, false, true>(f, l); return true; }
    return false;
  }
  if constexpr (kMotor) { if (f.motor) { fused_pwm<TASK, true, false>(f, l); return true; } }
  fused_pwm<TASK, false, false>(f, l);
  return true;
}
template <int TASK, class L>
inline bool fused_lat_family(const LaunchFlags &f, const L &l) {
  if (f.ctrl == 0) return fused_lean_or_full<TASK, 0, true>(f, l);
  if constexpr (TASK != PDS_TASK_TAKEOFF) {  // TakeOff fixes control_mode = 'PWM' (envs/takeoff.py:225)
    if (f.ctrl == 1) return fused_lean_or_full<TASK, 1, true>(f, l);
    return fused_lean_or_full<TASK, 2, true>(f, l);
  }
  return false;
}
template <int TASK, class L>
inline bool fused_pid_hold_family(const LaunchFlags &f, const L &l) {
  constexpr bool kMotor = TASK != PDS_TASK_TAKEOFF;
  if (f.hold) {
    if constexpr (kMotor) { if (f.motor) return fused_hold<TASK, true>(f, l); }
    return fused_hold<TASK, false>(f, l);
  }
  if constexpr (TASK != PDS_TASK_TAKEOFF) {
    if (f.ctrl == 1) return fused_lean_or_full<TASK, 1, false>(f, l);
    if (f.ctrl == 2) return fused_lean_or_full<TASK, 2, false>(f, l);
  }
  return false;
}
// The dispatcher of a task's own translation unit (csrc/pds_{rollout,evaluate*}_<task>.hip), which also holds the PID control
// modes and the Kalman hold.  Hover and Circle: the latency ring and control_mode PWM are the units behind `lat` and `pwm`, the
// launch functions of that kernel form (same signature: flags, grid, stream, args); TakeOff holds all its families itself and passes nullptr.
template <class L>
using FusedFamilyFn = bool(const LaunchFlags &, dim3, hipStream_t, decltype(L::args));
template <int TASK, class L>
inline bool fused_task(const LaunchFlags &f, const L &l, FusedFamilyFn<L> *lat, FusedFamilyFn<L> *pwm) {
  if (!rollout_supported(TASK, f)) return false;
  if (f.hold) return fused_pid_hold_family<TASK>(f, l);
  if constexpr (TASK == PDS_TASK_TAKEOFF) {  // (control_mode PWM only, envs/takeoff.py:225)
    if (f.lat) return fused_lat_family<TASK>(f, l);
    return fused_pwm_family<TASK>(f, l);
  } else {
    if (f.lat) return lat(f, l.grid, l.s, l.args);
    if (f.ctrl == 0) return pwm(f, l.grid, l.s, l.args);
    return fused_pid_hold_family<TASK>(f, l);
  }
}

}  // namespace pds
