// pds_rollout_deep.h -- ONE launch per rollout for ACTORS with THREE or FOUR hidden layers (gfx950): the T closed-loop steps
//     o -> standardise -> actor -> a = mu + sigma z, log p -> env.step(a) -> buffers
// for the (50, 30, 20), (32, 32, 32, 32) and the other actors of the reference's architecture search
// (experiments/01_find_NN_architecture), which struct pds_mlp of rollout_kernel (csrc/pds_rollout.h) has no room for.  Until here such a
// rollout ran as seven launches per step (critic, actor, sample, env step, V(final_obs), record + copies) replayed from a graph.  The
// kernel joins two pieces that are pinned bit for bit:
//   * from rollout_hist_kernel (csrc/pds_rollout_hist.h): the rollout form that keeps the CRITIC OUT of the kernel -- the sampling
//     (PDS_DRAW_ACTION_NOISE / PDS_EMIT_ACTION of csrc/pds_rollout.h), the env wave (step_once inside PDS_ENV_WAVE_BEGIN ..
//     PDS_ENV_WAVE_END, the bookkeeping PDS_RECORD_STEP), a partial last tile through rows / active / own_ok, and the slot list
//     fin_rows / fin_step for the last observation of the envs whose path bootstraps with V;
//   * from evaluate_deep_kernel (csrc/pds_evaluate_deep.h): the weight images of deep_stage, the input expression (v - mu) * is with the
//     features >= d_in giving (mu - mu) * is, and deep_forward<ACT, L, false> (csrc/pds_mlp_deep_tile.h) -- the function
//     pds_mlp_deep_forward runs, on the same lane roles,
// so the bits are those of T x (pds_mlp_deep_forward + pds_gaussian_sample + pds_step + pds_rollout_record).
//
// One block per 64-env tile and ONE team: four network waves (16 rows of the tile each) and the env wave.  LDS: the L weight images
// [64][68], the output layer's [8][68] and the biases are 55.4 KB at L = 3 and 73.5 KB at L = 4; the observation tile [64][TS], the
// finished envs' last rows [64][D], the actions, the statistics and the reset scratch come on top
// (profiles/rollout_deep_kernel_resources.txt has the compiler's figure per kernel).  The critic stays outside: a second image
// set at L = 4 would not fit the 160 KB beside the tiles, any critic depth is served by its own forward over obs_buf, and at two hidden
// layers the in-kernel critic measured 6 % ahead of this form (csrc/pds_rollout.h header).  There is no two-team form: the
// one-team evaluate_deep_kernel needs up to 221 VGPRs, above the 168 a ten-wave block leaves.
//
// Hand-over: two monotonic counters in LDS (rollout_wait_ge / rollout_post of csrc/pds_rollout.h), no stop protocol, no early exit --
// BOTH loops run exactly T iterations, whatever `rows` is:
//   network wave w, step s:  wait obs_ready >= s  ->  read its 16 rows of the tile  ->  actor, sample  ->  a(s) into act_all  ->
//                            post act_ready (+1);                                                     [T posts per wave]
//   env wave, step s:        wait act_ready >= 4 (s + 1)  ->  read act_all  ->  step_once writes the tile and `fin`  ->  slot list
//                            ->  post obs_ready (+1).                                                  [T posts]
// obs_ready reaches s only after the env wave's step s - 1 (0: the prologue's tile behind the block barrier), so network step s needs
// s posts of a loop that makes T > s of them; act_ready reaches 4 (s + 1) only after every network wave's step s, which waits for
// nothing but obs_ready >= s: by induction over s neither side waits for a post that is not made, for every T >= 1 (T = 1: the
// network waves pass their only wait at once and the env wave's wait needs their four posts; the env wave's last post has no
// reader).  All four network waves post also where their rows lie beyond `rows` (a partial tile): they compute on the zero rows of
// the prologue -- or on what step_once left there for its clamped lanes --, write their action slots, and only the stores to memory
// look at own_ok.  The tile is written by the env wave between its act_ready wait and its obs_ready post and read by the network
// waves between their obs_ready wait and their act_ready post; the action slots the other way round; `fin` belongs to the env
// wave; the weight images are written in the prologue in front of the only block barrier.  All five waves of a block are resident
// together (one block), so the waits cannot deadlock.
#pragma once
#include "pds_rollout.h"
#include "pds_rollout_deep_args.h"
#include "pds_mlp_deep_tile.h"

namespace pds {

template <class V_, int L>
__global__ __launch_bounds__(kRolloutThreads, 1) void rollout_deep_kernel(const RolloutDeepArgs ra) {
  namespace md = pds_mlp_detail;
  static_assert(L == 3 || L == 4, "three or four hidden layers");
  using V = std::conditional_t<regen_obs_variant<V_>(), StoredOh<V_>, V_>;
  constexpr int D = V::D;
  constexpr int TS = tile_stride<D>();
  constexpr int RM = merged_reset_variant<V>() ? RM_MERGED : RM_INLINE;
  constexpr int kScratchU4_ = (RM == RM_MERGED) ? kMergedScratchU4 : (inline_coop_variant<V>() ? inline_envs<V, false>() * scratch_stride<V>() : 0);
  static_assert(D <= md::kMaxDim, "network input <= 64 features");
  __shared__ __attribute__((aligned(16))) float Ws[L * md::kMaxDim * md::kS];  // per hidden layer [out][in], zero padded
  __shared__ __attribute__((aligned(16))) float Wos[md::kMaxOut * md::kS];     // 8 rows, see stage_wide of csrc/pds_mlp_tile.h
  __shared__ __attribute__((aligned(16))) float bs[L * md::kMaxDim], bos[md::kTW], mus[md::kMaxDim], iss[md::kMaxDim];
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
  const long long t = blockIdx.x;  // this block's 64-env tile
  const int T = ra.T;
  const int d_out = ra.pi.d_out;
  const long long rem0 = a.n - t * kWave;
  const int rows = rem0 >= kWave ? kWave : (int)rem0;

  // ---- prologue: the actor, the statistics and the tile's o(0) into LDS; env state into the env wave's registers ----
  md::deep_stage<L, kRolloutThreads>(ra.pi, Ws, Wos, bs, bos, tid, [](float v, int) { return v; });
  if (tid < md::kMaxDim) {
    const bool on = ra.mean != nullptr && tid < D;
    mus[tid] = on ? ra.mean[tid] : 0.f;
    iss[tid] = on ? 1.0f / (ra.stdv[tid] + ra.eps) : 1.f;
  }
  for (int idx = tid; idx < kWave * D; idx += kRolloutThreads) {
    const int r = idx / D, c = idx - r * D;
    tile[r * TS + c] = (r < rows) ? ra.obs0[(t * kWave + r) * D + c] : 0.f;
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
    for (int s = 0; s < T; ++s) {
      const RolloutDeepArgs &rl = *reinterpret_cast<const RolloutDeepArgs *>(&reload_args<331, true>(ra.s, s));
      const long long o1 = (long long)s * rl.s.n;
      rollout_wait_ge(&act_ready, kRolloutMlpWaves * (s + 1));  // the network waves have read o(s) and written a(s)
      PDS_OPAQUE_STEP_COPIES
      const float4 act = act_all[lane_s];
      StepOut so;
      step_once<V, kWave, RM, false>(rl.s, o1, rks, parity, nullptr, tile, nullptr, queue, scratch, lane_s, wave_base, ix, active, act, S,
                                     qcount, fin, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      PDS_RECORD_STEP(so)
      // the last observation of an env the TimeLimit cut bootstraps its path with V (also when it terminated on that step, and
      // for every env that finished on the rollout's last step: algs/iwpg/iwpg.py:374-379; `want` of rollout_hist_kernel) -> the
      // caller's slot list, from the rows step_once left in `fin`
      const bool want = dn && (so.trunc || s == T - 1);
      unsigned long long wm = __ballot(want);
      if (wm != 0ull) {  // wave-uniform, rare
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (step_once's wave-cooperative writes of `fin` are complete)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        while (wm != 0ull) {
          const int src = __builtin_ctzll(wm);
          wm &= wm - 1ull;
          const int slot = __builtin_amdgcn_readlane(nfin, src);
          if (slot < rl.slots) {
            float *dst = rl.fin_rows + ((long long)slot * rl.s.n + wave_base + src) * D;
            for (int c = lane; c < D; c += kWave) dst[c] = fin[src * D + c];
            if (lane == 0) rl.fin_step[(long long)slot * rl.s.n + wave_base + src] = s;
          }
        }
        if (want) ++nfin;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (`fin` is overwritten by the next step)
      }
      rollout_post(&obs_ready, lane);  // o(s + 1) is in the tile
    }
    PDS_ENV_WAVE_END(RolloutDeepArgs, 332)
    return;
  }

  // ================================ network waves: the actor for 16 rows of the tile each ========================
  const int own = wave * 16 + n16;  // this lane's sample row
  const bool own_ok = own < rows;
  const long long env_own = t * kWave + own;
  for (int s = 0; s < T; ++s) {
    const RolloutDeepArgs &rl = *reinterpret_cast<const RolloutDeepArgs *>(&reload_args<333, true>(ra.s, s));
    const long long o1 = (long long)s * rl.s.n;
    PDS_DRAW_ACTION_NOISE(rl, g == 0, call0 + (unsigned long long)s + 1ull, env_own, d_out)
    rollout_wait_ge(&obs_ready, s);  // o(s) is in the tile
#if PDS_ROLLOUT_ACTOR_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ACTOR_PRIO);
#endif
    // ---- input: lane (n16, g) holds features 16 kt + 4 g + q of its row = the B operands of layer 1 (mlp_deep_kernel's expression) --
    md::f32x4 cur[md::kNT];
#pragma unroll
    for (int kt = 0; kt < md::kNT; ++kt) {
      const int k0 = kt * md::kTW + 4 * g;
      const md::f32x4 mu = md::lds4(mus + k0), is = md::lds4(iss + k0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = (k0 + q < D) ? tile[own * TS + k0 + q] : mu[q];
        cur[kt][q] = (v - mu[q]) * is[q];
      }
    }
    const md::f32x4 mu = (rl.pi.activation == 0) ? md::deep_forward<0, L, false>(Ws, Wos, bs, bos, cur, nullptr, n16, g)
                                                 : md::deep_forward<1, L, false>(Ws, Wos, bs, bos, cur, nullptr, n16, g);
    if (g == 0) PDS_EMIT_ACTION(rl, mu, d_out, act_all[own], o1 + env_own, own_ok);  // lane n16 owns sample `own`: outputs 0..3 of the actor
    rollout_post(&act_ready, lane);  // this wave is done with the tile of step s
  }
}

// flags -> variant: fused_pwm_family<TASK> (csrc/pds_rollout.h) over this launcher, one block per 64-env tile
template <int L>
struct RolloutDeepLaunch {
  dim3 grid;
  hipStream_t s;
  const RolloutDeepArgs &args;
  template <class RV_>
  void run() const { hipLaunchKernelGGL((rollout_deep_kernel<RV_, L>), grid, dim3(kRolloutThreads), 0, s, args); }
};

// The launch function of one translation unit, csrc/pds_rollout_deep_<task>_l{3,4}.hip: the 16 variants of the task's family at one
// depth.  The caller has asked rollout_deep_family (fused_pwm_family looks at the noise, motor and ground-effect flags only).
#define PDS_ROLLOUT_DEEP_UNIT(NAME, TASK, L)                                                     \
  bool NAME(const LaunchFlags &f, dim3 grid, hipStream_t s, const RolloutDeepArgs &ra) {         \
    return fused_pwm_family<TASK>(f, RolloutDeepLaunch<L>{grid, s, ra});                         \
  }

}  // namespace pds
