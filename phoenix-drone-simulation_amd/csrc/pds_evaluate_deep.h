// pds_evaluate_deep.h -- ONE launch evaluates a POPULATION of policies with THREE or FOUR hidden layers (gfx950): P policies fly E
// episodes each,
//     o -> standardise(p) -> actor(p) mean -> env.step(a) -> return, length, cost and the flight metrics of the episode,
// for the actors struct pds_mlp of evaluate_kernel (csrc/pds_evaluate.h) has no room for: (50, 30, 20), (32, 32, 32, 32) and the other
// shapes of the reference's architecture search (include/pds_mlp_deep.h).  It joins two pieces that are pinned bit for bit:
//   * from evaluate_kernel: the policy per TILE (tile t flies policy t / tiles_per_policy: its tensors from row p of the flat
//     [P, param_count] block, its standardisation from row p of the [P, D] mean / std), the env wave -- step_once of csrc/pds_step.h,
//     return, length and cost frozen at an env's first `terminated | truncated`, the cost read back from the sink row behind the
//     post, the counted loop a stopped tile falls through, the eight PDS_EM_* flight metrics through em_lds -- stated by that
//     file's statement macros and not a second time, and the two counters with the kEvalStop protocol;
//   * from mlp_deep_kernel (csrc/pds_mlp_deep.hip): the weight images of deep_stage, the input expression (v - mu) * is with the
//     features >= d_in giving (mu - mu) * is, and deep_forward<ACT, L, false> (csrc/pds_mlp_deep_tile.h) -- the function
//     pds_mlp_deep_forward runs, on the same lane roles (lane (n16, g) of a wave: sample n16 of its 16 rows, features / outputs
//     4 g + q), so the action bits are those of max_steps x (pds_mlp_deep_forward per policy + pds_step).
// One block per 64-env tile and ONE team: four network waves and the env wave.  The L weight images [64][68], the output layer's
// [8][68] and the biases are 55.4 KB at L = 3 and 73.5 KB at L = 4; tile, actions, statistics, em_lds and the reset scratch come on
// top (profiles/evaluate_deep_kernel_resources.txt has the compiler's figure per kernel) -- two teams at L = 4 would not fit the
// 160 KB, and there is no two-team form.
//
// Hand-over: the two counters and the kEvalStop protocol of evaluate_kernel, stated and proved at the head of csrc/pds_evaluate.h;
// the env wave's side of it is that file's PDS_EVAL_STEP_HEAD / PDS_EVAL_STEP_TAIL, the same statements in both kernels.  A block
// holds one team, so blocks share no counter.  The tile is written by the env wave between its act_ready wait and its obs_ready
// post and read by the network waves between their obs_ready wait and their act_ready post; the action slots the other way
// round; em_lds belongs to the env wave; the weight images are written in the prologue in front of the only block barrier.
//
// METRICS: the env wave always sums the eight PDS_EM_* values, as evaluate_hist_kernel does (csrc/pds_evaluate_hist.h), and stores
// the [N, 8] row where d_metrics is non-NULL: one code object per variant and depth serves the plain and the metrics call.
// THE FORMS: EvalForm F of csrc/pds_evaluate_args.h, as in evaluate_kernel; every statement a form adds is behind an `if constexpr`
// on F, so EvalForm::Metrics is the code object it was.  Stats and Record keep evaluate_kernel's alive mask, es_lds<1>(): all ones
// from the prologue in front of the block barrier, then written by the env wave between PDS_EVAL_STILL and PDS_EVAL_STEP_TAIL and
// read by the network waves between their obs_ready wait and their act_ready post -- the tile's windows, no new counter, no new
// wait: the window argument at the head of csrc/pds_evaluate.h holds word for word.
//   Stats  (pds_evaluate_policies_deep_stats,  csrc/pds_evaluate_stats_deep_<task>_l{3,4}.hip):  + the observation sums.  Lane
//          (n16, g) of a network wave sums d = tile[own][k] - mus[k] and d * d of its features k = 16 kt + 4 g + q, kt < NIN, under
//          the mask bit of row `own` -- evaluate_kernel's statements behind the input gather, its row tree and its stores of
//          [t][wave][S1 / S2][64] behind the loop: the same operations in the same order, the composed path's slab on the bits.
//   Record (pds_evaluate_policies_deep_record, csrc/pds_evaluate_record_deep_<task>_l{3,4}.hip): + the recorded flights.  The env
//          wave: eval_record_column and PDS_ER_STEP behind the act_ready wait; the network waves copy the live rows of their 16
//          tile rows to obs_rec where it is given.
// (profiles/evaluate_deep_forms_kernel_resources.txt: the compiler's figures of the two forms' code objects.)
// Not here: observation histories, the latency ring, the PID control modes and the Kalman hold.
#pragma once
#include "pds_evaluate.h"
#include "pds_evaluate_deep_args.h"
#include "pds_evaluate_deep_forms_args.h"
#include "pds_mlp_deep_tile.h"

namespace pds {

// policy p's network: the launch's shape with the 2 (L + 1) tensors of row p of the flat [P, param_count] block
template <class KA>
PDS_DEV pds_mlp_deep eval_deep_policy_row(const KA &ka, long long p) {
  pds_mlp_deep m = ka.deep;
  const float *row = eval_deep_head(ka).e.params + p * ka.deep_param_count;  // W1 b1 .. W(L+1) b(L+1), torch order (pds_mlp_deep_param_count)
  const pds_mlp_detail::DeepOffsets o = pds_mlp_detail::deep_offsets(m);
#pragma unroll
  for (int l = 0; l < pds_mlp_detail::kDeepLayers; ++l) {
    m.w[l] = row + o.w[l];
    m.b[l] = row + o.b[l];
  }
  return m;
}

template <class V_, int L, EvalForm F = EvalForm::Metrics>
__global__ __launch_bounds__(kRolloutThreads, 1) void evaluate_deep_kernel(const EvalDeepKernelArgs<F> ka) {
  namespace md = pds_mlp_detail;
  using KA = EvalDeepKernelArgs<F>;
  static_assert(L == 3 || L == 4, "three or four hidden layers");
  static_assert(F != EvalForm::Plain, "the plain call is the metrics form with d_metrics NULL");
  const EvalArgs &ea = eval_deep_head(ka).e;
  using V = std::conditional_t<regen_obs_variant<V_>(), StoredOh<V_>, V_>;
  constexpr int D = V::D;
  constexpr int TS = tile_stride<D>();
  constexpr int NIN = (D + 15) / 16;
  constexpr int RM = merged_reset_variant<V>() ? RM_MERGED : RM_INLINE;
  constexpr int kScratchU4_ = (RM == RM_MERGED) ? kMergedScratchU4 : (inline_coop_variant<V>() ? inline_envs<V, false>() * scratch_stride<V>() : 0);
  static_assert(D <= md::kMaxDim, "network input <= 64 features");
  __shared__ __attribute__((aligned(16))) float Ws[L * md::kMaxDim * md::kS];  // per hidden layer [out][in], zero padded
  __shared__ __attribute__((aligned(16))) float Wos[md::kMaxOut * md::kS];     // 8 rows, see stage_wide of csrc/pds_mlp_tile.h
  __shared__ __attribute__((aligned(16))) float bs[L * md::kMaxDim], bos[md::kTW], mus[md::kMaxDim], iss[md::kMaxDim];
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
  const long long t = blockIdx.x;  // this block's 64-env tile (N = P x E, E a multiple of 64: every tile is full)
  [[maybe_unused]] const long long ntiles = a.n / kWave;  // (Record: PDS_ER_STEP's)
  const int T = ea.T;

  // ---- prologue: policy p's network and statistics and the tile's o(0) into LDS ---------------------------------------
  {
    const long long p = t / ea.tiles_per_policy;
    md::deep_stage<L, kRolloutThreads>(eval_deep_policy_row(ka, p), Ws, Wos, bs, bos, tid, [](float v, int) { return v; });
    if (tid < md::kMaxDim) {
      const bool on = ea.mean != nullptr && tid < D;
      mus[tid] = on ? ea.mean[p * D + tid] : 0.f;
      iss[tid] = on ? 1.0f / (ea.stdv[p * D + tid] + ea.eps) : 1.f;
    }
    for (int idx = tid; idx < kWave * D; idx += kRolloutThreads) {
      const int r = idx / D, c = idx - r * D;
      tile[r * TS + c] = ea.obs0[(t * kWave + r) * D + c];
    }
  }
  if (tid == 0) { obs_ready = 0; act_ready = 0; }
  if constexpr (eval_keeps_alive_mask(F)) {
    if (tid == 0) es_lds<1>()[0] = ~0ull;  // the mask of step 0
  }
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
    PDS_EVAL_WAVE_ACCUMULATORS
    float4 *em = em_lds<1>();
    PDS_EM_INIT(em)
    [[maybe_unused]] long long rec_col = -1;  // Record: column of lane 0 in the record, wave-uniform; < 0: this tile does not record
    if constexpr (F == EvalForm::Record) rec_col = eval_record_column(ea, ka.r.rec_tiles, t);
    for (int s = 0; s < T; ++s) {
      const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<321, true>(ea.s, s));
      PDS_EVAL_STEP_HEAD(&act_ready, act_all)  // the network waves have read o(s) and written a(s)
      {
        PDS_EM_STEP(em)
      }
      if constexpr (F == EvalForm::Record) {  // x(s) and a(s) where the env is in its first episode: four lines of the record, nothing carried
        if (rec_col >= 0) {
          PDS_ER_STEP(reinterpret_cast<const EvalRecordArgs *>(&el))
        }
      }
      StepOut so;
      step_once<V, kWave, RM, false>(el.s, o1, rks, parity, nullptr, tile, nullptr, queue, scratch, lane_s, wave_base, ix, active, act, S,
                                     qcount, nullptr, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      PDS_EVAL_RECORD_STEP(so)
      PDS_EVAL_STILL
      if constexpr (eval_keeps_alive_mask(F)) {
        if (lane == 0) es_lds<1>()[0] = still;  // the mask of step s + 1, in front of the post
      }
      PDS_EVAL_STEP_TAIL(&obs_ready, el)  // o(s + 1) is in the tile / the env wave has left
    }
    // (pds_evaluate_policies_deep leaves the handle "not reset"; kl: the EvalMetricsArgs at the head of every form's block)
    PDS_EVAL_WAVE_END(EvalMetricsArgs, 322)
    if (kl.metrics != nullptr) {
      PDS_EM_STORE(em, kl.metrics)
    }
    return;
  }

  // ================================ network waves: the actor for 16 rows of the tile each ========================
  const int own = wave * 16 + n16;  // this lane's sample row
  EsSums<NIN, F == EvalForm::Stats> es;  // Stats: the sums of this lane's 4 NIN features of row `own` (nothing otherwise)
  if constexpr (F == EvalForm::Stats) {
#pragma unroll
    for (int kt = 0; kt < NIN; ++kt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { es.s1[kt][q] = 0.f; es.s2[kt][q] = 0.f; }
    }
  }
  [[maybe_unused]] long long rec_col = -1;  // Record: as in the env wave; here < 0 also where no observations are asked for
  if constexpr (F == EvalForm::Record) {
    if (ka.r.obs_rec != nullptr) rec_col = eval_record_column(ea, ka.r.rec_tiles, t);
  }
  for (int s = 0;; ++s) {
    const KA &dl = *reinterpret_cast<const KA *>(&reload_args<323, true>(ea.s, s));
    if (eval_wait_ge(&obs_ready, s) >= kEvalStop) break;  // o(s) is in the tile, or the env wave has left
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
    if constexpr (F == EvalForm::Stats) {  // o(s) of row `own`, where its env was alive in front of step s (evaluate_kernel's statements)
      const bool al = ((es_lds<1>()[0] >> own) & 1ull) != 0ull;
#pragma unroll
      for (int kt = 0; kt < NIN; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = kt * 16 + 4 * g + q;  // (the gather's feature; k >= D: d = 0)
          const float m = mus[k];
          const float d = __fsub_rn((k < D) ? tile[own * TS + k] : m, m);
          es.s1[kt][q] = __fadd_rn(es.s1[kt][q], al ? d : 0.f);
          es.s2[kt][q] = __fadd_rn(es.s2[kt][q], al ? __fmul_rn(d, d) : 0.f);
        }
      }
    }
    if constexpr (F == EvalForm::Record) {  // o(s), raw, of this wave's 16 rows whose env was alive in front of step s: 16 D contiguous floats
      if (rec_col >= 0) {
        const EvalRecordArgs &rl = dl.r;
        const long long nrec = (ntiles / rl.m.e.tiles_per_policy) * rl.rec_tiles * kWave;
        float *out = rl.obs_rec + ((long long)s * nrec + rec_col + wave * 16) * D;
        const unsigned rows = (unsigned)(es_lds<1>()[0] >> (wave * 16)) & 0xFFFFu;
        for (int idx = lane; idx < 16 * D; idx += kWave) {
          const int r = idx / D, c = idx - r * D;
          if ((rows >> r) & 1u) out[idx] = tile[(wave * 16 + r) * TS + c];
        }
      }
    }
    const md::f32x4 y = (dl.deep.activation == 0) ? md::deep_forward<0, L, false>(Ws, Wos, bs, bos, cur, nullptr, n16, g)
                                                  : md::deep_forward<1, L, false>(Ws, Wos, bs, bos, cur, nullptr, n16, g);
    if (g == 0) act_all[own] = make_float4(y[0], y[1], y[2], y[3]);  // lane n16 owns sample `own`: the actor's four outputs
    rollout_post(&act_ready, lane);  // this wave is done with the tile of step s
  }
  if constexpr (F == EvalForm::Stats) {  // this wave's 16 rows per feature, then [t][wave][S1 / S2][64]: lane (0, g) stores the features 16 kt + 4 g ..
    float4 *out = reinterpret_cast<float4 *>(ka.st.obs_sums) + (t * kRolloutMlpWaves + wave) * (2 * 16);
#pragma unroll
    for (int kt = 0; kt < NIN; ++kt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int bit = 8; bit >= 1; bit >>= 1) {  // rows j and j + 8, then + 4, + 2, + 1
          es.s1[kt][q] = es_tree_add(es.s1[kt][q], bit);
          es.s2[kt][q] = es_tree_add(es.s2[kt][q], bit);
        }
      }
      if (n16 == 0) {
        out[kt * 4 + g] = make_float4(es.s1[kt][0], es.s1[kt][1], es.s1[kt][2], es.s1[kt][3]);
        out[16 + kt * 4 + g] = make_float4(es.s2[kt][0], es.s2[kt][1], es.s2[kt][2], es.s2[kt][3]);
      }
    }
#pragma unroll
    for (int kt = NIN; kt < 4; ++kt) {  // features >= 16 NIN (those in D .. 16 NIN - 1 summed d = 0)
      if (n16 == 0) { out[kt * 4 + g] = make_float4(0.f, 0.f, 0.f, 0.f); out[16 + kt * 4 + g] = make_float4(0.f, 0.f, 0.f, 0.f); }
    }
  }
}

// flags -> variant: fused_pwm_family<TASK> (csrc/pds_rollout.h) over this launcher, one block per 64-env tile
template <int L, EvalForm F = EvalForm::Metrics>
struct EvalDeepLaunch {
  dim3 grid;
  hipStream_t s;
  const EvalDeepKernelArgs<F> &args;
  template <class RV_>
  void run() const { hipLaunchKernelGGL((evaluate_deep_kernel<RV_, L, F>), grid, dim3(kRolloutThreads), 0, s, args); }
};

// The launch function of one translation unit, csrc/pds_evaluate_deep_<task>_l{3,4}.hip: the 16 variants of the task's family at
// one depth.  The caller has asked evaluate_deep_family (fused_pwm_family looks at the noise, motor and ground-effect flags only).
#define PDS_EVALUATE_DEEP_UNIT(NAME, TASK, L)                                                    \
  bool NAME(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepArgs &ka) {            \
    return fused_pwm_family<TASK>(f, EvalDeepLaunch<L>{grid, s, ka});                            \
  }
// ... and of a unit of the stats / record form, csrc/pds_evaluate_{stats,record}_deep_<task>_l{3,4}.hip
#define PDS_EVALUATE_DEEP_FORM_UNIT(NAME, TASK, L, FORM)                                                  \
  bool NAME(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalDeepKernelArgs<FORM> &ka) {         \
    return fused_pwm_family<TASK>(f, EvalDeepLaunch<L, FORM>{grid, s, ka});                               \
  }

}  // namespace pds
