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
// final_obs lands in a row the restart overwrites whole).
// The kernel has three forms, EvalHistForm F of csrc/pds_evaluate_hist_args.h, one entry point and one set of translation units each:
//   Metrics (pds_evaluate_policies_history,        csrc/pds_evaluate_hist_<task>*.hip):         the launch above
//   Record  (pds_evaluate_policies_history_record, csrc/pds_evaluate_hist_record_<task>*.hip):  + the recorded flights
//   Stats   (pds_evaluate_policies_history_stats,  csrc/pds_evaluate_hist_stats_<task>*.hip):   + the observation sums
// Every statement a form adds is behind `if constexpr (REC)` / `if constexpr (STATS)`.  No form records and sums.
//
// Hand-over: the two counters and the kEvalStop protocol of evaluate_kernel, stated and proved at the head of csrc/pds_evaluate.h;
// the env wave's side of it is that file's PDS_EVAL_STEP_HEAD / PDS_EVAL_STEP_TAIL, the same statements in both kernels.  What
// differs here: a block holds ONE team (so blocks share no counter, as teams there), and the LDS images of the env wave's window
// -- between its act_ready wait and its obs_ready post -- are the history tile, which the network waves read between their
// obs_ready wait and their act_ready post, and the kernel's own [o(k), o(k + 1)] row tile, which they never touch; the action
// slots go the other way round, and em_lds belongs to the env wave.  "o(s + 1) is in the tile" reads "the histories of step
// s + 1 are in LDS".  (REC and STATS: the alive mask of a step is written and read in the history tile's windows, by the tile's writer
// and readers, as that file says for its Stats and Record forms: no new counter, no new wait, the argument above word for word.)
//
// THE LATENCY RING (V::LAT; pds_evaluate_policies_history_latency*, include/pds_history_latency_evaluate.h;
// csrc/pds_evaluate_hist_<task>[_pid]_lat.hip, csrc/pds_evaluate_hist_lat_{record,stats}_<task>[_pid].hip): step_once flies the
// ring in memory as in every LAT kernel, and the env wave resolves the
// reference's views of action_buffer[-1] in its own history row, as rollout_hist_kernel does: it reads ep_step = ctr_step(S.ctr) in
// front of step_once, keeps the raw `act` of PDS_EVAL_STEP_HEAD, and eval_hist_advance_row<HALF, true> writes the action columns of
// the slots 0 .. H - j between its shift and its restart.  The argument of csrc/pds_evaluate.h holds word for word: the rule
// reads two registers of the env wave (ep_step, act) and writes this lane's own row of the history tile, inside the env wave's
// window -- behind its act_ready wait and in front of its obs_ready post, where the shift and the restart already write that row --,
// so the network waves see "the histories of step s + 1" behind the same post as before.  No new counter, no new wait; the alive
// mask, the record's copy and the sums read the tile in the windows they had.
//
// METRICS: the env wave always sums the eight PDS_EM_* values, exactly as evaluate_kernel<.., EvalForm::Metrics> does -- seven words
// per lane in LDS, read and written back behind the act_ready wait, one rounded instruction per product and sum -- and stores the
// [N, 8] row where d_metrics is non-NULL: one code object per variant instead of a plain and a metrics form.
//
// THE RECORD (REC): what evaluate_kernel<.., EvalForm::Record> does (the head of csrc/pds_evaluate.h), with the history tile in place
// of the observation tile.  Of a policy's E / 64 tiles the first rec_tiles record (wave-uniform; eval_record_column has the column).
//   The ENV wave stores x(s) = S.e and the raw a(s) of every lane `alive` in front of step s with PDS_ER_STEP -- four 16-byte
//   pieces to flight[s][piece][column], behind the act_ready wait and PDS_EM_STEP, in front of step_once; nothing is carried
//   across step_once but the column.
//   The NETWORK waves, where obs_rec is given, copy the rows of the history tile whose env is alive in front of step s, raw (before
//   standardisation), to obs_rec[s][column][H half]: each wave its 16 rows, the first H half floats of each at row stride S1, 16 H half
//   contiguous floats -- between their obs_ready wait and their act_ready post (the env wave rewrites the rows behind its
//   act_ready wait), and in front of gather_hist, so that the stores are under way while the actor computes.  One dword per lane
//   and pass (eval_hist_copy_rows<1>), or 16 bytes (<4>) where H half is a multiple of 4 and obs_rec is 16-byte aligned: the
//   same bits, wave-uniform, measured 12-18 % faster as a launch than the dword form (profiles/evaluate_history_record_timing.txt).
//   The alive mask is es_lds<1>(): all ones from the prologue in front of the block barrier, then `still` from the env wave's
//   lane 0 between PDS_EVAL_STILL and PDS_EVAL_STEP_TAIL.
//   Nothing else is written: the rows s >= length of an env and every row of a tile that does not record keep what the caller put
//   there; the terminal state and the terminal observation are not recorded, as at H = 2.
//   (profiles/evaluate_history_record_kernel_resources.txt: the compiler's figures of the record's code objects.)
//
// THE OBSERVATION SUMS (STATS): what evaluate_kernel<.., EvalForm::Stats> does (the head of csrc/pds_evaluate.h), with the history
// tile in place of the observation tile.  gather_hist gives lane (n16, g) of wave w the features 16 kt + 4 g + q (kt < HN) of row
// own = 16 w + n16: every (row, feature) has one owner lane, which carries S1 and S2 of its 4 HN features through the loop -- 8 HN
// accumulators, 32 / 48 / 64 / 96 floats at HN = 4 / 6 / 8 / 12.  Per step, where row `own` is alive in front of step s (its bit of
// es_lds<1>(), the record's mask: all ones from the prologue in front of the block barrier, then `still` from the env wave's lane 0
// between PDS_EVAL_STILL and PDS_EVAL_STEP_TAIL), d = hist[own][k] - mus[k] (k >= H half: d = mus[k] - mus[k] = 0; without
// statistics mus is 0 and x - 0 = x on the bits), S1 += d, S2 += d d: __fsub_rn, __fmul_rn, __fadd_rn, one rounded instruction
// each, steps in order.  A row that is not alive is skipped by a branch, not by adding a selected 0: x + 0 = x on the bits for
// every x but -0, and no sum is -0 (each starts at +0, and +0 + -0 = +0) -- the composed path's where(alive, d, 0) gives the same.
//   THE WINDOW: the sums read the history tile and the mask between the wave's obs_ready wait of step s and its act_ready post,
//   where gather_hist reads the tile; the env wave rewrites both only behind its act_ready wait of step s, i.e. behind this
//   wave's post.  They stand BEHIND the actor pass and the action store, directly in front of the post: there the 4 HN inputs and
//   the W1 pieces of the pass are dead, and the accumulators are all the wave carries.  In front of the pass (where the H = 2
//   kernel has them) the kernels of HN = 8 and 12 spilled (profiles/evaluate_history_stats_kernel_resources.txt).
//   HN = 12: 96 accumulators beside the pass are 2 registers more than the 256 a wave of this block may hold, so the last S2 quad
//   of every lane lives in LDS (es_park_lds, 4 KB; the lane's own slot: read and written back around its four sums, no hand-over).
//   On leaving the loop (the stop it saw in obs_ready) a wave sums its 16 rows per feature in es_tree_add's fixed tree -- rows j
//   and j + 8, then + 4, + 2, + 1 -- and its n16 == 0 lanes store the partial with 16-byte stores to
//   obs_sums[tile][wave][S1 / S2][W], W = 16 HN = 64 / 96 / 128 / 192: every column is written, those from H half on are zero.
//   No atomics; the four waves of a tile are summed by the host.  The metrics are summed and stored as in the other forms.
#pragma once
#include "pds_evaluate.h"
#include "pds_evaluate_hist_args.h"
#include "pds_rollout_hist.h"

namespace pds {

// The history of the next step for this lane's own row: PDS_HIST_SHIFT_APPEND with the second half of the step's row `krow` as
// the newest half, and, where the env finished (`dn`: `krow` is its reset row then), PDS_HIST_RESTART.  A function around the two
// macros of csrc/pds_rollout_hist.h, which says why each kernel keeps the form it was built on.
// LAT (the latency ring): between the two, the action columns of the slots 0 .. views - 1 become `raw` -- the rule of
// pds_history_advance_latency, whose condition the caller has evaluated (views = 0: the rule is off on this step).  In front of the
// restart, as in rollout_hist_kernel: a finished env's reset row is written behind the rule and whole, so the rule never shows in it.
template <int HALF, bool LAT = false>
PDS_DEV void eval_hist_advance_row(float *hrow, const float *krow, int H, bool dn, [[maybe_unused]] int views = 0,
                                   [[maybe_unused]] float4 raw = make_float4(0.f, 0.f, 0.f, 0.f)) {
  const int keep = H * HALF - HALF;
  const float *newest = krow + HALF;
  PDS_HIST_SHIFT_APPEND(hrow, newest, keep)
  if constexpr (LAT) {
    for (int j = 0; j < views; ++j) {
      float *u = hrow + j * HALF + (HALF - 4);
      u[0] = raw.x; u[1] = raw.y; u[2] = raw.z; u[3] = raw.w;
    }
  }
  if (dn) {
    PDS_HIST_RESTART(hrow, krow, H, keep)
  }
}

// The record's observation copy of one network wave: of its 16 rows of the history tile (`rows16`, row stride S1 floats) the
// first HS floats of every row whose bit of `rows` is set, to the 16 HS contiguous floats at `out`, W floats per lane and pass:
// W = 1 dword moves, W = 4 16-byte moves (HS a multiple of 4 and `out` 16-byte aligned; S1 is a multiple of 4 and the tile aligned).
// Piece idx = r Q + c of the 16 Q (Q = HS / W pieces a row): idx += 64 per pass, r and c follow without a division.
template <int W>
PDS_DEV void eval_hist_copy_rows(float *out, const float *rows16, int S1, int HS, unsigned rows, int lane) {
  using T = std::conditional_t<W == 4, float4, float>;
  const int Q = HS / W;
  int r = lane / Q, c = lane - r * Q;
  T *o = reinterpret_cast<T *>(out);
  for (int idx = lane; idx < 16 * Q; idx += kWave) {
    if ((rows >> r) & 1u) o[idx] = *reinterpret_cast<const T *>(rows16 + r * S1 + W * c);
    c += kWave;
    while (c >= Q) { c -= Q; ++r; }
  }
}

// The stats form at HN = 12 keeps the last S2 quad of every network lane here, not in a register: 96 accumulators beside the actor
// pass's 48 inputs and its W1 pieces are two registers more than the 256 a wave of this block may hold, and the history tile's read
// window has the time for one more b128 read and write a step.  4 KB, a lane's own slot: nobody else reads or writes it.
PDS_DEV float4 *es_park_lds() {
  __shared__ __attribute__((aligned(16))) float4 park[kRolloutMlpWaves * kWave];
  return park;
}

// the metrics array of every argument block (NULL: summed, not stored)
PDS_DEV float *eval_hist_metrics(const EvalHistArgs &kl) { return kl.m.metrics; }
PDS_DEV float *eval_hist_metrics(const EvalHistRecordArgs &kl) { return kl.r.m.metrics; }
PDS_DEV float *eval_hist_metrics(const EvalHistStatsArgs &kl) { return kl.st.m.metrics; }

template <class V_, int HN, EvalHistForm F = EvalHistForm::Metrics>
__global__ __launch_bounds__(kRolloutThreads, 1) void evaluate_hist_kernel(const EvalHistKernelArgs<F> ka) {
  using namespace pds_mlpf;
  constexpr bool REC = F == EvalHistForm::Record, STATS = F == EvalHistForm::Stats;
  constexpr bool PARK = STATS && HN == 12;  // (es_park_lds)
  const EvalArgs &ea = eval_head(ka);
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
  [[maybe_unused]] const long long ntiles = a.n / kWave;  // (REC: PDS_ER_STEP and the observation copy size the record by it)
  const int HS = H * HALF;         // floats per history row (= the actors' d_in <= 16 HN)

  // ---- prologue: policy p's actor and statistics and the tile's histories into LDS ------------------------------------
  {
    const long long p = t / ea.tiles_per_policy;
    stage_net_wide<HN>(eval_policy_row(ea, p), wpi, tid, kRolloutThreads);
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
  if constexpr (REC || STATS) {
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
    float *hrow = hist + lane * S1;
    float4 *em = em_lds<1>();
    PDS_EM_INIT(em)
    [[maybe_unused]] long long rec_col = -1;  // REC: column of lane 0 in the record, wave-uniform; < 0: this tile does not record
    if constexpr (REC) rec_col = eval_record_column(ea, ka.r.rec_tiles, t);
    for (int s = 0; s < T; ++s) {
      const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<311, true>(ea.s, s));
      PDS_EVAL_STEP_HEAD(&act_ready, act_all)  // the network waves have read the histories and written a(s)
      {
        PDS_EM_STEP(em)
      }
      if constexpr (REC) {  // x(s) and a(s) where the env is in its first episode: four lines of the record, nothing carried
        if (rec_col >= 0) {
          PDS_ER_STEP(reinterpret_cast<const EvalRecordArgs *>(&el))
        }
      }
      [[maybe_unused]] int ep_step = 0;  // LAT: env.step()s of this env since its last reset, in front of this one
      if constexpr (V::LAT) ep_step = (int)ctr_step(S.ctr);
      StepOut so;
      step_once<V, kWave, RM, false>(el.s, o1, rks, parity, nullptr, tile, nullptr, queue, scratch, lane_s, wave_base, ix, active, act, S,
                                     qcount, nullptr, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      PDS_EVAL_RECORD_STEP(so)
      // the history of step s + 1, this lane's own row (the env goes on behind its first episode: auto-reset in place).  The newest
      // half is the second half of the step's row; where the env finished that row is its reset row, and the restart overwrites
      // the whole history
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // (step_once's wave-cooperative writes of `tile` are complete)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if constexpr (V::LAT) {
        // the latency ring, as rollout_hist_kernel states it: at step j = ep_step + 1 <= H of an episode the action columns of the
        // slots 0 .. H - j are the reference's views of action_buffer[-1] and show the raw action where this step's apply_action
        // calls rewrote that row, floor(j agg / B) > floor((j - 1) agg / B).  Divergent, at most H four-float LDS writes.
        int views = H - ep_step;
        if (views > 0) {
          const int B = el.s.k.lat_steps, agg = el.s.k.agg;
          if (!((ep_step + 1) * agg / B > ep_step * agg / B)) views = 0;
        }
        eval_hist_advance_row<HALF, true>(hrow, tile + lane * TS, H, dn, views, act);
      } else {
        eval_hist_advance_row<HALF>(hrow, tile + lane * TS, H, dn);
      }
      PDS_EVAL_STILL
      if constexpr (REC || STATS) {
        if (lane == 0) es_lds<1>()[0] = still;  // the mask of step s + 1, in front of the post
      }
      PDS_EVAL_STEP_TAIL(&obs_ready, el)  // the histories of step s + 1 are in LDS / the env wave has left
    }
    // (pds_evaluate_policies_history leaves the handle "not reset")
    PDS_EVAL_WAVE_END(EvalHistKernelArgs<F>, 312)
    if (eval_hist_metrics(kl) != nullptr) {
      PDS_EM_STORE(em, eval_hist_metrics(kl))
    }
    return;
  }

  // ================================ network waves: the actor for 16 rows of the tile each ========================
  const int own = wave * 16 + n16;  // this lane's sample row
  [[maybe_unused]] long long rec_col = -1;  // REC: as in the env wave; here < 0 also where no observations are asked for
  if constexpr (REC) {
    if (ka.r.obs_rec != nullptr) rec_col = eval_record_column(ea, ka.r.rec_tiles, t);
  }
  [[maybe_unused]] EsSums<HN, STATS> es;  // STATS: the sums of this lane's 4 HN features of row `own` (nothing otherwise)
  if constexpr (STATS) {
#pragma unroll
    for (int kt = 0; kt < HN; ++kt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { es.s1[kt][q] = 0.f; es.s2[kt][q] = 0.f; }
    }
    if constexpr (PARK) es_park_lds()[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int s = 0;; ++s) {
    const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<313, true>(ea.s, s));
    if (eval_wait_ge(&obs_ready, s) >= kEvalStop) break;  // the histories of step s are in LDS, or the env wave has left
#if PDS_ROLLOUT_ACTOR_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ACTOR_PRIO);
#endif
    if constexpr (REC) {  // the histories of step s, raw, of this wave's 16 rows whose env was alive in front of step s
      if (rec_col >= 0) {
        const EvalRecordArgs &rl = *reinterpret_cast<const EvalRecordArgs *>(&el);
        const long long nrec = (ntiles / rl.m.e.tiles_per_policy) * rl.rec_tiles * kWave;
        float *out = rl.obs_rec + ((long long)s * nrec + rec_col + wave * 16) * HS;
        const unsigned rows = (unsigned)(es_lds<1>()[0] >> (wave * 16)) & 0xFFFFu;
        // (wave-uniform.  16-byte pieces where rows and record allow them: the same bits in a quarter of the passes)
        if ((HS & 3) == 0 && (reinterpret_cast<uintptr_t>(rl.obs_rec) & 15u) == 0) eval_hist_copy_rows<4>(out, hist + wave * 16 * S1, S1, HS, rows, lane);
        else eval_hist_copy_rows<1>(out, hist + wave * 16 * S1, S1, HS, rows, lane);
      }
    }
    f32x4 x_own[HN];
    gather_hist<HN>(hist + own * S1, HS, mus, iss, g, x_own);
    PDS_FORWARD16_WIDE(el.shape, mu)
    if (g == 0) act_all[own] = make_float4(mu[0], mu[1], mu[2], mu[3]);  // lane n16 owns sample `own`: the actor's four outputs
    if constexpr (STATS) {  // the history of row `own` at step s, where its env was alive in front of step s (a row that is not adds nothing: x + 0 = x on the bits, no sum is -0)
      if (((es_lds<1>()[0] >> own) & 1ull) != 0ull) {
#pragma unroll
        for (int kt = 0; kt < HN; ++kt) {
          const int k0 = kt * 16 + 4 * g;  // (gather_hist's features and its reads; k >= HS: d = 0)
          const f32x4 v = lds4(hist + own * S1 + k0), m = lds4(mus + k0);
          if constexpr (PARK) {
            if (kt == HN - 1) { const float4 p = es_park_lds()[tid]; es.s2[kt][0] = p.x; es.s2[kt][1] = p.y; es.s2[kt][2] = p.z; es.s2[kt][3] = p.w; }
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float d = __fsub_rn((k0 + q < HS) ? v[q] : m[q], m[q]);
            es.s1[kt][q] = __fadd_rn(es.s1[kt][q], d);
            es.s2[kt][q] = __fadd_rn(es.s2[kt][q], __fmul_rn(d, d));
          }
          if constexpr (PARK) {
            if (kt == HN - 1) es_park_lds()[tid] = make_float4(es.s2[kt][0], es.s2[kt][1], es.s2[kt][2], es.s2[kt][3]);
          }
        }
      }
    }
    rollout_post(&act_ready, lane);  // this wave is done with the histories of step s
  }
  if constexpr (STATS) {  // this wave's 16 rows per feature, then [t][wave][S1 / S2][16 HN]: lane (0, g) stores the features 16 kt + 4 g ..
    float4 *out = reinterpret_cast<float4 *>(ka.st.obs_sums) + (t * kRolloutMlpWaves + wave) * (2 * 4 * HN);
    if constexpr (PARK) { const float4 p = es_park_lds()[tid]; es.s2[HN - 1][0] = p.x; es.s2[HN - 1][1] = p.y; es.s2[HN - 1][2] = p.z; es.s2[HN - 1][3] = p.w; }
#pragma unroll
    for (int kt = 0; kt < HN; ++kt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int bit = 8; bit >= 1; bit >>= 1) {  // rows j and j + 8, then + 4, + 2, + 1
          es.s1[kt][q] = es_tree_add(es.s1[kt][q], bit);
          es.s2[kt][q] = es_tree_add(es.s2[kt][q], bit);
        }
      }
      if (n16 == 0) {  // (every kt < HN: the whole slab is written, the features in H half .. 16 HN - 1 summed d = 0)
        out[kt * 4 + g] = make_float4(es.s1[kt][0], es.s1[kt][1], es.s1[kt][2], es.s1[kt][3]);
        out[4 * HN + kt * 4 + g] = make_float4(es.s2[kt][0], es.s2[kt][1], es.s2[kt][2], es.s2[kt][3]);
      }
    }
  }
}

// flags -> variant and input width: hist_task / hist_pid (on the ring: hist_lat_task / hist_lat_pid) of csrc/pds_rollout_hist.h over
// this launcher
template <EvalHistForm F>
struct EvalHistLaunchT {
  dim3 grid;  // one block per 64-env tile
  hipStream_t s;
  const EvalHistKernelArgs<F> &args;
  template <class RV_, int HN>
  void run() const { hipLaunchKernelGGL((evaluate_hist_kernel<RV_, HN, F>), grid, dim3(kRolloutThreads), 0, s, args); }
};
using EvalHistLaunch = EvalHistLaunchT<EvalHistForm::Metrics>;
using EvalHistRecordLaunch = EvalHistLaunchT<EvalHistForm::Record>;  // csrc/pds_evaluate_hist_record_<task>*.hip
using EvalHistStatsLaunch = EvalHistLaunchT<EvalHistForm::Stats>;    // csrc/pds_evaluate_hist_stats_<task>*.hip

}  // namespace pds
