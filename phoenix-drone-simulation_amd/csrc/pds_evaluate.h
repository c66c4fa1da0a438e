// pds_evaluate.h -- ONE launch evaluates a POPULATION of policies (gfx950): P policies fly E episodes each,
//     o -> standardise(p) -> actor(p) mean -> env.step(a) -> return, length, cost of the episode
// of the caller's evaluation loop (utils/evaluation.py:52-107, EnvironmentEvaluator.eval_once: act deterministically until
// terminated or truncated, sum reward and info['cost']; ActorCritic.step in eval mode, algs/core.py:370-393).  It is the
// evaluation counterpart of rollout_kernel (csrc/pds_rollout.h) and keeps its wave roles -- four network waves on
// forward16_shape (csrc/pds_mlp_fwd.h: the code path of pds_mlp_forward, same bits), one env wave on step_once (csrc/pds_step.h:
// the code path of pds_step, same bits), LDS counters between them -- without what an evaluation does not need: no critic
// image and no critic pass, no V(final_obs) and no `fin` rows, no action noise and no log-probability, no [T, N] buffer.
//
// The policy is per TILE, not per launch: the N = P x E envs are P contiguous blocks of E envs (E a multiple of 64), tile t
// belongs to policy p = t / (E / 64) and stages that policy's six tensors from row p of the flat [P, param_count] block and its
// standardisation from row p of the [P, D] mean / std.  Two teams of a block may fly different policies, so each team has its own
// weight image and its own mus / iss (the critic's LDS pays for the second image): per team 39 744 B of weights + 512 B of
// statistics + the observation tile (8.7-13.3 KB) + 1 KB of actions + the reset scratch: 52.9-55.9 KB per team, 105.9-111.8 KB for
// two -- of the CU's 160 KB, below the two-team rollout_kernel's 123-134 KB (profiles/evaluate_kernel_resources.txt has the compiler's figure per kernel).
//
// Return, length and cost of an env accumulate in the env wave's registers and freeze at the env's first `terminated |
// truncated` (the env itself goes on: auto-reset in place, as under the composed loop).  A tile STOPS once none of its 64 lanes
// is still in its first episode -- a population holds many policies that fall within 50-150 of the 500 steps.
//
// Hand-over (rollout_wait_ge / rollout_post of csrc/pds_rollout.h; all five waves of a team are resident together):
//   act_ready: +1 per network wave and step, after the wave has read o(s) and written its 16 actions of step s.  The env wave
//              waits for 4 (s + 1) in front of step s.
//   obs_ready: posted ONCE by the env wave at the end of every iteration s, after o(s + 1) is in the tile: +1 when it will run
//              step s + 1, + kEvalStop when it will not (no lane in its first episode, or s + 1 == T).  After iteration s the
//              counter is therefore either s + 1 or >= kEvalStop, never anything else, and the one atomic add makes the
//              decision and the signal the same event.
//   A network wave waits for obs_ready >= s in front of step s and looks at the value that ended its wait: s (the env wave
//   will wait for this step's actions: compute and post them) or >= kEvalStop (it will not: leave).  So every wait has its post:
//   the env wave only waits for actions of a step it announced with +1, the network waves only wait for an iteration's end, and
//   the env wave ends EVERY iteration it starts with a post and its last one with the stop.  No wave waits for a signal that never
//   comes; the env wave never waits after its stop, so the team drains without it.  Teams share no counter: one team of a block
//   leaves while the other flies on (there is no block barrier behind the prologue).
//   LDS images: the tile is written by the env wave between its act_ready wait and its obs_ready post, and read by the network
//   waves between their obs_ready wait and their act_ready post; the action slots the other way round.
//   (EvalForm::Stats and Record, below: the alive mask of a step is written and read in the tile's windows, by the tile's writer and readers.)
//
// The cost of a step: StepOut carries reward and flags only, and step_once stores the cost through StepArgs::cost like every
// per-step stream.  The env wave reads its own lane's word back from the sink row BEHIND its post (same lane, same address:
// program order), so the round trip runs while the network waves compute, and adds it in front of the next step.
//
// The kernel has four forms, EvalForm F of csrc/pds_evaluate_args.h, one entry point and one set of translation units each;
// every statement a form adds is behind an `if constexpr` on F, and its LDS belongs to a function only the forms that use it call.
//   Plain   (pds_evaluate_policies,         csrc/pds_evaluate_<task>*.hip):          return, length and cost, as above
//   Metrics (pds_evaluate_policies_metrics, csrc/pds_evaluate_metrics_<task>*.hip):  + the flight metrics
//   Stats   (pds_evaluate_policies_stats,   csrc/pds_evaluate_stats_<task>*.hip):    + the flight metrics and the observation sums
//   Record  (pds_evaluate_policies_record,  csrc/pds_evaluate_record_<task>*.hip):   + the flight metrics and the recorded flights
// eval_sums_metrics(F): every form but Plain.  eval_keeps_alive_mask(F): Stats and Record.  No form gathers sums and records.
//
// THE FLIGHT METRICS (eval_sums_metrics(F)): the env wave also sums the eight
// PDS_EM_* flight metrics (include/pds.h) over the states x(0) .. x(L - 1) its first episode's policy acted in -- the true roll,
// pitch and body rates, the last action and the action handed over are in its registers anyway.  Every product and every sum is an
// instruction of its own (__fmul_rn / __fadd_rn / __fsub_rn): the composed path does the same arithmetic with one torch op each.
// Seven words per lane carry the eight values from step to step: five float sums, the saturated steps above the two sign bits of
// the previous roll and pitch rate, and the two crossing counters as the halves of one word (an episode has at most 65 535 steps:
// pds_create).  The counters are integers until the store: exact, like the float sum of ones they stand for.
// WHERE the seven words live between two steps: in LDS (em_lds, 2 KB per team, touched by the env wave's own lanes only), read
// and written back BEHIND the act_ready wait, around the update -- two ds_read_b128 and two ds_write_b128 a step.  Kept in
// registers across step_once they took Hover at its defaults from 149 to 173 VGPRs and its two-team form over the 168-register
// cap; from LDS the env wave carries nothing through the step (151).  The update is NOT in front of the wait, where the wave
// idles: with the attitude and rate terms there the compiler gave the env wave 40-50 more VGPRs whichever way the sums were
// kept (Hover at its defaults 201-215; 88 of the 102 two-team forms and ten one-team forms spilled) --
// profiles/evaluate_metrics_kernel_resources.txt has both findings.
//
// THE OBSERVATION SUMS (F == EvalForm::Stats): the NETWORK waves
// also sum, per feature k < D, d = o_k(s) - mean[p][k] (d = o_k without statistics: mus is 0 there and x - 0 = x on the bits) and
// d * d over every observation o(s) a first-episode policy acted on -- row r of the tile at step s where env r was `alive` in
// front of step s, the predicate of ep_len.  gather_input gives lane (n16, g) of wave w the features 16 kt + 4 g + q of row
// 16 w + n16: every (row, feature) has one owner lane, which carries S1 and S2 of its 4 NIN features in registers through the
// loop, steps in order, one rounded instruction per difference, product and sum (the composed path: one torch op each).
//   The alive mask: one 64-bit word per team in LDS (es_lds), bit r = env r is in its first episode.  The mask of step 0, all
//   ones, is written in the prologue in front of the block barrier.  The env wave writes the mask of step s + 1 in the tile's
//   window -- between its act_ready wait of step s and its obs_ready post -- and the network waves read it in the tile's window:
//   between their obs_ready wait and their act_ready post.  It adds no counter and no wait: the hand-over above is the mask's.
//   A wave that leaves its loop (the stop it saw in obs_ready, whichever step that was) sums its 16 rows per feature in a fixed
//   tree -- rows j and j + 8, then j and j + 4, then + 2, then + 1: cross-lane moves and __fadd_rn, no atomics -- and stores its
//   partial to obs_sums[tile][wave][S1 / S2][64] with 16-byte stores, features >= D zero.  The four waves of a tile are summed by
//   the host: on the device that would take a hand-over.
//
// THE RECORD (F == EvalForm::Record): the flights leave the kernel.  Of a policy's E / 64 tiles the first rec_tiles record (wave-uniform; EvalRecordArgs,
// csrc/pds_evaluate_args.h, has the column of a lane); the metrics are summed as in the metrics form and stored where an array is given.
//   The ENV wave stores x(s) = S.e -- the reference log's twelve columns, in the log's order -- and the raw a(s) of every lane
//   `alive` in front of step s (the predicate of ep_len) as four 16-byte pieces to flight[s][piece][column]: per piece a wave
//   writes one contiguous 1 KiB line.  Where PDS_EM_STEP is: behind the act_ready wait, which is where the action exists, and
//   for the reason given under the flight metrics not in front of it.  Plain vector stores of registers the wave holds there anyway;
//   nothing is carried across step_once but the column, two scalar registers.
//   The NETWORK waves, where obs_rec is given, copy the rows of the tile whose env is alive in front of step s, raw, to
//   obs_rec[s][column][D]: each wave its 16 rows, 16 D contiguous floats, one dword per lane and pass -- in the tile's read window,
//   between their obs_ready wait and their act_ready post.  The alive mask is the stats form's (es_lds): same windows, no new
//   counter, no new wait.
//   Nothing else is written: a stopped tile writes nothing more, the rows s >= length of an env and every row of a tile that does
//   not record keep what the caller put there.  NOT recorded: the terminal state x(L) and the terminal observation -- a finished
//   env is reset in place inside step_once, and final_obs is NULL in this kernel.
// (profiles/evaluate_{metrics,stats,record}_kernel_resources.txt: the compiler's figures of every form's code objects.)
#pragma once
#include "pds_evaluate_args.h"
#include "pds_rollout.h"

namespace pds {

constexpr int kEvalStop = 1 << 30;  // added to obs_ready instead of 1: the env wave has left

// rollout_wait_ge that also says what it saw
PDS_DEV int eval_wait_ge(int *flag, int need) {
  int v;
  while ((v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP))) < need)
    __builtin_amdgcn_s_sleep(1);
  return v;
}
PDS_DEV void eval_post(int *flag, int lane, int inc) {  // + inc, after every lane's LDS accesses of this phase
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0) __hip_atomic_fetch_add(flag, inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// policy p's network: the launch's shape with the six tensors of row p of the flat [P, param_count] block
PDS_DEV pds_mlp eval_policy_row(const EvalArgs &ea, long long p) {
  pds_mlp m = ea.shape;
  const float *row = ea.params + p * ea.param_count;  // W1 b1 W2 b2 W3 b3, torch order (pds_mlp_param_count)
  m.w1 = row;
  m.b1 = m.w1 + m.h1 * m.d_in;
  m.w2 = m.b1 + m.h1;
  m.b2 = m.w2 + m.h2 * m.h1;
  m.w3 = m.b2 + m.h2;
  m.b3 = m.w3 + m.d_out * m.h2;
  return m;
}

// the metrics form's seven words per lane between two steps: [team][0][lane] = roll_sq, pitch_sq, rate_sq, action_rate_sq;
// [team][1][lane] = tilt_max, saturated steps << 2 | sign bits, pitch crossings << 16 | roll crossings, unused
template <int TEAMS>
PDS_DEV float4 *em_lds() {
  __shared__ float4 em[TEAMS * 2 * kWave];
  return em;
}

// the stats form's alive mask per team: bit r = env r of the tile is in its first episode (windows: the head of this file)
template <int TEAMS>
PDS_DEV unsigned long long *es_lds() {
  __shared__ unsigned long long alive_mask[TEAMS];
  return alive_mask;
}
// a network lane's accumulators of the stats form: S1 and S2 of its 4 NIN features; the other forms carry none
template <int NIN, bool SUMS>
struct EsSums {
  float s1[NIN][4], s2[NIN][4];
};
template <int NIN>
struct EsSums<NIN, false> {};
// v + (v of the lane whose row differs in bit `bit`): one level of the stats form's row tree (the sum is the same in both lanes)
PDS_DEV float es_tree_add(float v, int bit) { return __fadd_rn(v, __shfl_xor(v, bit)); }

// ---- the env wave of an evaluation, for evaluate_kernel and evaluate_hist_kernel (csrc/pds_evaluate_hist.h): statement macros
// over the kernels' own locals, in the style of PDS_ENV_WAVE_BEGIN / PDS_RECORD_STEP of csrc/pds_rollout.h and for the reason
// given there -- the metrics update as a forced-inline function (the state by reference) moved all 44 kernels of the TakeOff
// metrics unit and all 8 of the TakeOff history unit: -21 .. +15 instructions, and the scratch of five spilling two-team forms
// (208 -> 212, 216 -> 212 B, ...), which is what two_teams_fit decides by (profiles/fused_refactor_identity.txt).  Locals of
// PDS_ENV_WAVE_BEGIN apart, they read lane, T, s, ix, ea, t and wave_base. ----
// In front of the loop.  Declares the frozen accumulators ep_ret, ep_len, ep_cost and what they hang on:
#define PDS_EVAL_WAVE_ACCUMULATORS                                                                         \
  float ep_ret = 0.f, ep_len = 0.f, ep_cost = 0.f;                                                         \
  bool alive = true;     /* this lane's env is in its first episode */                                     \
  float c_step = 0.f;    /* the last step's cost, on its way back from the sink row ... */                 \
  bool c_counts = false; /* ... and whether it belongs to the first episode */                             \
  int qcount = 0;                                                                                          \
  bool stopped = false;  /* wave-uniform: this tile has posted its stop */
// The head of iteration s, down to the action.  A stopped tile falls through its remaining iterations (a scalar compare and a
// branch each) instead of leaving the loop: the loop stays a counted one.  With a data-dependent exit -- `if (!more) break;` behind
// the step -- the compiler gave the env wave of the observation-noise variants 40 more VGPRs (Hover at its defaults: 202 against
// 149), and their two-team form spilled (profiles/evaluate_kernel_resources.txt).  The parity of the state ring goes on toggling
// there: behind the loop it is parity(entry) ^ (T & 1) in EVERY tile, as after a rollout of T steps -- the library reads tile 0's
// parity for all envs between launches (csrc/pds_api.hip field_kernel: which hist slot is the last action, which the one before).
// Then the wait for the four network waves' posts of step s on `act_ready`, the cost of step s - 1 (read back behind its post),
// and PDS_OPAQUE_STEP_COPIES / PDS_SINK_ROW_OFFSET of csrc/pds_rollout.h.  Declares rks, lane_s, o1 and act = `acts`[lane].
#define PDS_EVAL_STEP_HEAD(act_ready, acts)                       \
  if (stopped) { parity ^= 1; continue; }                         \
  rollout_wait_ge(act_ready, kRolloutMlpWaves * (s + 1));         \
  ep_cost += c_counts ? c_step : 0.f;                             \
  PDS_OPAQUE_STEP_COPIES                                          \
  PDS_SINK_ROW_OFFSET                                             \
  const float4 act = acts[lane_s];
// Behind step_once: the accumulator updates of evaluation.evaluate, in its order and its form (x + 0 for an env that has
// finished).  Declares dn: the env finished in this step, whichever episode it was in.
#define PDS_EVAL_RECORD_STEP(so)            \
  ep_ret += alive ? so.reward : 0.f;        \
  ep_len += alive ? 1.f : 0.f;              \
  c_counts = alive;                         \
  const bool dn = so.done || so.trunc;      \
  alive = alive && !dn;
// The tail of iteration s in two pieces (the stats form writes its mask between them).  Declares still: the lanes in their first
// episode, and more (wave-uniform): the env wave will run step s + 1.
#define PDS_EVAL_STILL                               \
  const unsigned long long still = __ballot(alive);  \
  const bool more = still != 0ull && s + 1 < T;
// ... the ONE post of the iteration on `obs_ready`, +1 or the stop (the protocol at the head of this file); behind it the read-back
// of this lane's cost of the step from the sink row of `el`.
#define PDS_EVAL_STEP_TAIL(obs_ready, el)                   \
  eval_post(obs_ready, lane, more ? 1 : kEvalStop);         \
  c_step = *at(el.s.cost, ix);                              \
  stopped = !more;
// Behind the loop: the last step's cost; the state as the tile left it and the clock T ticks on, whichever step the tile stopped
// at (the caller resets before it steps again); return, length and cost of the first episode.  RA: the kernel's argument struct,
// ID: its reload_args tag; declares kl (the reloaded RA) and el (its EvalArgs).
#define PDS_EVAL_WAVE_END(RA, ID)                                                              \
  ep_cost += c_counts ? c_step : 0.f;                                                          \
  const RA &kl = *reinterpret_cast<const RA *>(&reload_args<ID, true>(ea.s, T));               \
  const EvalArgs &el = eval_head(kl);                                                          \
  store_state<V>(el.s, ix, parity, S, true);                                                   \
  advance_clock(el.s.st.clk, t, rk0, parity, (uint32_t)T, lane);                               \
  *at(el.ret, ix) = ep_ret;                                                                    \
  *at(el.len, ix) = ep_len;                                                                    \
  *at(el.cost, ix) = ep_cost;
// ---- the flight metrics (the head of this file), `em` = this team's 2 x 64 float4 of em_lds ----
// zero sums and the signs of x(0)'s roll and pitch rate
#define PDS_EM_INIT(em)                                                                                                         \
  em[lane] = make_float4(0.f, 0.f, 0.f, 0.f);                                                                                   \
  em[kWave + lane] = make_float4(0.f, __int_as_float((S.e.wx < 0.f ? 1 : 0) | (S.e.wy < 0.f ? 2 : 0)), __int_as_float(0), 0.f);
// x(s), the state the policy acted in, and a(s), raw, against u(k - 1) = the last action before the step: between the action read
// and step_once, in a block of its own.  (Tilt: one compare each -- a NaN angle is passed over, whichever it is.)
#define PDS_EM_STEP(em)                                                                                                                   \
  const float4 sums = em[lane_s], rest = em[kWave + lane_s];                                                                              \
  float m_roll = sums.x, m_pitch = sums.y, m_rate = sums.z, m_act = sums.w, m_tilt = rest.x;                                              \
  int m_sat = __float_as_int(rest.y), m_cross = __float_as_int(rest.z);                                                                   \
  const EnvRegs &e = S.e;                                                                                                                 \
  m_roll = __fadd_rn(m_roll, alive ? __fmul_rn(e.roll, e.roll) : 0.f);                                                                    \
  m_pitch = __fadd_rn(m_pitch, alive ? __fmul_rn(e.pitch, e.pitch) : 0.f);                                                                \
  const float w2 = __fadd_rn(__fadd_rn(__fmul_rn(e.wx, e.wx), __fmul_rn(e.wy, e.wy)), __fmul_rn(e.wz, e.wz));                             \
  m_rate = __fadd_rn(m_rate, alive ? w2 : 0.f);                                                                                           \
  const float ar = fabsf(e.roll), ap = fabsf(e.pitch);                                                                                    \
  m_tilt = (alive && ar > m_tilt) ? ar : m_tilt;                                                                                          \
  m_tilt = (alive && ap > m_tilt) ? ap : m_tilt;                                                                                          \
  const int neg = (e.wx < 0.f ? 1 : 0) | (e.wy < 0.f ? 2 : 0);                                                                            \
  const int crossed = alive ? ((neg ^ m_sat) & 3) : 0;                                                                                    \
  m_cross += (crossed & 1) | ((crossed & 2) << 15);                                                                                       \
  m_sat = (m_sat & ~3) | neg;                                                                                                             \
  const float d0 = __fsub_rn(act.x, S.h1.x), d1 = __fsub_rn(act.y, S.h1.y), d2 = __fsub_rn(act.z, S.h1.z), d3 = __fsub_rn(act.w, S.h1.w); \
  const float dd = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)), __fmul_rn(d3, d3));           \
  m_act = __fadd_rn(m_act, alive ? dd : 0.f);                                                                                             \
  const bool sat = fabsf(act.x) > 1.f || fabsf(act.y) > 1.f || fabsf(act.z) > 1.f || fabsf(act.w) > 1.f;                                  \
  m_sat += (alive && sat) ? 4 : 0;                                                                                                        \
  em[lane_s] = make_float4(m_roll, m_pitch, m_rate, m_act);                                                                               \
  em[kWave + lane_s] = make_float4(m_tilt, __int_as_float(m_sat), __int_as_float(m_cross), 0.f);
// row `env` of `metrics` [N, 8] as two 16-byte pieces (every tile is full: env < N), in a block of its own
#define PDS_EM_STORE(em, metrics)                                                                                 \
  float4 *row = reinterpret_cast<float4 *>(metrics) + 2 * (wave_base + lane);                                     \
  const float4 rest = em[kWave + lane];                                                                           \
  const int m_sat = __float_as_int(rest.y), m_cross = __float_as_int(rest.z);                                     \
  row[0] = em[lane];                                                                                              \
  row[1] = make_float4(rest.x, (float)(m_sat >> 2), (float)(m_cross & 0xFFFF), (float)((unsigned)m_cross >> 16));

// ---- the record of the flights (the head of this file) ----
// the column of lane 0 of tile t in the record (csrc/pds_evaluate_args.h EvalRecordArgs), or -1 where the tile does not record
PDS_DEV long long eval_record_column(const EvalArgs &ea, int rec_tiles, long long t) {
  const long long p = t / ea.tiles_per_policy;
  const int k = (int)(t - p * ea.tiles_per_policy);
  return k < rec_tiles ? (p * rec_tiles + k) * kWave : -1;
}
// x(s) = S.e and a(s) = act of the lanes in their first episode, behind the act_ready wait and in front of step_once: four plain
// 16-byte stores of registers the wave holds there anyway.  `rl`: the reloaded EvalRecordArgs
#define PDS_ER_STEP(rl)                                                                                   \
  const long long nrec = (ntiles / (rl)->m.e.tiles_per_policy) * (rl)->rec_tiles * kWave;                 \
  float4 *line = (rl)->flight + (long long)s * 4 * nrec + rec_col + lane_s;                               \
  if (alive) {                                                                                            \
    line[0] = make_float4(S.e.px, S.e.py, S.e.pz, S.e.vx);                                                \
    line[nrec] = make_float4(S.e.vy, S.e.vz, S.e.roll, S.e.pitch);                                        \
    line[2 * nrec] = make_float4(S.e.yaw, S.e.wx, S.e.wy, S.e.wz);                                        \
    line[3 * nrec] = act;                                                                                 \
  }

template <class V_, int TEAMS, EvalForm F>
__global__ __launch_bounds__(kRolloutThreads * TEAMS, 1) void evaluate_kernel(const EvalKernelArgs<F> ka) {
  using namespace pds_mlpf;
  const EvalArgs &ea = eval_head(ka);
  using V = std::conditional_t<regen_obs_variant<V_>(), StoredOh<V_>, V_>;
  constexpr int D = V::D;
  constexpr int TS = tile_stride<D>();
  constexpr int NIN = (D + 15) / 16;
  constexpr int RM = merged_reset_variant<V>() ? RM_MERGED : RM_INLINE;
  constexpr int kScratchU4_ = (RM == RM_MERGED) ? kMergedScratchU4 : (inline_coop_variant<V>() ? inline_envs<V, false>() * scratch_stride<V>() : 0);
  static_assert(D <= 64, "network input <= 64 features");
  __shared__ __attribute__((aligned(16))) float net_all[TEAMS][kNetFloats];
  __shared__ __attribute__((aligned(16))) float mus_all[TEAMS][64], iss_all[TEAMS][64];
  __shared__ __attribute__((aligned(16))) float tile_all[TEAMS][kWave * TS];
  __shared__ __attribute__((aligned(16))) float4 act_all[TEAMS][kWave];
  __shared__ uint32_t queue_all[TEAMS][kQueueCap];
  __shared__ U4 scratch_all[TEAMS][kScratchU4_ > 0 ? kScratchU4_ : 1];
  __shared__ int obs_ready[TEAMS], act_ready[TEAMS];
#ifdef PDS_STAMPS
  unsigned long long stamp_[kStampSlots];
#endif
  prefetch_kernargs();
  const StepArgs &a = ea.s;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int team = __builtin_amdgcn_readfirstlane(tid / kRolloutThreads);  // wave-uniform
  const int ttid = tid - team * kRolloutThreads;                           // thread within its team
  const int wave = __builtin_amdgcn_readfirstlane(ttid >> 6);              // wave within its team
  const bool is_env = wave >= kRolloutMlpWaves;
  const int n16 = lane & 15, g = lane >> 4;
  const long long ntiles = a.n / kWave;  // (N = P x E, E a multiple of 64: every tile is full)
  const long long t = (long long)blockIdx.x * TEAMS + team;  // this team's tile; >= ntiles: the last block of an odd tile count
  const int T = ea.T;
  const NetLds w = net_lds(net_all[team]);
  float *mus = mus_all[team], *iss = iss_all[team], *tile = tile_all[team];

  // ---- prologue, per team: policy p's network and statistics and the tile's o(0) into LDS -----------------------------
  if (t < ntiles) {
    const long long p = t / ea.tiles_per_policy;
    stage_net(eval_policy_row(ea, p), w, ttid, kRolloutThreads);
    if (ttid < 64) {
      const bool on = ea.mean != nullptr && ttid < D;
      mus[ttid] = on ? ea.mean[p * D + ttid] : 0.f;
      iss[ttid] = on ? 1.0f / (ea.stdv[p * D + ttid] + ea.eps) : 1.f;
    }
    for (int idx = ttid; idx < kWave * D; idx += kRolloutThreads) {
      const int r = idx / D, c = idx - r * D;
      tile[r * TS + c] = ea.obs0[(t * kWave + r) * D + c];
    }
  }
  if (tid < TEAMS) { obs_ready[tid] = 0; act_ready[tid] = 0; }
  if constexpr (eval_keeps_alive_mask(F)) {
    if (tid < TEAMS) es_lds<TEAMS>()[tid] = ~0ull;  // the mask of step 0
  }
  __syncthreads();  // (the only block barrier: from here on the roles meet through the counters)
  if (t >= ntiles) return;

  if (is_env) {
    // ================================ env wave: the tile's 64 envs in registers =================================
#if PDS_ROLLOUT_ENV_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ENV_PRIO);  // the env wave's instructions before its SIMD-mates' (network waves)
#endif
    const long long wave_base = t * kWave;
    const bool active = true;
    const Idx<V> ix{wave_base, (uint32_t)lane};
    PDS_ENV_WAVE_BEGIN
    PDS_EVAL_WAVE_ACCUMULATORS
    // the flight metrics: zero sums; bit 0 / 1 of the second word: wx / wy of the previous state was negative (x(0) has no previous state:
    // its own signs, no crossing)
    float4 *em = nullptr;
    if constexpr (eval_sums_metrics(F)) {
      em = em_lds<TEAMS>() + team * 2 * kWave;
      PDS_EM_INIT(em)
    }
    long long rec_col = -1;  // Record: column of lane 0 in the record, wave-uniform; < 0: this tile does not record
    if constexpr (F == EvalForm::Record) rec_col = eval_record_column(ea, ka.rec_tiles, t);
    for (int s = 0; s < T; ++s) {
      const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<301, true>(ea.s, s));
      PDS_EVAL_STEP_HEAD(&act_ready[team], act_all[team])  // the network waves have read o(s) and written a(s)
      if constexpr (eval_sums_metrics(F)) {  // x(s), the state the policy acted in, and a(s), raw, against u(k - 1) = the last action before the step
        PDS_EM_STEP(em)
      }
      if constexpr (F == EvalForm::Record) {  // x(s) and a(s) where the env is in its first episode: four lines of the record, nothing carried
        if (rec_col >= 0) {
          PDS_ER_STEP(reinterpret_cast<const EvalRecordArgs *>(&el))
        }
      }
      StepOut so;
      step_once<V, kWave, RM, false>(el.s, o1, rks, parity, nullptr, tile, nullptr, queue_all[team], scratch_all[team], lane_s,
                                     wave_base, ix, active, act, S, qcount, nullptr, &so PDS_STAMP_ARG);
      PDS_NEXT_TICK(rk, parity)
      PDS_EVAL_RECORD_STEP(so)
      PDS_EVAL_STILL
      if constexpr (eval_keeps_alive_mask(F)) {
        if (lane == 0) es_lds<TEAMS>()[team] = still;  // the mask of step s + 1, in front of the post
      }
      PDS_EVAL_STEP_TAIL(&obs_ready[team], el)  // o(s + 1) is in the tile / this team's env wave has left
    }
    // (pds_evaluate_policies leaves the handle "not reset")
    PDS_EVAL_WAVE_END(EvalArgs, 302)
    if constexpr (F == EvalForm::Record) {  // (the metrics are summed whether or not the caller takes them)
      if (reinterpret_cast<const EvalMetricsArgs *>(&el)->metrics != nullptr) {
        PDS_EM_STORE(em, reinterpret_cast<const EvalMetricsArgs *>(&el)->metrics)
      }
    } else if constexpr (eval_sums_metrics(F)) {
      PDS_EM_STORE(em, reinterpret_cast<const EvalMetricsArgs *>(&el)->metrics)
    }
    return;
  }

  // ================================ network waves: 16 rows of the tile each ====================================
  const int own = wave * 16 + n16;  // this lane's sample row
  EsSums<NIN, F == EvalForm::Stats> es;  // Stats: the sums of this lane's 4 NIN features of row `own` (nothing otherwise)
  if constexpr (F == EvalForm::Stats) {
#pragma unroll
    for (int kt = 0; kt < NIN; ++kt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { es.s1[kt][q] = 0.f; es.s2[kt][q] = 0.f; }
    }
  }
  long long rec_col = -1;  // Record: as in the env wave; here < 0 also where no observations are asked for
  if constexpr (F == EvalForm::Record) {
    if (ka.obs_rec != nullptr) rec_col = eval_record_column(ea, ka.rec_tiles, t);
  }
  for (int s = 0;; ++s) {
    const EvalArgs &el = *reinterpret_cast<const EvalArgs *>(&reload_args<303, true>(ea.s, s));
    if (eval_wait_ge(&obs_ready[team], s) >= kEvalStop) break;  // o(s) is in the tile, or the env wave has left
#if PDS_ROLLOUT_ACTOR_PRIO
    __builtin_amdgcn_s_setprio(PDS_ROLLOUT_ACTOR_PRIO);
#endif
    f32x4 x_own[NIN];
    gather_input<NIN>(tile, TS, own, D, mus, iss, g, x_own);
    if constexpr (F == EvalForm::Stats) {  // o(s) of row `own`, where its env was alive in front of step s
      const bool al = ((es_lds<TEAMS>()[team] >> own) & 1ull) != 0ull;
#pragma unroll
      for (int kt = 0; kt < NIN; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = kt * 16 + 4 * g + q;  // (gather_input's feature; k >= D: d = 0)
          const float m = mus[k];
          const float d = __fsub_rn((k < D) ? tile[own * TS + k] : m, m);
          es.s1[kt][q] = __fadd_rn(es.s1[kt][q], al ? d : 0.f);
          es.s2[kt][q] = __fadd_rn(es.s2[kt][q], al ? __fmul_rn(d, d) : 0.f);
        }
      }
    }
    if constexpr (F == EvalForm::Record) {  // o(s), raw, of this wave's 16 rows whose env was alive in front of step s: 16 D contiguous floats
      if (rec_col >= 0) {
        const EvalRecordArgs &rl = *reinterpret_cast<const EvalRecordArgs *>(&el);
        const long long nrec = (ntiles / rl.m.e.tiles_per_policy) * rl.rec_tiles * kWave;
        float *out = rl.obs_rec + ((long long)s * nrec + rec_col + wave * 16) * D;
        const unsigned rows = (unsigned)(es_lds<TEAMS>()[team] >> (wave * 16)) & 0xFFFFu;
        for (int idx = lane; idx < 16 * D; idx += kWave) {
          const int r = idx / D, c = idx - r * D;
          if ((rows >> r) & 1u) out[idx] = tile[(wave * 16 + r) * TS + c];
        }
      }
    }
    const f32x4 mu = (el.shape.activation == 0) ? forward16_shape<0, NIN>(w, el.shape, x_own, n16, g) : forward16_shape<1, NIN>(w, el.shape, x_own, n16, g);
    if (g == 0) act_all[team][own] = make_float4(mu[0], mu[1], mu[2], mu[3]);  // lane n16 owns sample `own`: the actor's four outputs
    rollout_post(&act_ready[team], lane);  // this wave is done with the tile of step s
  }
  if constexpr (F == EvalForm::Stats) {  // this wave's 16 rows per feature, then [t][wave][S1 / S2][64]: lane (0, g) stores the features 16 kt + 4 g ..
    float4 *out = reinterpret_cast<float4 *>(ka.obs_sums) + (t * kRolloutMlpWaves + wave) * (2 * 16);
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

// grid.x = number of 64-env tiles; more tiles than CUs: two teams per block (RolloutLaunch's rule) where the two-team form of
// this variant and this kernel form fits (two_teams_fit, csrc/pds_rollout.h, on the form's own two code objects).
template <EvalForm F>
struct EvalLaunchT {
  dim3 grid;
  hipStream_t s;
  const EvalKernelArgs<F> &args;
  template <class RV_>
  void run() const {
    if (grid.x > (unsigned)kRolloutTwoTeamsAbove && two_teams_fit<&evaluate_kernel<RV_, 1, F>, &evaluate_kernel<RV_, 2, F>>())
      hipLaunchKernelGGL((evaluate_kernel<RV_, 2, F>), dim3((grid.x + 1) / 2), dim3(2 * kRolloutThreads), 0, s, args);
    else
      hipLaunchKernelGGL((evaluate_kernel<RV_, 1, F>), grid, dim3(kRolloutThreads), 0, s, args);
  }
};

// ---- the seven launch functions of pds_evaluate_args.h.  flags -> variant is the fused family's one table (fused_task and the
// fused_*_family of csrc/pds_rollout.h) over an EvalLaunchT.  Each function is defined and explicitly instantiated by the
// translation unit that holds its kernels, csrc/pds_evaluate[_metrics|_stats|_record]_<task>[_pwm|_lat].hip, for that unit's
// FORM: a definition every unit could see would instantiate a family's kernels in its task's dispatcher unit as well. ----
// control_mode PWM (FAMILY = fused_pwm_family) or the latency ring (fused_lat_family) of Hover / Circle
#define PDS_EVALUATE_FAMILY_UNIT(NAME, FAMILY, TASK, FORM)                                     \
  template <EvalForm F>                                                                        \
  bool NAME(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka) {     \
    return FAMILY<TASK>(f, EvalLaunchT<F>{grid, s, ka});                                       \
  }                                                                                            \
  template bool NAME<FORM>(const LaunchFlags &, dim3, hipStream_t, const EvalKernelArgs<FORM> &);
// a task's dispatcher + the PID control modes and the Kalman hold; lat, pwm: fused_task's, the unit's own form <F> of the two
// family functions (TakeOff, which holds all its families: nullptr, nullptr)
#define PDS_EVALUATE_TASK_UNIT(NAME, TASK, FORM, lat, pwm)                                     \
  template <EvalForm F>                                                                        \
  bool NAME(const LaunchFlags &f, dim3 grid, hipStream_t s, const EvalKernelArgs<F> &ka) {     \
    return fused_task<TASK>(f, EvalLaunchT<F>{grid, s, ka}, lat, pwm);                         \
  }                                                                                            \
  template bool NAME<FORM>(const LaunchFlags &, dim3, hipStream_t, const EvalKernelArgs<FORM> &);

}  // namespace pds
