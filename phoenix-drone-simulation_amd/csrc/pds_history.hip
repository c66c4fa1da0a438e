// pds_history.hip -- observation histories other than the default of 2 (observation_history_size = H,
// envs/base.py:44, 303-319, 417-431; experiments/04_* use 1, 2, 4, 6, 8).
//
// The step kernel produces the reference's default row [o(k-1), u(k-2), o(k), u(k-1)] (two "halves" of
// |o| + 4 floats).  For another H the env keeps the last H halves of every env, [N, H, half], and one
// launch per step advances them:
//   env still running:   hist' = [hist[1:], newest half]
//   env finished (auto-reset): final = [hist[1:], newest half of its LAST observation (final_obs)]
//                              hist' = [H - 1 copies of the reset row's first half, its second half]
//                              (DroneBaseEnv.reset fills the deques with the first reset observation and
//                               compute_history() appends the next one, envs/base.py:417-431)
// HBM-bound
// (reads H * half + up to 2 * half floats per env, writes H * half, + H * half for a finished env).
// Until round 2 this was a chain of torch.cat / torch.where calls (5 - 25 x the step kernel's own time).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pds.h"
#include "../../include/pds_history_latency.h"

namespace pds_history_detail {

constexpr int kEnvsPerBlock = 64;
constexpr int kStepsCap = 1 << 30;  // the per-env step count of the latency form stops here (the rule looks at counts < H <= 4096)

// One block per 64 envs: their H * half floats each are one contiguous piece of hist' (coalesced 4-B streams);
// (env, slot, float) of an element come from two float multiplications by reciprocals (exact for these
// small integers: the nearest integer boundary is >= 0.5 / (H * half) away), not from integer divisions.
// (Staging the piece through LDS for 16-byte accesses was slower: 403 vs 337 us per step at 2^20 envs, H = 4.)
//
// LAT (pds_history_advance_latency): the latency ring under a history other than 2.  CrazyFlieAgent.reset leaves last_action a
// VIEW of action_buffer[-1] (envs/agents.py:386); DroneBaseEnv.reset puts that view H times into action_history and
// compute_history appends it once more (envs/base.py:424-429), so at the j-th env.step after a reset (j = 1, 2, ...) the action
// columns of the slots 0 .. H - j still show whatever the ring's last row holds NOW.  That row is rewritten by every B-th
// apply_action (B = lat_steps), and an env step makes agg of them with this step's action: when
// floor(j agg / B) > floor((j - 1) agg / B) those columns become the step's raw action, in the final history of an env that
// finishes at step j too; the restart needs nothing (the reset row's u0 already is the new ring's last row).  j - 1 is read from
// steps_in, and steps_out takes j, or 0 behind an auto-reset (two arrays: every thread of an env reads the count one of them
// writes).  A count >= H switches the rule off (what set_latency leaves: the reference allocates a NEW ring there, the views
// keep the old one).
template <bool LAT>
__global__ __launch_bounds__(256) void history_kernel(long long n, int half, int H, const float *__restrict__ obs2,
                                                      const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                                                      const float *__restrict__ final_obs2, int auto_reset,
                                                      const float *__restrict__ hist_in, float *__restrict__ hist_out,
                                                      float *__restrict__ final_hist, const float *__restrict__ act,
                                                      const int32_t *__restrict__ steps_in, int32_t *__restrict__ steps_out,
                                                      int lat_steps, int agg) {
  const int row = H * half;
  const float inv_row = 1.0f / (float)row, inv_half = 1.0f / (float)half;
  const long long env0 = (long long)blockIdx.x * kEnvsPerBlock;
  const int envs = (int)min((long long)kEnvsPerBlock, n - env0);
  const long long base = env0 * row;
  for (int k = threadIdx.x; k < envs * row; k += 256) {
    const int el = (int)(((float)k + 0.5f) * inv_row);
    const int r = k - el * row;
    const int j = (int)(((float)r + 0.5f) * inv_half), c = r - j * half;  // history slot, float within the half
    const long long env = env0 + el;
    const bool done = (term[env] | trunc[env]) != 0;
    const float *o2 = obs2 + env * (2ll * half);
    // the env's history as it stands after this step, before any reset
    float shifted;
    if (j < H - 1) {
      shifted = hist_in[base + k + half];
    } else {
      shifted = (auto_reset && done) ? final_obs2[env * (2ll * half) + half + c] : o2[half + c];
    }
    if (LAT) {
      if (c >= half - 4 && lat_steps > 0) {
        const int before = steps_in[env];  // env.step()s since the env's last reset, in front of this one
        // slots 0 .. H - (before + 1).  (A launcher-made bit table of the steps at which the row is rewritten, in place of the
        // two integer divisions, measured the same: 305 against 307 us at 2^20 envs, H = 4 -- the two dependent loads are the cost.)
        if (j < H - before && (before + 1) * agg / lat_steps > before * agg / lat_steps)
          shifted = act[env * 4 + (c - (half - 4))];
      }
    }
    float out = shifted;
    if (auto_reset && done) {
      if (final_hist != nullptr) final_hist[base + k] = shifted;
      out = (j < H - 1) ? o2[c] : o2[half + c];
    }
    hist_out[base + k] = out;
  }
  if (LAT) {  // the block's step counts, behind the element loop (a store among its loads and stores cost the loop its schedule)
    for (int el = threadIdx.x; el < envs; el += 256) {
      const long long env = env0 + el;
      const int before = steps_in[env];
      steps_out[env] = (auto_reset && (term[env] | trunc[env]) != 0) ? 0 : (before < kStepsCap ? before + 1 : before);
    }
  }
}

}  // namespace pds_history_detail

extern "C" int pds_history_advance(int64_t n, int half, int history, const float *d_obs2, const uint8_t *d_terminated,
                                   const uint8_t *d_truncated, const float *d_final_obs2, int auto_reset,
                                   const float *d_hist_in, float *d_hist_out, float *d_final_hist, void *stream) {
  if (n < 1 || half < 1 || history < 1 || !d_obs2 || !d_terminated || !d_truncated || !d_hist_in || !d_hist_out ||
      d_hist_in == d_hist_out || (auto_reset && !d_final_obs2))
    return PDS_EINVAL;
  if ((long long)history * half > 4096) return PDS_EINVAL;  // (the kernel's index arithmetic is exact up to here)
  const unsigned grid = (unsigned)((n + pds_history_detail::kEnvsPerBlock - 1) / pds_history_detail::kEnvsPerBlock);
  hipLaunchKernelGGL(pds_history_detail::history_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)n, half, history,
                     d_obs2, d_terminated, d_truncated, d_final_obs2, auto_reset, d_hist_in, d_hist_out, d_final_hist,
                     (const float *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, 0, 1);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_history_advance_latency(int64_t n, int half, int history, const float *d_obs2, const uint8_t *d_terminated,
                                           const uint8_t *d_truncated, const float *d_final_obs2, int auto_reset,
                                           const float *d_hist_in, float *d_hist_out, float *d_final_hist, const float *d_actions,
                                           const int32_t *d_steps_in, int32_t *d_steps_out, int lat_steps, int agg, void *stream) {
  if (n < 1 || half < 5 || history < 1 || !d_obs2 || !d_terminated || !d_truncated || !d_hist_in || !d_hist_out ||
      d_hist_in == d_hist_out || (auto_reset && !d_final_obs2) || !d_actions || !d_steps_in || !d_steps_out ||
      d_steps_in == d_steps_out || lat_steps < 0 || agg < 1 || agg > 4096)
    return PDS_EINVAL;
  if ((long long)history * half > 4096) return PDS_EINVAL;  // (the kernel's index arithmetic is exact up to here)
  const unsigned grid = (unsigned)((n + pds_history_detail::kEnvsPerBlock - 1) / pds_history_detail::kEnvsPerBlock);
  hipLaunchKernelGGL(pds_history_detail::history_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)n, half, history,
                     d_obs2, d_terminated, d_truncated, d_final_obs2, auto_reset, d_hist_in, d_hist_out, d_final_hist, d_actions,
                     d_steps_in, d_steps_out, lat_steps, agg);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
