// pds_ddpg.hip -- the deterministic policy gradient of DDPG (algs/ddpg/ddpg.py:316-340, 431-464) on gfx950: the actor's loss
// -Q(o, pi(o)).mean() differentiated through the Q network INTO ITS INPUT (the action columns) and on through the actor, the
// Bellman backup of the Q update, and the polyak step of the target networks.
//
// The shared part -- argument block, staging, the critic's forward on [obs | action] and its backward chain into the action
// columns, the Bellman write, launch and shape check -- is csrc/pds_actor_critic.h (read its header first).  This file holds what
// is DDPG's: per 16-sample tile a wave of ddpg_grad_kernel runs
//   1  actor forward on the first D columns of the replay row [obs | act]            load_obs, wide_forward<.., 4, true>
//   2  a = act_limit tanh(mu)                                                        (tanhf: 4 values per sample), put_action
//   3  Q forward on [obs | a], its activations in registers                          forward_regs
//   4  da = d(-Q) / da                                                               action_grad<AQ, 1>
//   5  dmu = da act_limit (1 - tanh^2)
//   6  the actor's wide_backward from dmu into the wave's accumulators (dW2, dW1 on split-bf16 MFMAs, as mlp_wide_kernel)
// The actor's dW1 beyond column D is never stored.  Every wave writes its partial; reduce_kernel (csrc/pds_mlp.hip, through
// launch_reduce) sums them in a fixed order (sum_partials: no atomics, same inputs same bits), scales by 1 / B and may take the
// Adam step of pds_adam_step.  Q's parameters are only read.  Also here: the polyak step of the target networks and DDPG's
// exploration action.
//
// LDS budget (D + 4, h1, h2 <= 64; every image at the 68-float stride of the narrow kernels):
//   per network  W1 64 x 68 + W2 64 x 68 + W3 8 x 68 + biases 144 floats      = 37 568 B, two networks 75 136 B
//   W1q's action columns, transposed, 8 x 68                                  =  2 176 B
//   per wave     X, H1, H2 16 x 68 each + dY 16 x 20 (the ACTOR's; Q has none) = 14 336 B
//   four waves (one per SIMD, up to 512 registers each: the accumulators take 180)  75 136 + 2 176 + 4 x 14 336 = 134 656 B
// of 163 840.  Four waves fit because the chain keeps Q's activations in registers; with a second set of images for Q (23 KB per
// wave) they would not, and five waves of this form would leave the SIMDs unevenly loaded.  The target kernel holds the two
// networks and one X image per wave (92 544 B).  No register spills: 162 + 160 .. 164 registers (gradient), 55 + 24 (target).
// Bound: MFMA f32, as the kernels it is built from.
#include <math.h>

#include "pds_actor_critic.h"
#include "pds_explore.h"

namespace pds_mlp_detail {

// Steps 1-3 for one tile: -> Q(o, act_limit tanh(pi(o))) in register 0 of the lanes (n, 0).  th: tanh(mu) (lanes (n, 0):
// outputs 0 .. 3), h2p: the actor's H2, h1q / h2q: Q's activations.  GRAD: the actor's H1 / H2 also go to their images.
template <int AP, int AQ, bool GRAD>
__device__ __forceinline__ f32x4 actor_q_forward(const NetLds &P, const NetLds &Q, const AcArgs &a, long long row, float *Ximg,
                                                 float *H1img, float *H2img, f32x4 (&h2p)[kNT], f32x4 (&h1q)[kNT],
                                                 f32x4 (&h2q)[kNT], f32x4 &th, int n, int g) {
  f32x4 xin[kAcNin];
  load_obs(a, row, Ximg, xin, n, g);
  const f32x4 mu = wide_forward<AP, kAcNin, GRAD>(P.W1, P.W2, P.W3, P.b1, P.b2, P.b3, xin, H1img, H2img, h2p, n, g);
#pragma unroll
  for (int q = 0; q < 4; ++q) th[q] = tanhf(mu[q]);
  put_action(a, th, Ximg, xin, n, g);
  return forward_regs<AQ>(Q, xin, h1q, h2q, n, g);
}

template <int AP, int AQ>
__global__ __launch_bounds__(kWideWaves * 64, 1) void ddpg_grad_kernel(const AcArgs a) {
  __shared__ __attribute__((aligned(16))) AcLds<1> L;
  __shared__ __attribute__((aligned(16))) float Wa[kMaxOut * kS];  // (only rows 0 .. 3 are used: dmu lives in lane group 0)
  __shared__ __attribute__((aligned(16))) float images[kWideWaves * kAcImg];
  const pds_mlp &m = a.pi;
  const WaveTiles w = wave_tiles<kWideWaves>(a.B);
  const int n = w.n, g = w.g;
  L.stage<kWideWaves * 64>(a);
  stage_wa<kWideWaves * 64>(a.q[0], m.d_in, Wa);
  const NetLds P = L.net(0), Q[1] = {L.net(1)};
  const float *const WaQ[1] = {Wa};
  float *Ximg = images + w.wave * kAcImg;
  float *H1img = Ximg + kTS * kS, *H2img = H1img + kTS * kS, *dYimg = H2img + kTS * kS;
  for (int i = w.lane; i < kAcImg; i += 64) Ximg[i] = 0.f;
  __syncthreads();

  WideGrads<kAcNin> G;
  G.zero();
  float st_q = 0.f, st_cnt = 0.f;

  for (long long t = w.wid; t < w.ntiles; t += w.nw) {
    const long long row = tile_row(a, t, n);
    const bool valid = row >= 0;
    f32x4 h2p[kNT], h1q[kNT], h2q[kNT], th;
    const f32x4 yq = actor_q_forward<AP, AQ, true>(P, Q[0], a, row, Ximg, H1img, H2img, h2p, h1q, h2q, th, n, g);
    if (valid && g == 0) { st_q += yq[0]; st_cnt += 1.f; }
    const f32x4 da = action_grad<AQ, 1>(Q, WaQ, h1q, h2q, valid, true, n, g);
    f32x4 dmu;
#pragma unroll
    for (int q = 0; q < 4; ++q) dmu[q] = (valid && g == 0) ? da[q] * a.limit * (1.f - th[q] * th[q]) : 0.f;
    wide_backward<AP, kAcNin, true>(P.W2, P.W3, Ximg, H1img, H2img, dYimg, dmu, h2p, G, n, g);
  }

  // ---- this WAVE's partial sums -> partials[wave of the grid][flat parameter layout of the actor + statistics] -------------
  float *out = a.partials + w.wid * a.pstride;
  const Offsets o = offsets(m);
  G.store(m, o, out, n, g);
  store_stats(out, o.total, {st_q, 0.f, 0.f, st_cnt}, w.lane);
}

// target[row] = rew[row] + gamma (1 - done[row]) Q_targ(obs2[row], act_limit tanh(pi_targ(obs2[row]))) (bellman_write;
// algs/ddpg/ddpg.py:324-326)
template <int AP, int AQ>
__global__ __launch_bounds__(kWideWaves * 64, 1) void ddpg_target_kernel(const AcArgs a) {
  __shared__ __attribute__((aligned(16))) AcLds<1> L;
  __shared__ __attribute__((aligned(16))) float images[kWideWaves * kTS * kS];
  const WaveTiles w = wave_tiles<kWideWaves>(a.B);
  const int n = w.n, g = w.g;
  L.stage<kWideWaves * 64>(a);
  const NetLds P = L.net(0), Q = L.net(1);
  float *Ximg = images + w.wave * kTS * kS;
  for (int i = w.lane; i < kTS * kS; i += 64) Ximg[i] = 0.f;
  __syncthreads();
  for (long long t = w.wid; t < w.ntiles; t += w.nw) {
    const long long row = tile_row(a, t, n);
    f32x4 h2p[kNT], h1q[kNT], h2q[kNT], th;
    const f32x4 yq = actor_q_forward<AP, AQ, false>(P, Q, a, row, Ximg, nullptr, nullptr, h2p, h1q, h2q, th, n, g);
    if (row >= 0 && g == 0) bellman_write(a, row, yq[0]);
    PDS_WAVE_SYNC();  // the X image is rewritten by the next tile
  }
}

// t = rn(rn(rho t) + rn(omr s)) over the six tensors of a network (p_targ.mul_(polyak); p_targ.add_((1 - polyak) * p),
// algs/ddpg/ddpg.py:459-464: two in-place ops, the scalars rounded to float32)
__global__ __launch_bounds__(256) void polyak_kernel(pds_mlp t, pds_mlp s, int total, float rho, float omr) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const Offsets o = offsets(t);
  float *dst;
  const float *src;
  at_param(o, p, [&](const float *pds_mlp::*w, int i) { dst = const_cast<float *>(t.*w) + i; src = s.*w + i; });
  *dst = __fadd_rn(__fmul_rn(rho, *dst), __fmul_rn(omr, *src));
}

static int ddpg_check(const pds_mlp *pi, const pds_mlp *q) { return ac_check(pi, q, 4); }

// one thread per row of the actor's [n, 4] pre-tanh output: DDPG's exploration action (csrc/pds_explore.h ddpg_explore, the device
// function the network waves of csrc/pds_collect.h call), z = the variates of pds_gaussian_sample for sample id id_base + i
__global__ __launch_bounds__(256) void ddpg_explore_kernel(const float *net, const float *log_std, long long n, float limit,
                                                           unsigned long long seed, unsigned long long call,
                                                           unsigned long long id_base, float *act) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pds_explore::f32x4 y = *reinterpret_cast<const pds_explore::f32x4 *>(net + i * 4);
  const pds_explore::f32x4 ls = {log_std[0], log_std[1], log_std[2], log_std[3]};
  const pds_explore::f32x4 z = pds_explore::gaussian_draw4(id_base + (unsigned long long)i, call, seed);
  *reinterpret_cast<pds_explore::f32x4 *>(act + i * 4) = pds_explore::ddpg_explore(y, ls, z, limit);
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int pds_ddpg_supported(const pds_mlp *pi, const pds_mlp *q) { return ddpg_check(pi, q) == PDS_OK ? 1 : 0; }

extern "C" int64_t pds_ddpg_workspace_floats(const pds_mlp *pi, const pds_mlp *q) {
  const int rc = ddpg_check(pi, q);
  if (rc != PDS_OK) return rc;
  return (int64_t)kWideMaxBlocks * kWideWaves * (offsets(*pi).total + kStats);
}

extern "C" int pds_ddpg_policy_grad(const pds_mlp *pi, const pds_mlp *q, const float *d_oa, const int64_t *d_index, int64_t B,
                                    float act_limit, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                                    void *stream) {
  if (!pi || !q || !d_oa || !d_grads || !d_stats || !d_workspace || B < 1 ||
      !adam_ok(opt))
    return PDS_EINVAL;
  const int rc = ddpg_check(pi, q);
  if (rc != PDS_OK) return rc;
  AcArgs a{};
  a.pi = *pi; a.q[0] = *q; a.x = d_oa; a.ldx = q->d_in; a.index = d_index; a.B = B; a.limit = act_limit;
  const Offsets o = offsets(*pi);
  a.partials = d_workspace;
  a.pstride = o.total + kStats;
  const int blocks = wide_grid_blocks(B);
  hipStream_t s = (hipStream_t)stream;
  for_activations(a, [&](auto ap, auto aq) {
    hipLaunchKernelGGL((ddpg_grad_kernel<decltype(ap)::value, decltype(aq)::value>), dim3(blocks), dim3(kWideWaves * 64), 0, s, a);
  });
  return launch_reduce(d_workspace, a.pstride, blocks * kWideWaves, o.total, 1.0f / (float)B, d_grads, d_stats, *pi, opt, s);
}

extern "C" int pds_ddpg_target(const pds_mlp *pi_targ, const pds_mlp *q_targ, const float *d_obs2, const int64_t *d_index,
                               int64_t B, const float *d_rew, const float *d_done, float gamma, float act_limit,
                               float *d_target_rows, void *stream) {
  if (!pi_targ || !q_targ || !d_obs2 || !d_rew || !d_done || !d_target_rows || B < 1) return PDS_EINVAL;
  const int rc = ddpg_check(pi_targ, q_targ);
  if (rc != PDS_OK) return rc;
  AcArgs a{};
  a.pi = *pi_targ; a.q[0] = *q_targ; a.x = d_obs2; a.ldx = pi_targ->d_in; a.index = d_index; a.B = B; a.limit = act_limit;
  a.rew = d_rew; a.done = d_done; a.gamma = gamma; a.target = d_target_rows;
  hipStream_t s = (hipStream_t)stream;
  for_activations(a, [&](auto ap, auto aq) {
    hipLaunchKernelGGL((ddpg_target_kernel<decltype(ap)::value, decltype(aq)::value>), dim3(wide_grid_blocks(B)),
                       dim3(kWideWaves * 64), 0, s, a);
  });
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_polyak(const pds_mlp *targ, const pds_mlp *src, double polyak, void *stream) {
  if (check(targ) != PDS_OK || check(src) != PDS_OK || targ->d_in != src->d_in || targ->h1 != src->h1 || targ->h2 != src->h2 ||
      targ->d_out != src->d_out || !(polyak >= 0.0 && polyak <= 1.0))
    return PDS_EINVAL;
  const int total = offsets(*targ).total;
  hipLaunchKernelGGL(polyak_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, *targ, *src, total,
                     (float)polyak, (float)(1.0 - polyak));
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_ddpg_explore(const float *d_net_out, const float *d_log_std, int64_t n, float act_limit, uint64_t seed,
                                uint64_t call, uint64_t id_base, float *d_act, void *stream) {
  if (!d_net_out || !d_log_std || !d_act || !(act_limit > 0.f) || !sample_ids_ok(id_base, n) ||
      ((((uintptr_t)d_net_out) | ((uintptr_t)d_act)) & 15u))
    return PDS_EINVAL;
  hipLaunchKernelGGL(ddpg_explore_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_net_out, d_log_std,
                     (long long)n, act_limit, (unsigned long long)seed, (unsigned long long)call, (unsigned long long)id_base, d_act);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
