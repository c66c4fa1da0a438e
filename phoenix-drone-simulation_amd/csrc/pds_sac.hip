// pds_sac.hip -- Soft Actor-Critic (algs/sac/sac.py:35-124, 295-337, 439-474) on gfx950: the squashed-Gaussian actor with a
// state-dependent standard deviation, its reparameterised sample with the tanh correction of the log-probability, the
// entropy-regularised backup over the min of twin target Qs, and the gradient of (alpha logp - min(Q1, Q2)).mean() through the
// smaller Q into BOTH heads of the actor.  Read csrc/pds_actor_critic.h first: the argument block, the staging, the critics'
// forward on [obs | action] and their masked backward chain into the action columns, the Bellman write, launch and shape check
// are stated there for this file and csrc/pds_ddpg.hip.  Here: the two heads, the sample, the min-selection and the 8-wide dy.
//
// The actor is ONE pds_mlp with d_out = 8: w3 / b3 = [mu_layer; log_std_layer] stacked.  In the tile core lane (n, 0) holds
// outputs 0 .. 3 of sample n (mu), lane (n, 1) outputs 4 .. 7 (log_std); one xor-16 shuffle brings the two together, and both
// lane groups then evaluate the sample (sac_draw, csrc/pds_explore.h) redundantly -- the same instructions on the same values -- so the
// 8-wide output gradient dy = [dmu | dlog_std] is already in the lanes wide_backward wants it in.
//
// Per 16-sample tile a wave of sac_grad_kernel runs:
//   1  actor forward on the first D columns of the replay row (H1 / H2 to their images)      load_obs, wide_forward<.., 4, true>
//   2  log_std clamped to [-20, 2], eps from the noise contract, u = mu + exp(log_std) eps, a = act_limit tanh(u), logp
//   3  a into columns D .. D + 3 of the X image (put_action); Q1 then Q2 forward on [obs | a], activations in registers   forward_regs
//   4  sel = Q1 <= Q2 per sample; the chosen Q's activations per sample
//   5  da of the chosen Q, in lane groups 0 and 1                                            action_grad<AQ, 2>
//   6  du_j = 2 alpha tanh(u_j) + da_j act_limit (1 - tanh^2 u_j); dmu = du; dlog_std_j = du_j exp(log_std_j) eps_j - alpha where
//      the clamp does not bind (torch.clamp passes the gradient on [-20, 2] inclusive), 0 where it does
//   7  the actor's wide_backward from the 8-wide dy
// The masked double chain costs 80 MFMAs per tile more than one network's (64 for W2q^T dZ2, 16 for Wa) next to about 700;
// nothing cheaper was found, as the A operands (W2q, Wa) differ between the two Qs and a tile's samples choose independently.
// reduce_kernel (csrc/pds_mlp.hip, through launch_reduce) sums the waves' partials in a fixed order, scales by 1 / B
// and may take the Adam step: same inputs, same bits.  Q1 and Q2 are only read.
//
// Noise contract: eps of the sample at POSITION g of the mini-batch (not its buffer row: repeated rows get
// independent noise) = the four variates pds_gaussian_sample draws for sample id id_base + g, block 0, in `call` under `seed`.
//
// LDS budget (D + 4, h1, h2 <= 64; every image at the 68-float stride):
//   per network  W1 64 x 68 + W2 64 x 68 + W3 8 x 68 + biases 144 floats       = 37 568 B, three networks 112 704 B
//   Wa of Q1 and of Q2, 8 x 68 each                                            =  4 352 B
//   per wave     X, H1, H2 16 x 68 each + dY 16 x 20 (the actor's)             = 14 336 B
//   four waves 112 704 + 4 352 + 4 x 14 336 = 174 400 B: over the 163 840 B of a CU.  THREE waves: 160 064 B, which fits.
// Decision: three waves per block (192 threads, one SIMD of the CU idle).  The routes that keep four were weighed and left:
// staging Q2 over the forward-only part of Q1 (W1q) puts two block-wide barriers into every tile and ties the four waves'
// tiles together, where they now run unsynchronised; reading W2q / Wa from L2 in the backward chain turns 96 LDS operand reads
// per lane and tile into global loads on the critical path of a kernel with one wave per SIMD and nothing to hide them behind.
// Three waves lose at most a quarter of the matrix rate at large batches and nothing at B <= 3 x 16 x 256.  Measured: the
// three-wave kernel against autograd (profiles/sac_timing.txt).  NOT measured: a four-wave variant -- none was built.
// The target kernel holds the three networks and one X image per wave: 112 704 + 4 x 4 352 = 130 112 B at four waves.
// Resources the compiler reports for gfx950 (-O3; the range is over the four activation pairs), no kernel uses scratch:
//   sac_grad_kernel    198 .. 203 vector + 156 .. 160 accumulator registers, scratch 0, LDS 160 064 B
//   sac_target_kernel   99 + 12,                                              scratch 0, LDS 130 112 B
//   sac_sample_kernel   28,                                                   scratch 0, LDS       0 B
// Bound: MFMA f32, as the kernels it is built from.
#include <math.h>

#include "pds_actor_critic.h"
#include "pds_device.h"
#include "pds_explore.h"

namespace pds_mlp_detail {

constexpr int kSacWaves = 3;   // waves per block of the gradient kernel (LDS budget above)

// softplus, SacDraw / sac_draw (the squashed-Gaussian sample of one row, stated once for the three kernels here and for the
// network waves of csrc/pds_collect.h) and kLogStdMin / kLogStdMax: csrc/pds_explore.h
using pds_explore::kLogStdMax;
using pds_explore::kLogStdMin;
using pds_explore::sac_draw;
using pds_explore::SacDraw;

// mu and log_std of sample n from the actor's 8 outputs: lane group 0 holds mu, group 1 log_std (groups 2 / 3 hold the aliased
// rows 8 .. 15 and take part in the shuffle only); afterwards BOTH groups of a pair hold both
__device__ __forceinline__ void heads(const f32x4 y, int g, f32x4 &mu, f32x4 &log_std) {
  f32x4 other;
#pragma unroll
  for (int q = 0; q < 4; ++q) other[q] = __shfl_xor(y[q], 16);
  const bool lo = (g & 1) == 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    mu[q] = lo ? y[q] : other[q];
    log_std[q] = lo ? other[q] : y[q];
  }
}

template <int AP, int AQ>
__global__ __launch_bounds__(kSacWaves * 64, 1) void sac_grad_kernel(const AcArgs a) {
  __shared__ __attribute__((aligned(16))) AcLds<2> L;
  __shared__ __attribute__((aligned(16))) float Wa1[kMaxOut * kS], Wa2[kMaxOut * kS];
  __shared__ __attribute__((aligned(16))) float images[kSacWaves * kAcImg];
  const pds_mlp &m = a.pi;
  const WaveTiles w = wave_tiles<kSacWaves>(a.B);
  const int n = w.n, g = w.g;
  L.stage<kSacWaves * 64>(a);
  stage_wa<kSacWaves * 64>(a.q[0], m.d_in, Wa1);
  stage_wa<kSacWaves * 64>(a.q[1], m.d_in, Wa2);
  const NetLds P = L.net(0), Q[2] = {L.net(1), L.net(2)};
  const float *const WaQ[2] = {Wa1, Wa2};
  float *Ximg = images + w.wave * kAcImg;
  float *H1img = Ximg + kTS * kS, *H2img = H1img + kTS * kS, *dYimg = H2img + kTS * kS;
  for (int i = w.lane; i < kAcImg; i += 64) Ximg[i] = 0.f;
  __syncthreads();

  WideGrads<kAcNin> G;
  G.zero();
  float st_q = 0.f, st_logp = 0.f, st_cnt = 0.f;

  for (long long t = w.wid; t < w.ntiles; t += w.nw) {
    const long long row = tile_row(a, t, n);
    const bool valid = row >= 0;
    f32x4 xin[kAcNin], h2p[kNT], mu, lsr;
    load_obs(a, row, Ximg, xin, n, g);
    const f32x4 y = wide_forward<AP, kAcNin, true>(P.W1, P.W2, P.W3, P.b1, P.b2, P.b3, xin, H1img, H2img, h2p, n, g);
    heads(y, g, mu, lsr);
    const SacDraw d = sac_draw(mu, lsr, (unsigned long long)(t * kTS + n), a.call, a.seed, false);
    put_action(a, d.th, Ximg, xin, n, g);
    // ---- Q1 and Q2 on [obs | a]; the Q value sits in register 0 of the lanes (n, 0) -> every lane of sample n -------------------
    f32x4 h1s[kNT], h2s[kNT];  // the CHOSEN Q's activations, per sample
    bool first;
    {
      f32x4 h1a[kNT], h2a[kNT], h1b[kNT], h2b[kNT];
      const f32x4 ya = forward_regs<AQ>(Q[0], xin, h1a, h2a, n, g);
      const f32x4 yb = forward_regs<AQ>(Q[1], xin, h1b, h2b, n, g);
      const float qa = __shfl(ya[0], n), qb = __shfl(yb[0], n);
      first = qa <= qb;
      if (valid && g == 0) { st_q += first ? qa : qb; st_logp += d.logp; st_cnt += 1.f; }
#pragma unroll
      for (int it = 0; it < kNT; ++it)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          h1s[it][q] = first ? h1a[it][q] : h1b[it][q];
          h2s[it][q] = first ? h2a[it][q] : h2b[it][q];
        }
    }
    // ---- da of the smaller Q (lane groups 0 and 1), then the two heads' output gradient -----------------------------------------
    const f32x4 da = action_grad<AQ, 2>(Q, WaQ, h1s, h2s, valid, first, n, g);
    f32x4 dy;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float du = a.alpha * 2.f * d.th[q] + da[q] * a.limit * (1.f - d.th[q] * d.th[q]);
      const bool open = lsr[q] >= kLogStdMin && lsr[q] <= kLogStdMax;
      const float dls = open ? du * d.sig[q] * d.eps[q] - a.alpha : 0.f;
      dy[q] = (valid && g < 2) ? (g == 0 ? du : dls) : 0.f;
    }
    wide_backward<AP, kAcNin, true>(P.W2, P.W3, Ximg, H1img, H2img, dYimg, dy, h2p, G, n, g);
  }

  // ---- this WAVE's partial sums -> partials[wave of the grid][flat parameter layout of the actor + statistics] -------------
  float *out = a.partials + w.wid * a.pstride;
  const Offsets o = offsets(m);
  G.store(m, o, out, n, g);
  store_stats(out, o.total, {st_q, st_logp, 0.f, st_cnt}, w.lane);
}

// target[row] = rew[row] + gamma (1 - done[row]) (min(Q1_targ, Q2_targ)(obs2[row], a2) - alpha logp2), a2 and logp2 from the
// CURRENT policy; every product and sum rounded separately (bellman_write; torch's
// `r + gamma * (1 - d) * (q_pi_targ - alpha * logp_a2)`, algs/sac/sac.py:303-311)
template <int AP, int AQ>
__global__ __launch_bounds__(kWideWaves * 64, 1) void sac_target_kernel(const AcArgs a) {
  __shared__ __attribute__((aligned(16))) AcLds<2> L;
  __shared__ __attribute__((aligned(16))) float images[kWideWaves * kTS * kS];
  const WaveTiles w = wave_tiles<kWideWaves>(a.B);
  const int n = w.n, g = w.g;
  L.stage<kWideWaves * 64>(a);
  const NetLds P = L.net(0), QA = L.net(1), QB = L.net(2);
  float *Ximg = images + w.wave * kTS * kS;
  for (int i = w.lane; i < kTS * kS; i += 64) Ximg[i] = 0.f;
  __syncthreads();
  for (long long t = w.wid; t < w.ntiles; t += w.nw) {
    const long long row = tile_row(a, t, n);
    f32x4 xin[kAcNin], h2p[kNT], h1q[kNT], h2q[kNT], mu, lsr;
    load_obs(a, row, Ximg, xin, n, g);
    const f32x4 y = wide_forward<AP, kAcNin, false>(P.W1, P.W2, P.W3, P.b1, P.b2, P.b3, xin, nullptr, nullptr, h2p, n, g);
    heads(y, g, mu, lsr);
    const SacDraw d = sac_draw(mu, lsr, (unsigned long long)(t * kTS + n), a.call, a.seed, false);
    put_action(a, d.th, Ximg, xin, n, g);
    const f32x4 ya = forward_regs<AQ>(QA, xin, h1q, h2q, n, g);
    const f32x4 yb = forward_regs<AQ>(QB, xin, h1q, h2q, n, g);
    if (row >= 0 && g == 0) bellman_write(a, row, __fsub_rn(fminf(ya[0], yb[0]), __fmul_rn(a.alpha, d.logp)));
    PDS_WAVE_SYNC();  // the X image is rewritten by the next tile
  }
}

// one thread per row of the actor's [n, 8] output: the rollout's action (two launches per vector step with pds_mlp_forward)
__global__ __launch_bounds__(256) void sac_sample_kernel(const float *head, long long n, float limit, unsigned long long seed,
                                                         unsigned long long call, unsigned long long id_base, int deterministic,
                                                         float *act, float *logp) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f32x4 mu = *reinterpret_cast<const f32x4 *>(head + i * 8), ls = *reinterpret_cast<const f32x4 *>(head + i * 8 + 4);
  const SacDraw d = sac_draw(mu, ls, id_base + (unsigned long long)i, call, seed, deterministic != 0);
  f32x4 av;
#pragma unroll
  for (int q = 0; q < 4; ++q) av[q] = limit * d.th[q];
  *reinterpret_cast<f32x4 *>(act + i * 4) = av;
  if (logp != nullptr) logp[i] = d.logp;
}

// ac_check for an actor with 8 outputs, and Q2 a valid network of Q1's shape and activation (else PDS_EINVAL)
static int sac_check(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2) {
  const int rc = ac_check(pi, q1, 8);
  if (rc == PDS_EINVAL || check(q2) != PDS_OK || q2->d_out != 1 || q2->d_in != q1->d_in || q2->h1 != q1->h1 ||
      q2->h2 != q1->h2 || q2->activation != q1->activation)
    return PDS_EINVAL;
  return rc;
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int pds_sac_supported(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2) {
  return (pi && q1 && q2 && sac_check(pi, q1, q2) == PDS_OK) ? 1 : 0;
}

extern "C" int64_t pds_sac_workspace_floats(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2) {
  if (!pi || !q1 || !q2) return PDS_EINVAL;
  const int rc = sac_check(pi, q1, q2);
  if (rc != PDS_OK) return rc;
  return (int64_t)kWideMaxBlocks * kSacWaves * (offsets(*pi).total + kStats);
}

extern "C" int pds_sac_sample(const float *d_head, int64_t n, float act_limit, uint64_t seed, uint64_t call, uint64_t id_base,
                              int deterministic, float *d_act, float *d_logp, void *stream) {
  if (!d_head || !d_act || !sample_ids_ok(id_base, n)) return PDS_EINVAL;
  hipLaunchKernelGGL(sac_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_head,
                     (long long)n, act_limit, (unsigned long long)seed, (unsigned long long)call, (unsigned long long)id_base,
                     deterministic, d_act, d_logp);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_sac_target(const pds_mlp *pi, const pds_mlp *q1_targ, const pds_mlp *q2_targ, const float *d_obs2,
                              const int64_t *d_index, int64_t B, const float *d_rew, const float *d_done, float gamma,
                              float alpha, float act_limit, uint64_t seed, uint64_t call, float *d_target_rows, void *stream) {
  if (!pi || !q1_targ || !q2_targ || !d_obs2 || !d_rew || !d_done || !d_target_rows || B < 1) return PDS_EINVAL;
  const int rc = sac_check(pi, q1_targ, q2_targ);
  if (rc != PDS_OK) return rc;
  AcArgs a{};
  a.pi = *pi; a.q[0] = *q1_targ; a.q[1] = *q2_targ; a.x = d_obs2; a.ldx = pi->d_in; a.index = d_index; a.B = B;
  a.limit = act_limit; a.alpha = alpha; a.seed = seed; a.call = call;
  a.rew = d_rew; a.done = d_done; a.gamma = gamma; a.target = d_target_rows;
  hipStream_t s = (hipStream_t)stream;
  for_activations(a, [&](auto ap, auto aq) {
    hipLaunchKernelGGL((sac_target_kernel<decltype(ap)::value, decltype(aq)::value>), dim3(wide_grid_blocks(B)),
                       dim3(kWideWaves * 64), 0, s, a);
  });
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_sac_policy_grad(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2, const float *d_oa,
                                   const int64_t *d_index, int64_t B, float alpha, float act_limit, uint64_t seed, uint64_t call,
                                   float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream) {
  if (!pi || !q1 || !q2 || !d_oa || !d_grads || !d_stats || !d_workspace || B < 1 ||
      !adam_ok(opt))
    return PDS_EINVAL;
  const int rc = sac_check(pi, q1, q2);
  if (rc != PDS_OK) return rc;
  AcArgs a{};
  a.pi = *pi; a.q[0] = *q1; a.q[1] = *q2; a.x = d_oa; a.ldx = q1->d_in; a.index = d_index; a.B = B;
  a.limit = act_limit; a.alpha = alpha; a.seed = seed; a.call = call;
  const Offsets o = offsets(*pi);
  a.partials = d_workspace;
  a.pstride = o.total + kStats;
  const int blocks = wide_grid_blocks(B, kSacWaves);
  hipStream_t s = (hipStream_t)stream;
  for_activations(a, [&](auto ap, auto aq) {
    hipLaunchKernelGGL((sac_grad_kernel<decltype(ap)::value, decltype(aq)::value>), dim3(blocks), dim3(kSacWaves * 64), 0, s, a);
  });
  return launch_reduce(d_workspace, a.pstride, blocks * kSacWaves, o.total, 1.0f / (float)B, d_grads, d_stats, *pi, opt, s);
}
