// pds_ddpg.hip -- the deterministic policy gradient of DDPG (algs/ddpg/ddpg.py:316-340, 431-464) on gfx950: the actor's loss
// -Q(o, pi(o)).mean() differentiated through the Q network INTO ITS INPUT (the action columns) and on through the actor, the
// Bellman backup of the Q update, and the polyak step of the target networks.
//
// The one operation no on-policy trainer needs is the gradient of a network with respect to its input.  Per 16-sample tile a
// wave runs, on the tile core of csrc/pds_mlp_tile.h (read its header first):
//   1  actor forward on the first D columns of the replay row [obs | act]            wide_forward<.., 4, true>
//   2  a = act_limit tanh(mu)                                                        (tanhf: 4 values per sample)
//   3  Q forward on [obs | a]: a goes into columns D .. D + 3 of the wave's X image, and every lane reads its B operands back
//   4  Q's backward chain from dq = -1, WITHOUT weight-gradient accumulators: dZ2 = -W3q act'(H2q) (one output: no GEMM),
//      dZ1 = (W2q^T dZ2) act'(H1q); H1q and H2q stay in registers, so Q needs no image of its own
//   5  da = W1q[:, D : D + 4]^T dZ1: the four action columns of W1q are staged transposed as an 8-row image (the form of W3's),
//      so da lands in the lanes and registers the actor's output has (lane (n, 0): outputs 0 .. 3 of sample n)
//   6  dmu = da act_limit (1 - tanh^2)
//   7  the actor's wide_backward from dmu into the wave's accumulators (dW2, dW1 on split-bf16 MFMAs, as mlp_wide_kernel)
// ONE X image serves both networks: the actor's staged W1 is zero beyond column D, and its dW1 beyond column D is never stored.
// Every wave writes its partial; ddpg_reduce_kernel sums them in a fixed order (sum_partials: no atomics, same inputs same
// bits), scales by 1 / B and may take the Adam step -- the arithmetic of pds_adam_step / reduce_kernel (csrc/pds_mlp.hip)
// expression for expression.  Q's parameters are only read.
//
// LDS budget (D + 4, h1, h2 <= 64; every image at the 68-float stride of the narrow kernels):
//   per network  W1 64 x 68 + W2 64 x 68 + W3 8 x 68 + biases 144 floats      = 37 568 B, two networks 75 136 B
//   W1q's action columns, transposed, 8 x 68                                  =  2 176 B
//   per wave     X, H1, H2 16 x 68 each + dY 16 x 20 (the ACTOR's; Q has none) = 14 336 B
//   four waves (one per SIMD, up to 512 registers each: the accumulators take 180)  75 136 + 2 176 + 4 x 14 336 = 134 656 B
// of 163 840.  Four waves fit because step 4 keeps Q's activations in registers; with a second set of images for Q (23 KB per
// wave) they would not, and five waves of this form would leave the SIMDs unevenly loaded.  The target kernel holds the two
// networks and one X image per wave (92 544 B).  No register spills: 174 + 160 registers (gradient), 63 + 24 (target).
// Bound: MFMA f32, as the kernels it is built from.
#include <math.h>

#include "pds_explore.h"
#include "pds_mlp_tile.h"

namespace pds_mlp_detail {

constexpr int kDdpgNin = 4;  // input tiles: D + 4 <= 64
static_assert(wide_stride<kDdpgNin>() == kS, "the X image shares the 68-float stride");
constexpr int kDdpgImg = 3 * kTS * kS + kTS * kSY;  // X, H1, H2, dY per wave (gradient kernel)

struct DdpgArgs {
  pds_mlp pi, q;
  const float *x;            // [rows, ldx]: replay rows [obs | act] (gradient), next observations (target)
  int ldx;
  const int64_t *index;      // optional gather: sample g reads row index[g]
  long long B;
  float limit;               // act_limit
  float *partials;           // gradient: [waves of the grid][pstride]
  int pstride;
  const float *rew, *done;   // target: [rows]
  float gamma;
  float *target;             // target: [rows], written at the ROW
};

// Steps 1-3 for one tile: -> Q(o, act_limit tanh(pi(o))) in register 0 of the lanes (n, 0).  th: tanh(mu) (lanes (n, 0):
// outputs 0 .. 3), h2p: the actor's H2, h1q / h2q: Q's activations.  GRAD: the actor's H1 / H2 also go to their images.
template <int AP, int AQ, bool GRAD>
__device__ __forceinline__ f32x4 actor_q_forward(const NetLds &P, const NetLds &Q, const DdpgArgs &a, long long row, float *Ximg,
                                                 float *H1img, float *H2img, f32x4 (&h2p)[kNT], f32x4 (&h1q)[kNT],
                                                 f32x4 (&h2q)[kNT], f32x4 &th, int n, int g) {
  const int D = a.pi.d_in;
  f32x4 xin[kDdpgNin];
#pragma unroll
  for (int kt = 0; kt < kDdpgNin; ++kt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kt * kTW + 4 * g + q;
      xin[kt][q] = (row >= 0 && k < D) ? a.x[row * a.ldx + k] : 0.f;  // (the stored action is not read: 0 x inf)
    }
    sts4(Ximg + n * kS + kt * kTW + 4 * g, xin[kt]);
  }
  const f32x4 mu = wide_forward<AP, kDdpgNin, GRAD>(P.W1, P.W2, P.W3, P.b1, P.b2, P.b3, xin, H1img, H2img, h2p, n, g);
#pragma unroll
  for (int q = 0; q < 4; ++q) th[q] = tanhf(mu[q]);
  PDS_WAVE_SYNC();
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) Ximg[n * kS + D + q] = a.limit * th[q];  // D + 3 <= 63
  }
  PDS_WAVE_SYNC();
#pragma unroll
  for (int kt = 0; kt < kDdpgNin; ++kt) xin[kt] = lds4(Ximg + n * kS + kt * kTW + 4 * g);
  return forward_regs<AQ>(Q, xin, h1q, h2q, n, g);
}

#define PDS_DDPG_NETS()                                                                                                  \
  __shared__ __attribute__((aligned(16))) float W1p[kMaxDim * kS], W2p[kMaxDim * kS], W3p[kMaxOut * kS];                 \
  __shared__ __attribute__((aligned(16))) float W1q[kMaxDim * kS], W2q[kMaxDim * kS], W3q[kMaxOut * kS];                 \
  __shared__ __attribute__((aligned(16))) float b1p[kMaxDim], b2p[kMaxDim], b3p[kTW], b1q[kMaxDim], b2q[kMaxDim], b3q[kTW]; \
  stage_wide<kS>(a.pi, W1p, W2p, W3p, b1p, b2p, b3p, threadIdx.x, [](float t, int) { return t; });                       \
  stage_wide<kS>(a.q, W1q, W2q, W3q, b1q, b2q, b3q, threadIdx.x, [](float t, int) { return t; });                        \
  const NetLds P{W1p, W2p, W3p, b1p, b2p, b3p}, Q{W1q, W2q, W3q, b1q, b2q, b3q}

template <int AP, int AQ>
__global__ __launch_bounds__(kWideWaves * 64, 1) void ddpg_grad_kernel(const DdpgArgs a) {
  PDS_DDPG_NETS();
  __shared__ __attribute__((aligned(16))) float Wa[kMaxOut * kS];  // Wa[r][k] = W1q[k][D + r], r < 4: rows as W3's image
  __shared__ __attribute__((aligned(16))) float images[kWideWaves * kDdpgImg];
  const pds_mlp &m = a.pi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;  // C/D layout: column (sample) n, rows 4 g + q
  for (int i = tid; i < kMaxOut * kS; i += kWideWaves * 64) {
    const int r = i / kS, k = i - r * kS;
    Wa[i] = (r < 4 && k < a.q.h1) ? a.q.w1[k * a.q.d_in + m.d_in + r] : 0.f;
  }
  float *Ximg = images + wave * kDdpgImg;
  float *H1img = Ximg + kTS * kS, *H2img = H1img + kTS * kS, *dYimg = H2img + kTS * kS;
  for (int i = lane; i < kDdpgImg; i += 64) Ximg[i] = 0.f;
  __syncthreads();

  WideGrads<kDdpgNin> G;
  G.zero();
  float st_q = 0.f, st_cnt = 0.f;

  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kWideWaves + wave, nw = (long long)gridDim.x * kWideWaves;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;  // source row of this lane's sample, -1: none
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    const bool valid = row >= 0;
    f32x4 h2p[kNT], h1q[kNT], h2q[kNT], th;
    const f32x4 yq = actor_q_forward<AP, AQ, true>(P, Q, a, row, Ximg, H1img, H2img, h2p, h1q, h2q, th, n, g);
    if (valid && g == 0) { st_q += yq[0]; st_cnt += 1.f; }
    // ---- Q's backward chain from dq = -1 (the loss is -Q.mean(); 1 / B at the reduction), no weight gradients ----------
    f32x4 dz2[kNT], cc[kNT], dz1[kNT];
#pragma unroll
    for (int it = 0; it < kNT; ++it) {  // dZ2 = W3q^T dq * act'(H2q): one output row, no GEMM
      const f32x4 w3 = lds4(W3q + it * kTW + 4 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) dz2[it][q] = valid ? -w3[q] * act_grad<AQ>(h2q[it][q]) : 0.f;
      cc[it] = (f32x4)(0.f);
    }
#pragma unroll
    for (int kt = 0; kt < kNT; ++kt)  // dZ1^T = (W2q^T dZ2^T) * act'(H1q^T), as wide_backward
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int jt = 0; jt < kNT; ++jt) cc[jt] = PDS_MFMA(W2q[(kt * kTW + 4 * g + j) * kS + jt * kTW + n], dz2[kt][j], cc[jt]);
#pragma unroll
    for (int jt = 0; jt < kNT; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q) dz1[jt][q] = cc[jt][q] * act_grad<AQ>(h1q[jt][q]);
    // ---- da = W1q[:, D : D + 4]^T dZ1, dmu = da act_limit (1 - tanh^2): the other lane groups hold aliased rows ---------
    const f32x4 da = gemm_lds<kNT, kS>(Wa, 0, dz1, n & (kMaxOut - 1), g, (f32x4)(0.f));
    f32x4 dmu;
#pragma unroll
    for (int q = 0; q < 4; ++q) dmu[q] = (valid && g == 0) ? da[q] * a.limit * (1.f - th[q] * th[q]) : 0.f;
    wide_backward<AP, kDdpgNin, true>(W2p, W3p, Ximg, H1img, H2img, dYimg, dmu, h2p, G, n, g);
  }

  // ---- this WAVE's partial sums -> partials[wave of the grid][flat parameter layout of the actor + statistics] -------------
  float *out = a.partials + wid * a.pstride;
  const Offsets o = offsets(m);
  G.store(m, o, out, n, g);
  float s4[kStats] = {st_q, 0.f, 0.f, st_cnt};  // lanes of group 0 hold per-sample sums
#pragma unroll
  for (int q = 0; q < kStats; ++q) {
    float v = s4[q];
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) out[o.total + q] = v;
  }
}

// target[row] = rew[row] + gamma (1 - done[row]) Q_targ(obs2[row], act_limit tanh(pi_targ(obs2[row]))), every product and the
// sum rounded separately (torch's `r + gamma * (1 - d) * q_pi_targ`, algs/ddpg/ddpg.py:324-326)
template <int AP, int AQ>
__global__ __launch_bounds__(kWideWaves * 64, 1) void ddpg_target_kernel(const DdpgArgs a) {
  PDS_DDPG_NETS();
  __shared__ __attribute__((aligned(16))) float images[kWideWaves * kTS * kS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  float *Ximg = images + wave * kTS * kS;
  for (int i = lane; i < kTS * kS; i += 64) Ximg[i] = 0.f;
  __syncthreads();
  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kWideWaves + wave, nw = (long long)gridDim.x * kWideWaves;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    f32x4 h2p[kNT], h1q[kNT], h2q[kNT], th;
    const f32x4 yq = actor_q_forward<AP, AQ, false>(P, Q, a, row, Ximg, nullptr, nullptr, h2p, h1q, h2q, th, n, g);
    if (row >= 0 && g == 0)
      a.target[row] = __fadd_rn(a.rew[row], __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.f, a.done[row])), yq[0]));
    PDS_WAVE_SYNC();  // the X image is rewritten by the next tile
  }
}

// The partial-sum kernel of the gradient: reduce_kernel of csrc/pds_mlp.hip, its Adam step included (torch.optim.Adam, the
// arithmetic of pds_adam_step expression for expression, so both routes give the same bits).
struct DdpgAdam {
  float *em, *ev;  // exp_avg, exp_avg_sq [total]; em == nullptr: no step
  float lr, b1, b2, eps, bc1, bc2s;
};

__global__ __launch_bounds__(1024) void ddpg_reduce_kernel(const float *partials, int pstride, int nwaves, int total,
                                                           float denom_scale, float *grads, float *stats, pds_mlp m,
                                                           DdpgAdam ad) {
  const int p = blockIdx.x * 64 + (threadIdx.x & 63);
  const float t = sum_partials(partials, pstride, nwaves, p, p < total + kStats);
  if ((threadIdx.x >> 6) == 0 && p < total + kStats) {
    if (p < total) {
      const float gr = t * denom_scale;
      grads[p] = gr;
      if (ad.em != nullptr) {
        const Offsets o = offsets(m);
        float *dst;
        if (p < o.b1) dst = const_cast<float *>(m.w1) + p;
        else if (p < o.w2) dst = const_cast<float *>(m.b1) + (p - o.b1);
        else if (p < o.b2) dst = const_cast<float *>(m.w2) + (p - o.w2);
        else if (p < o.w3) dst = const_cast<float *>(m.b2) + (p - o.b2);
        else if (p < o.b3) dst = const_cast<float *>(m.w3) + (p - o.w3);
        else dst = const_cast<float *>(m.b3) + (p - o.b3);
        const float mm = ad.b1 * ad.em[p] + (1.f - ad.b1) * gr;
        const float vv = ad.b2 * ad.ev[p] + (1.f - ad.b2) * gr * gr;
        ad.em[p] = mm; ad.ev[p] = vv;
        const float denom = sqrtf(vv) / ad.bc2s + ad.eps;
        *dst = *dst - (ad.lr / ad.bc1) * (mm / denom);
      }
    } else {
      stats[p - total] = t;
    }
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
  if (p < o.b1) { dst = const_cast<float *>(t.w1) + p; src = s.w1 + p; }
  else if (p < o.w2) { dst = const_cast<float *>(t.b1) + (p - o.b1); src = s.b1 + (p - o.b1); }
  else if (p < o.b2) { dst = const_cast<float *>(t.w2) + (p - o.w2); src = s.w2 + (p - o.w2); }
  else if (p < o.w3) { dst = const_cast<float *>(t.b2) + (p - o.b2); src = s.b2 + (p - o.b2); }
  else if (p < o.b3) { dst = const_cast<float *>(t.w3) + (p - o.w3); src = s.w3 + (p - o.w3); }
  else { dst = const_cast<float *>(t.b3) + (p - o.b3); src = s.b3 + (p - o.b3); }
  *dst = __fadd_rn(__fmul_rn(rho, *dst), __fmul_rn(omr, *src));
}

// PDS_OK, PDS_EINVAL (a network outside every kernel family, actor d_out != 4, Q d_out != 1, Q d_in != D + 4) or
// PDS_EUNSUPPORTED (D + 4 > 64)
static int ddpg_check(const pds_mlp *pi, const pds_mlp *q) {
  if (check(pi) != PDS_OK || check(q) != PDS_OK || pi->d_out != 4 || q->d_out != 1 || q->d_in != pi->d_in + 4) return PDS_EINVAL;
  return q->d_in <= kMaxDim ? PDS_OK : PDS_EUNSUPPORTED;
}

int launch_ddpg_reduce(const float *partials, int pstride, int nwaves, int total, float denom_scale, float *grads, float *stats,
                       const pds_mlp &m, const pds_adam *opt, hipStream_t s) {
  DdpgAdam ad{};
  if (opt != nullptr) {
    ad.em = opt->d_exp_avg; ad.ev = opt->d_exp_avg_sq;
    ad.lr = opt->lr; ad.b1 = opt->beta1; ad.b2 = opt->beta2; ad.eps = opt->eps;
    ad.bc1 = 1.0f - powf(opt->beta1, (float)opt->step);  // as pds_adam_step
    ad.bc2s = sqrtf(1.0f - powf(opt->beta2, (float)opt->step));
  }
  const int nred = total + kStats;
  hipLaunchKernelGGL(ddpg_reduce_kernel, dim3((nred + 63) / 64), dim3(1024), 0, s, partials, pstride, nwaves, total,
                     denom_scale, grads, stats, m, ad);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

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

#define PDS_DDPG_LAUNCH(KERNEL, g, s, a)                                                                      \
  do {                                                                                                        \
    const dim3 b_(kWideWaves * 64);                                                                           \
    if ((a).pi.activation == 0) {                                                                             \
      if ((a).q.activation == 0) hipLaunchKernelGGL((KERNEL<0, 0>), g, b_, 0, s, a);                          \
      else hipLaunchKernelGGL((KERNEL<0, 1>), g, b_, 0, s, a);                                                \
    } else {                                                                                                  \
      if ((a).q.activation == 0) hipLaunchKernelGGL((KERNEL<1, 0>), g, b_, 0, s, a);                          \
      else hipLaunchKernelGGL((KERNEL<1, 1>), g, b_, 0, s, a);                                                \
    }                                                                                                         \
  } while (0)

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
      (opt != nullptr && !(opt->d_exp_avg && opt->d_exp_avg_sq && opt->step >= 1)))
    return PDS_EINVAL;
  const int rc = ddpg_check(pi, q);
  if (rc != PDS_OK) return rc;
  DdpgArgs a{};
  a.pi = *pi; a.q = *q; a.x = d_oa; a.ldx = q->d_in; a.index = d_index; a.B = B; a.limit = act_limit;
  const Offsets o = offsets(*pi);
  a.partials = d_workspace;
  a.pstride = o.total + kStats;
  const int blocks = wide_grid_blocks(B);
  hipStream_t s = (hipStream_t)stream;
  PDS_DDPG_LAUNCH(ddpg_grad_kernel, dim3(blocks), s, a);
  return launch_ddpg_reduce(d_workspace, a.pstride, blocks * kWideWaves, o.total, 1.0f / (float)B, d_grads, d_stats, *pi, opt, s);
}

extern "C" int pds_ddpg_target(const pds_mlp *pi_targ, const pds_mlp *q_targ, const float *d_obs2, const int64_t *d_index,
                               int64_t B, const float *d_rew, const float *d_done, float gamma, float act_limit,
                               float *d_target_rows, void *stream) {
  if (!pi_targ || !q_targ || !d_obs2 || !d_rew || !d_done || !d_target_rows || B < 1) return PDS_EINVAL;
  const int rc = ddpg_check(pi_targ, q_targ);
  if (rc != PDS_OK) return rc;
  DdpgArgs a{};
  a.pi = *pi_targ; a.q = *q_targ; a.x = d_obs2; a.ldx = pi_targ->d_in; a.index = d_index; a.B = B; a.limit = act_limit;
  a.rew = d_rew; a.done = d_done; a.gamma = gamma; a.target = d_target_rows;
  hipStream_t s = (hipStream_t)stream;
  PDS_DDPG_LAUNCH(ddpg_target_kernel, dim3(wide_grid_blocks(B)), s, a);
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
  // the id packing of PDS_GAUSSIAN_PHILOX holds sample ids below 2^56
  if (!d_net_out || !d_log_std || !d_act || n < 1 || !(act_limit > 0.f) || id_base > (1ull << 56) ||
      (uint64_t)n > (1ull << 56) - id_base || ((((uintptr_t)d_net_out) | ((uintptr_t)d_act)) & 15u))
    return PDS_EINVAL;
  hipLaunchKernelGGL(ddpg_explore_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_net_out, d_log_std,
                     (long long)n, act_limit, (unsigned long long)seed, (unsigned long long)call, (unsigned long long)id_base, d_act);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
