// pds_sac.hip -- Soft Actor-Critic (algs/sac/sac.py:35-124, 295-337, 439-474) on gfx950: the squashed-Gaussian actor with a
// state-dependent standard deviation, its reparameterised sample with the tanh correction of the log-probability, the
// entropy-regularised backup over the min of twin target Qs, and the gradient of (alpha logp - min(Q1, Q2)).mean() through the
// smaller Q into BOTH heads of the actor.  Read csrc/pds_ddpg.hip first: steps 3-5 of its header are reused as they stand
// (forward_regs, the backward chain without weight-gradient accumulators, the transposed action-column image Wa).
//
// The actor is ONE pds_mlp with d_out = 8: w3 / b3 = [mu_layer; log_std_layer] stacked.  In the tile core lane (n, 0) holds
// outputs 0 .. 3 of sample n (mu), lane (n, 1) outputs 4 .. 7 (log_std); one xor-16 shuffle brings the two together, and both
// lane groups then evaluate the sample (sac_draw, csrc/pds_explore.h) redundantly -- the same instructions on the same values -- so the
// 8-wide output gradient dy = [dmu | dlog_std] is already in the lanes wide_backward wants it in.
//
// Per 16-sample tile a wave of sac_grad_kernel runs:
//   1  actor forward on the first D columns of the replay row (H1 / H2 to their images)      wide_forward<.., 4, true>
//   2  log_std clamped to [-20, 2], eps from the noise contract, u = mu + exp(log_std) eps, a = act_limit tanh(u), logp
//   3  a into columns D .. D + 3 of the X image; Q1 then Q2 forward on [obs | a], activations in registers   forward_regs
//   4  sel = Q1 <= Q2 per sample.  dZ2 of BOTH Qs from dq = -1, each masked to zero for the samples that chose the other; the two
//      W2q^T dZ2 products accumulate into ONE set of tiles (a masked column adds exact zeros), act'(H1q) is the chosen Q's
//   5  da = Wa1 dZ1[sel] + Wa2 dZ1[!sel], again one accumulator.  Rows 4 .. 7 of the Wa images repeat rows 0 .. 3, so lane
//      group 1 holds da as well
//   6  du_j = 2 alpha tanh(u_j) + da_j act_limit (1 - tanh^2 u_j); dmu = du; dlog_std_j = du_j exp(log_std_j) eps_j - alpha where
//      the clamp does not bind (torch.clamp passes the gradient on [-20, 2] inclusive), 0 where it does
//   7  the actor's wide_backward from the 8-wide dy
// The masked double chain costs 80 MFMAs per tile more than one network's (64 for W2q^T dZ2, 16 for Wa) next to about 700;
// nothing cheaper was found, as the A operands (W2q, Wa) differ between the two Qs and a tile's samples choose independently.
// ddpg_reduce_kernel (csrc/pds_ddpg.hip, through launch_ddpg_reduce) sums the waves' partials in a fixed order, scales by 1 / B
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
//   sac_grad_kernel    226 .. 244 vector + 156 .. 160 accumulator registers, scratch 0, LDS 160 064 B
//   sac_target_kernel  111 + 12,                                              scratch 0, LDS 130 112 B
//   sac_sample_kernel   28,                                                   scratch 0, LDS       0 B
// Bound: MFMA f32, as the kernels it is built from.
#include <math.h>

#include "pds_mlp_tile.h"
#include "pds_device.h"
#include "pds_explore.h"

namespace pds_mlp_detail {

constexpr int kSacNin = 4;     // input tiles: D + 4 <= 64
constexpr int kSacWaves = 3;   // waves per block of the gradient kernel (LDS budget above)
static_assert(wide_stride<kSacNin>() == kS, "the X image shares the 68-float stride");
constexpr int kSacImg = 3 * kTS * kS + kTS * kSY;  // X, H1, H2, dY per wave (gradient kernel)

struct SacArgs {
  pds_mlp pi, q1, q2;
  const float *x;            // [rows, ldx]: replay rows [obs | act] (gradient), next observations (target)
  int ldx;
  const int64_t *index;      // optional gather: sample g reads row index[g]
  long long B;
  float limit, alpha;        // act_limit, entropy temperature
  unsigned long long seed, call;
  float *partials;           // gradient: [waves of the grid][pstride]
  int pstride;
  const float *rew, *done;   // target: [rows]
  float gamma;
  float *target;             // target: [rows], written at the ROW
};

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

// this lane's B operands of the first layer from row `row` of a.x (columns < D; the stored action is not read), also into the
// wave's X image
__device__ __forceinline__ void load_obs(const SacArgs &a, long long row, float *Ximg, f32x4 (&xin)[kSacNin], int n, int g) {
  const int D = a.pi.d_in;
#pragma unroll
  for (int kt = 0; kt < kSacNin; ++kt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kt * kTW + 4 * g + q;
      xin[kt][q] = (row >= 0 && k < D) ? a.x[row * a.ldx + k] : 0.f;
    }
    sts4(Ximg + n * kS + kt * kTW + 4 * g, xin[kt]);
  }
}

// a = act_limit th into columns D .. D + 3 of the X image (D + 3 <= 63), then every lane's B operands read back
__device__ __forceinline__ void put_action(const SacArgs &a, const f32x4 th, float *Ximg, f32x4 (&xin)[kSacNin], int n, int g) {
  const int D = a.pi.d_in;
  PDS_WAVE_SYNC();
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) Ximg[n * kS + D + q] = a.limit * th[q];
  }
  PDS_WAVE_SYNC();
#pragma unroll
  for (int kt = 0; kt < kSacNin; ++kt) xin[kt] = lds4(Ximg + n * kS + kt * kTW + 4 * g);
}

#define PDS_SAC_NETS(THREADS)                                                                                            \
  __shared__ __attribute__((aligned(16))) float W1p[kMaxDim * kS], W2p[kMaxDim * kS], W3p[kMaxOut * kS];                 \
  __shared__ __attribute__((aligned(16))) float W1a[kMaxDim * kS], W2a[kMaxDim * kS], W3a[kMaxOut * kS];                 \
  __shared__ __attribute__((aligned(16))) float W1b[kMaxDim * kS], W2b[kMaxDim * kS], W3b[kMaxOut * kS];                 \
  __shared__ __attribute__((aligned(16))) float b1p[kMaxDim], b2p[kMaxDim], b3p[kTW], b1a[kMaxDim], b2a[kMaxDim], b3a[kTW], \
      b1b[kMaxDim], b2b[kMaxDim], b3b[kTW];                                                                              \
  stage_wide<kS, THREADS>(a.pi, W1p, W2p, W3p, b1p, b2p, b3p, threadIdx.x, [](float t, int) { return t; });              \
  stage_wide<kS, THREADS>(a.q1, W1a, W2a, W3a, b1a, b2a, b3a, threadIdx.x, [](float t, int) { return t; });              \
  stage_wide<kS, THREADS>(a.q2, W1b, W2b, W3b, b1b, b2b, b3b, threadIdx.x, [](float t, int) { return t; });              \
  const NetLds P{W1p, W2p, W3p, b1p, b2p, b3p}, QA{W1a, W2a, W3a, b1a, b2a, b3a}, QB{W1b, W2b, W3b, b1b, b2b, b3b}

template <int AP, int AQ>
__global__ __launch_bounds__(kSacWaves * 64, 1) void sac_grad_kernel(const SacArgs a) {
  PDS_SAC_NETS(kSacWaves * 64);
  // Wa[r][k] = W1q[k][D + (r & 3)], r < 8: rows as W3's image, rows 4 .. 7 repeat rows 0 .. 3 (da also in lane group 1)
  __shared__ __attribute__((aligned(16))) float Wa1[kMaxOut * kS], Wa2[kMaxOut * kS];
  __shared__ __attribute__((aligned(16))) float images[kSacWaves * kSacImg];
  const pds_mlp &m = a.pi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;  // C/D layout: column (sample) n, rows 4 g + q
  for (int i = tid; i < kMaxOut * kS; i += kSacWaves * 64) {
    const int r = i / kS, k = i - r * kS;
    Wa1[i] = k < a.q1.h1 ? a.q1.w1[k * a.q1.d_in + m.d_in + (r & 3)] : 0.f;
    Wa2[i] = k < a.q2.h1 ? a.q2.w1[k * a.q2.d_in + m.d_in + (r & 3)] : 0.f;
  }
  float *Ximg = images + wave * kSacImg;
  float *H1img = Ximg + kTS * kS, *H2img = H1img + kTS * kS, *dYimg = H2img + kTS * kS;
  for (int i = lane; i < kSacImg; i += 64) Ximg[i] = 0.f;
  __syncthreads();

  WideGrads<kSacNin> G;
  G.zero();
  float st_q = 0.f, st_logp = 0.f, st_cnt = 0.f;

  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kSacWaves + wave, nw = (long long)gridDim.x * kSacWaves;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;  // source row of this lane's sample, -1: none
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    const bool valid = row >= 0;
    f32x4 xin[kSacNin], h2p[kNT], mu, lsr;
    load_obs(a, row, Ximg, xin, n, g);
    const f32x4 y = wide_forward<AP, kSacNin, true>(P.W1, P.W2, P.W3, P.b1, P.b2, P.b3, xin, H1img, H2img, h2p, n, g);
    heads(y, g, mu, lsr);
    const SacDraw d = sac_draw(mu, lsr, (unsigned long long)(s0 + n), a.call, a.seed, false);
    put_action(a, d.th, Ximg, xin, n, g);
    // ---- Q1 and Q2 on [obs | a]; the Q value sits in register 0 of the lanes (n, 0) -> every lane of sample n -------------------
    f32x4 h1s[kNT], h2s[kNT];  // the CHOSEN Q's activations, per sample
    bool first;
    {
      f32x4 h1a[kNT], h2a[kNT], h1b[kNT], h2b[kNT];
      const f32x4 ya = forward_regs<AQ>(QA, xin, h1a, h2a, n, g);
      const f32x4 yb = forward_regs<AQ>(QB, xin, h1b, h2b, n, g);
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
    // ---- the smaller Q's backward chain from dq = -1: both Qs' operands, the other's dZ masked to zero per sample ----------------
    f32x4 dza[kNT], dzb[kNT], cc[kNT];
#pragma unroll
    for (int it = 0; it < kNT; ++it) {  // dZ2 = W3q^T dq * act'(H2q): one output row, no GEMM
      const f32x4 wa = lds4(W3a + it * kTW + 4 * g), wb = lds4(W3b + it * kTW + 4 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gr = act_grad<AQ>(h2s[it][q]);
        dza[it][q] = (valid && first) ? -wa[q] * gr : 0.f;
        dzb[it][q] = (valid && !first) ? -wb[q] * gr : 0.f;
      }
      cc[it] = (f32x4)(0.f);
    }
#pragma unroll
    for (int kt = 0; kt < kNT; ++kt)  // dZ1^T = (W2q^T dZ2^T) * act'(H1q^T)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int jt = 0; jt < kNT; ++jt) {
          cc[jt] = PDS_MFMA(W2a[(kt * kTW + 4 * g + j) * kS + jt * kTW + n], dza[kt][j], cc[jt]);
          cc[jt] = PDS_MFMA(W2b[(kt * kTW + 4 * g + j) * kS + jt * kTW + n], dzb[kt][j], cc[jt]);
        }
#pragma unroll
    for (int jt = 0; jt < kNT; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = cc[jt][q] * act_grad<AQ>(h1s[jt][q]);
        dza[jt][q] = first ? v : 0.f;
        dzb[jt][q] = first ? 0.f : v;
      }
    // ---- da = W1q[:, D : D + 4]^T dZ1 of the chosen Q (lane groups 0 and 1), then the two heads' output gradient ----------------
    f32x4 da = gemm_lds<kNT, kS>(Wa1, 0, dza, n & (kMaxOut - 1), g, (f32x4)(0.f));
    da = gemm_lds<kNT, kS>(Wa2, 0, dzb, n & (kMaxOut - 1), g, da);
    f32x4 dy;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float du = a.alpha * 2.f * d.th[q] + da[q] * a.limit * (1.f - d.th[q] * d.th[q]);
      const bool open = lsr[q] >= kLogStdMin && lsr[q] <= kLogStdMax;
      const float dls = open ? du * d.sig[q] * d.eps[q] - a.alpha : 0.f;
      dy[q] = (valid && g < 2) ? (g == 0 ? du : dls) : 0.f;
    }
    wide_backward<AP, kSacNin, true>(W2p, W3p, Ximg, H1img, H2img, dYimg, dy, h2p, G, n, g);
  }

  // ---- this WAVE's partial sums -> partials[wave of the grid][flat parameter layout of the actor + statistics] -------------
  float *out = a.partials + wid * a.pstride;
  const Offsets o = offsets(m);
  G.store(m, o, out, n, g);
  float s4[kStats] = {st_q, st_logp, 0.f, st_cnt};  // lanes of group 0 hold per-sample sums
#pragma unroll
  for (int q = 0; q < kStats; ++q) {
    float v = s4[q];
    for (int dd = 8; dd >= 1; dd >>= 1) v += __shfl_xor(v, dd);
    if (lane == 0) out[o.total + q] = v;
  }
}

// target[row] = rew[row] + gamma (1 - done[row]) (min(Q1_targ, Q2_targ)(obs2[row], a2) - alpha logp2), a2 and logp2 from the
// CURRENT policy; every product and sum rounded separately (torch's `r + gamma * (1 - d) * (q_pi_targ - alpha * logp_a2)`,
// algs/sac/sac.py:303-311)
template <int AP, int AQ>
__global__ __launch_bounds__(kWideWaves * 64, 1) void sac_target_kernel(const SacArgs a) {
  PDS_SAC_NETS(kWideWaves * 64);
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
    f32x4 xin[kSacNin], h2p[kNT], h1q[kNT], h2q[kNT], mu, lsr;
    load_obs(a, row, Ximg, xin, n, g);
    const f32x4 y = wide_forward<AP, kSacNin, false>(P.W1, P.W2, P.W3, P.b1, P.b2, P.b3, xin, nullptr, nullptr, h2p, n, g);
    heads(y, g, mu, lsr);
    const SacDraw d = sac_draw(mu, lsr, (unsigned long long)(s0 + n), a.call, a.seed, false);
    put_action(a, d.th, Ximg, xin, n, g);
    const f32x4 ya = forward_regs<AQ>(QA, xin, h1q, h2q, n, g);
    const f32x4 yb = forward_regs<AQ>(QB, xin, h1q, h2q, n, g);
    if (row >= 0 && g == 0) {
      const float soft = __fsub_rn(fminf(ya[0], yb[0]), __fmul_rn(a.alpha, d.logp));
      a.target[row] = __fadd_rn(a.rew[row], __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.f, a.done[row])), soft));
    }
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

// PDS_OK, PDS_EINVAL (a network outside every kernel family, actor d_out != 8, Q d_out != 1, Q d_in != D + 4, Q1 and Q2 of
// different shape or activation) or PDS_EUNSUPPORTED (D + 4 > 64): the rules of ddpg_check
static int sac_check(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2) {
  if (check(pi) != PDS_OK || check(q1) != PDS_OK || check(q2) != PDS_OK || pi->d_out != 8 || q1->d_out != 1 ||
      q1->d_in != pi->d_in + 4 || q2->d_out != 1 || q2->d_in != q1->d_in || q2->h1 != q1->h1 || q2->h2 != q1->h2 ||
      q2->activation != q1->activation)
    return PDS_EINVAL;
  return q1->d_in <= kMaxDim ? PDS_OK : PDS_EUNSUPPORTED;
}

inline int sac_grid_blocks(long long B) {  // wide_grid_blocks for blocks of kSacWaves waves
  const long long tiles = (B + kTS - 1) / kTS;
  const long long blocks = (tiles + kSacWaves - 1) / kSacWaves;
  return (int)(blocks < kWideMaxBlocks ? blocks : kWideMaxBlocks);
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

#define PDS_SAC_LAUNCH(KERNEL, g, b, s, a)                                                                    \
  do {                                                                                                        \
    if ((a).pi.activation == 0) {                                                                             \
      if ((a).q1.activation == 0) hipLaunchKernelGGL((KERNEL<0, 0>), g, b, 0, s, a);                          \
      else hipLaunchKernelGGL((KERNEL<0, 1>), g, b, 0, s, a);                                                 \
    } else {                                                                                                  \
      if ((a).q1.activation == 0) hipLaunchKernelGGL((KERNEL<1, 0>), g, b, 0, s, a);                          \
      else hipLaunchKernelGGL((KERNEL<1, 1>), g, b, 0, s, a);                                                 \
    }                                                                                                         \
  } while (0)

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
  // the id packing of PDS_GAUSSIAN_PHILOX holds sample ids below 2^56
  if (!d_head || !d_act || n < 1 || id_base > (1ull << 56) || (uint64_t)n > (1ull << 56) - id_base) return PDS_EINVAL;
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
  SacArgs a{};
  a.pi = *pi; a.q1 = *q1_targ; a.q2 = *q2_targ; a.x = d_obs2; a.ldx = pi->d_in; a.index = d_index; a.B = B;
  a.limit = act_limit; a.alpha = alpha; a.seed = seed; a.call = call;
  a.rew = d_rew; a.done = d_done; a.gamma = gamma; a.target = d_target_rows;
  hipStream_t s = (hipStream_t)stream;
  PDS_SAC_LAUNCH(sac_target_kernel, dim3(wide_grid_blocks(B)), dim3(kWideWaves * 64), s, a);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_sac_policy_grad(const pds_mlp *pi, const pds_mlp *q1, const pds_mlp *q2, const float *d_oa,
                                   const int64_t *d_index, int64_t B, float alpha, float act_limit, uint64_t seed, uint64_t call,
                                   float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream) {
  if (!pi || !q1 || !q2 || !d_oa || !d_grads || !d_stats || !d_workspace || B < 1 ||
      (opt != nullptr && !(opt->d_exp_avg && opt->d_exp_avg_sq && opt->step >= 1)))
    return PDS_EINVAL;
  const int rc = sac_check(pi, q1, q2);
  if (rc != PDS_OK) return rc;
  SacArgs a{};
  a.pi = *pi; a.q1 = *q1; a.q2 = *q2; a.x = d_oa; a.ldx = q1->d_in; a.index = d_index; a.B = B;
  a.limit = act_limit; a.alpha = alpha; a.seed = seed; a.call = call;
  const Offsets o = offsets(*pi);
  a.partials = d_workspace;
  a.pstride = o.total + kStats;
  const int blocks = sac_grid_blocks(B);
  hipStream_t s = (hipStream_t)stream;
  PDS_SAC_LAUNCH(sac_grad_kernel, dim3(blocks), dim3(kSacWaves * 64), s, a);
  return launch_ddpg_reduce(d_workspace, a.pstride, blocks * kSacWaves, o.total, 1.0f / (float)B, d_grads, d_stats, *pi, opt, s);
}
