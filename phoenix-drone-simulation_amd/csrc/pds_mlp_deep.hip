// pds_mlp_deep.hip -- the trainer's dense kernels for networks with THREE or FOUR hidden layers (include/pds_mlp_deep.h): forward,
// PPO-clip policy gradient and value-regression gradient, each with the Adam step that may ride on its partial-sum kernel.
//
// Who needs it: the reference's architecture search (experiments/01_find_NN_architecture/01_find_NN_architecture.py) grids
// (50, 30, 20), (40, 40, 40), (30, 30, 30), (32, 32, 32, 32) and (25, 25, 25, 25) beside the two-layer shapes; struct pds_mlp has
// room for h1, h2 only, so those networks ran as PyTorch ops.
//
// The design is mlp_wide_kernel's (csrc/pds_mlp_wide.hip, csrc/pds_mlp_tile.h; read those first): a wave owns a 16-sample tile,
// every GEMM of forward and backward runs on v_mfma_f32_16x16x4_f32 with the transposed chain (activations stay in registers from
// layer to layer), the weight gradients accumulate in registers over the wave's tiles, every WAVE writes its partial and a second
// kernel sums the partials in a fixed order.  What changes with the depth L (a template parameter: the layer loops below have
// constant bounds and are unrolled, no layer index is a run-time value):
//   * LDS: L weight images [64][68] + [8][68] of the output layer + biases = 55.4 KB at L = 3, 73.5 KB at L = 4; per wave the
//     images X, H1 .. HL [16][68] and dY [16][20] = 18.7 KB at L = 3, 23.0 KB at L = 4.  Four waves fit the 160 KB at L = 3
//     (130.2 KB); at L = 4 they do not (165.7 KB): the gradient forms at L = 4 run THREE waves per block (142.7 KB), the forward
//     form holds no images and keeps four.  No image can be reused: H(l) is read by the dW GEMM of layer l + 1 after every later
//     layer's image has been read, so all L + 1 are live when the backward chain starts;
//   * registers: 64 accumulators per hidden layer's weight gradient + 16 of the output layer's + 4 L + 4 of the bias gradients
//     (per-lane partial sums) = 292 at L = 4: one wave per SIMD, as in mlp_wide_kernel;
//   * d_in <= 64 only: the first layer is one more [64][68] image (no K-tiling), its four input tiles always multiplied.
// All GEMMs are f32 MFMA; nothing depends on the batch size.
#include "pds_mlp_deep_tile.h"

namespace pds_mlp_detail {

constexpr int kDeepMaxBlocks = 256;  // one persistent block per CU
constexpr int kDeepMaxWaves = 4;
template <int L, int LOSS>
constexpr int deep_waves() { return (L == 4 && LOSS != LOSS_NONE) ? 3 : kDeepMaxWaves; }

struct DeepArgs {
  pds_mlp_deep m;
  const float *x;            // [rows, d_in]
  const int64_t *index;      // optional gather: sample g reads row index[g]
  long long B;               // samples
  const float *mean, *stdv;  // optional input standardisation (x - mean) / (std + eps)
  float eps;
  float *y;                  // forward output [B, d_out]
  const float *act, *adv, *logp_old, *log_std;  // PPO
  const float *target;                          // MSE
  float clip;
  float *partials;           // [waves of the grid][pstride]
  int pstride;
};

template <int LOSS, int ACT, int L>
__global__ __launch_bounds__((deep_waves<L, LOSS>() * 64), 1) void mlp_deep_kernel(const DeepArgs a) {
  constexpr int kW = deep_waves<L, LOSS>(), kThreads = kW * 64;
  constexpr int kI = kTS * kS;
  constexpr int kImg = (LOSS == LOSS_NONE) ? 0 : (L + 1) * kI + kTS * kSY;  // X, H1 .. HL, dY per wave
  __shared__ __attribute__((aligned(16))) float Ws[L * kMaxDim * kS];  // per hidden layer [out][in], zero padded
  __shared__ __attribute__((aligned(16))) float Wos[kMaxOut * kS];     // 8 rows, see stage_wide of csrc/pds_mlp_tile.h
  __shared__ __attribute__((aligned(16))) float bs[L * kMaxDim], bos[kTW], mus[kMaxDim], iss[kMaxDim];
  __shared__ float isg[kTW], lsg[kTW];
  __shared__ __attribute__((aligned(16))) float images[kImg > 0 ? kW * kImg : 4];
  const pds_mlp_deep &m = a.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;  // C/D layout: column (sample) n, rows 4 g + q
  deep_stage<L, kThreads>(m, Ws, Wos, bs, bos, tid, [](float t, int) { return t; });
  if (tid < kMaxDim) {
    const bool std_on = a.mean != nullptr && tid < m.d_in;
    mus[tid] = std_on ? a.mean[tid] : 0.f;
    iss[tid] = std_on ? 1.0f / (a.stdv[tid] + a.eps) : 1.f;
  }
  if (tid < kTW) {
    const float ls = (LOSS == LOSS_PPO && tid < m.d_out) ? a.log_std[tid] : 0.f;
    lsg[tid] = ls;
    isg[tid] = expf(-ls);  // 1 / sigma
  }
  float *img = images + wave * kImg;  // [sample][feature] images for the weight-gradient GEMMs
  if (LOSS != LOSS_NONE)
    for (int i = lane; i < kImg; i += 64) img[i] = 0.f;
  __syncthreads();

  DeepGrads<L> G;
  if constexpr (LOSS != LOSS_NONE) G.zero();  // (the forward form accumulates nothing)
  float st_loss = 0.f, st_ratio = 0.f, st_kl = 0.f, st_cnt = 0.f;

  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kW + wave, nw = (long long)gridDim.x * kW;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;  // source row of this lane's sample, -1: none
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    const bool valid = row >= 0;
    // ---- input: lane (n, g) holds features 16 kt + 4 g + q of its sample = the B operands of layer 1 --
    f32x4 cur[kNT];
#pragma unroll
    for (int kt = 0; kt < kNT; ++kt) {
      const int k0 = kt * kTW + 4 * g;
      const f32x4 mu = lds4(mus + k0), is = lds4(iss + k0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = (valid && k0 + q < m.d_in) ? a.x[row * m.d_in + k0 + q] : mu[q];
        cur[kt][q] = (v - mu[q]) * is[q];
      }
      if (LOSS != LOSS_NONE) sts4(img + n * kS + kt * kTW + 4 * g, cur[kt]);
    }
    float c_act[4] = {0.f, 0.f, 0.f, 0.f}, c_adv = 0.f, c_old = 0.f, c_tgt = 0.f;
    if (LOSS == LOSS_PPO && valid) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (4 * g + q < m.d_out) c_act[q] = a.act[(s0 + n) * m.d_out + 4 * g + q];
      c_adv = a.adv[s0 + n]; c_old = a.logp_old[s0 + n];
    }
    if (LOSS == LOSS_MSE && valid) c_tgt = a.target[row];
    const f32x4 y = deep_forward<ACT, L, LOSS != LOSS_NONE>(Ws, Wos, bs, bos, cur, img, n, g);
    if constexpr (LOSS == LOSS_NONE) {
      if (valid) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * g + q < m.d_out) a.y[(s0 + n) * m.d_out + 4 * g + q] = y[q];
      }
    } else {
      // ---- loss and its gradient with respect to the network output (mlp_wide_kernel, same expressions) -------
      f32x4 dy = (f32x4)(0.f);
      if (LOSS == LOSS_PPO) {  // compute_loss_pi, algs/ppo/ppo.py:22-40
        float lp = 0.f, kl = 0.f;
        f32x4 zs = (f32x4)(0.f);  // z / sigma
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = 4 * g + q;
          if (j < m.d_out) {
            const float z = (c_act[q] - y[q]) * isg[j];
            lp += -0.5f * z * z - lsg[j] - 0.91893853320467274178f;
            kl += 0.5f * z * z;
            zs[q] = z * isg[j];
          }
        }
        lp += __shfl_xor(lp, 16); lp += __shfl_xor(lp, 32);
        kl += __shfl_xor(kl, 16); kl += __shfl_xor(kl, 32);
        const float ratio = expf(lp - c_old);
        const float lo = 1.f - a.clip, hi = 1.f + a.clip;
        const float obj = fminf(ratio * c_adv, fminf(fmaxf(ratio, lo), hi) * c_adv);
        const bool cut = (c_adv > 0.f && ratio > hi) || (c_adv < 0.f && ratio < lo);
        const float gcoef = (cut || !valid) ? 0.f : -c_adv * ratio;  // d(-obj)/d logp
        dy = gcoef * zs;
        if (valid && g == 0) { st_loss += -obj; st_ratio += ratio; st_kl += kl; st_cnt += 1.f; }
      } else {  // compute_loss_v: mse_loss(v(obs), target_v), algs/iwpg/iwpg.py:272-275
        if (valid && g == 0) {
          const float d = y[0] - c_tgt;
          st_loss += d * d; st_cnt += 1.f;
          dy[0] = 2.f * d;
        }
      }
      deep_backward<ACT, L>(Ws, Wos, img, dy, G, n, g);
    }
  }

  if constexpr (LOSS != LOSS_NONE) {
    // ---- this WAVE's partial sums -> partials[wave of the grid][...] (flat parameter layout + statistics) ----------
    float *out = a.partials + wid * a.pstride;
    const DeepOffsets o = deep_offsets(m);
    G.store(m, o, out, n, g);
    store_stats(out, o.total, {st_loss, st_ratio, st_kl, st_cnt}, lane);
  }
}

// reduce_kernel of csrc/pds_mlp.hip for the deep layout: block = 64 outputs x 16 slices of the part range (sum_partials), the
// optimiser step that may ride on it is adam_apply of pds_mlp_common.h, as in deep_adam_kernel
__global__ __launch_bounds__(1024) void deep_reduce_kernel(const float *partials, int pstride, int nwaves, int total,
                                                           float denom_scale, float *grads, float *stats, pds_mlp_deep m,
                                                           AdamK ad) {
  const int p = blockIdx.x * 64 + (threadIdx.x & 63);
  const float t = sum_partials(partials, pstride, nwaves, p, p < total + kStats);
  if ((threadIdx.x >> 6) == 0 && p < total + kStats) {
    if (p < total) {
      const float gr = t * denom_scale;
      grads[p] = gr;
      if (ad.em != nullptr) adam_apply(ad, p, gr, deep_param_ptr(m, p));
    } else {
      stats[p - total] = t;
    }
  }
}

// torch.optim.Adam on the flat gradient of one deep MLP (adam_apply), one thread per parameter
__global__ __launch_bounds__(256) void deep_adam_kernel(pds_mlp_deep m, const float *g, int total, AdamK ad) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  adam_apply(ad, p, g[p], deep_param_ptr(m, p));
}

// blocks of `waves` waves, one 16-sample tile per wave and round
static int deep_grid_blocks(long long B, int waves) {
  const long long tiles = (B + kTS - 1) / kTS;
  const long long blocks = (tiles + waves - 1) / waves;
  return (int)(blocks < kDeepMaxBlocks ? blocks : kDeepMaxBlocks);
}

template <int LOSS>
static int deep_launch(const DeepArgs &a, hipStream_t s) {  // -> waves of the grid
  const int L = a.m.n_hidden, waves = L == 4 ? deep_waves<4, LOSS>() : deep_waves<3, LOSS>();
  const dim3 g(deep_grid_blocks(a.B, waves)), b(waves * 64);
  if (L == 3) {
    if (a.m.activation == 0) hipLaunchKernelGGL((mlp_deep_kernel<LOSS, 0, 3>), g, b, 0, s, a);
    else hipLaunchKernelGGL((mlp_deep_kernel<LOSS, 1, 3>), g, b, 0, s, a);
  } else {
    if (a.m.activation == 0) hipLaunchKernelGGL((mlp_deep_kernel<LOSS, 0, 4>), g, b, 0, s, a);
    else hipLaunchKernelGGL((mlp_deep_kernel<LOSS, 1, 4>), g, b, 0, s, a);
  }
  return (int)g.x * waves;
}

template <int LOSS>
static int deep_launch_grad(DeepArgs &a, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt, void *stream) {
  const int total = deep_offsets(a.m).total;
  hipStream_t s = (hipStream_t)stream;
  a.partials = d_workspace;
  a.pstride = total + kStats;
  const int parts = deep_launch<LOSS>(a, s);
  hipLaunchKernelGGL(deep_reduce_kernel, dim3((total + kStats + 63) / 64), dim3(1024), 0, s, d_workspace, a.pstride, parts, total,
                     1.0f / (float)a.B, d_grads, d_stats, a.m, adam_k(opt));
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int pds_mlp_deep_supported(const pds_mlp_deep *m) { return deep_check(m) == PDS_OK && m->d_in <= kMaxDim ? 1 : 0; }

extern "C" int pds_mlp_deep_param_count(const pds_mlp_deep *m) {
  if (deep_check(m) != PDS_OK) return PDS_EINVAL;
  return deep_offsets(*m).total;
}

extern "C" int64_t pds_mlp_deep_workspace_floats(const pds_mlp_deep *m) {
  if (deep_check(m) != PDS_OK) return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  return (int64_t)kDeepMaxBlocks * kDeepMaxWaves * (deep_offsets(*m).total + kStats);  // one partial per WAVE of the grid
}

extern "C" int pds_mlp_deep_forward(const pds_mlp_deep *m, const float *d_x, const int64_t *d_index, int64_t B, const float *d_mean,
                                    const float *d_std, float eps, float *d_y, void *stream) {
  if (deep_check(m) != PDS_OK || !d_x || !d_y || B < 1 || ((d_mean == nullptr) != (d_std == nullptr))) return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  DeepArgs a{};
  a.m = *m; a.x = d_x; a.index = d_index; a.B = B; a.mean = d_mean; a.stdv = d_std; a.eps = eps; a.y = d_y;
  deep_launch<LOSS_NONE>(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_mlp_deep_ppo_policy_grad_step(const pds_mlp_deep *m, const float *d_x, const float *d_act, const float *d_adv,
                                                 const float *d_logp_old, const float *d_log_std, int64_t B, float clip_ratio,
                                                 float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                                                 void *stream) {
  if (deep_check(m) != PDS_OK || !d_x || !d_act || !d_adv || !d_logp_old || !d_log_std || !d_grads || !d_stats || !d_workspace ||
      B < 1 || !adam_ok(opt))
    return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  DeepArgs a{};
  a.m = *m; a.x = d_x; a.B = B; a.act = d_act; a.adv = d_adv; a.logp_old = d_logp_old; a.log_std = d_log_std;
  a.clip = clip_ratio;
  return deep_launch_grad<LOSS_PPO>(a, d_grads, d_stats, d_workspace, opt, stream);
}

extern "C" int pds_mlp_deep_value_grad_step(const pds_mlp_deep *m, const float *d_x, const int64_t *d_index, const float *d_target,
                                            int64_t B, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                                            void *stream) {
  if (deep_check(m) != PDS_OK || m->d_out != 1 || !d_x || !d_target || !d_grads || !d_stats || !d_workspace || B < 1 ||
      !adam_ok(opt))
    return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  DeepArgs a{};
  a.m = *m; a.x = d_x; a.index = d_index; a.B = B; a.target = d_target;
  return deep_launch_grad<LOSS_MSE>(a, d_grads, d_stats, d_workspace, opt, stream);
}

extern "C" int pds_mlp_deep_adam_step(const pds_mlp_deep *m, const float *d_grads, float *d_exp_avg, float *d_exp_avg_sq,
                                      int64_t step, float lr, float beta1, float beta2, float eps, void *stream) {
  const pds_adam opt{d_exp_avg, d_exp_avg_sq, step, lr, beta1, beta2, eps};
  if (deep_check(m) != PDS_OK || !d_grads || !adam_ok(&opt)) return PDS_EINVAL;
  const int total = deep_offsets(*m).total;
  hipLaunchKernelGGL(deep_adam_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, d_grads, total,
                     adam_k(&opt));
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
