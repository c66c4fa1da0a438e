// pds_mlp_wide.hip -- the trainer's dense kernels for networks with MORE than 64 inputs (64 < d_in <= 192): the first layer
// K-tiled over up to twelve 16-wide input tiles.
//
// Who needs it: `observation_history_size` >= 4 (envs/base.py:303-319: the observation is the last H [o, u] halves) --
// Hover 68 / 102 / 136 inputs at H = 4 / 6 / 8, Circle 80 / 120 / 160, TakeOff 96 / 144 / 192; what the reference's
// experiments/04_history_of_state_action_inputs/04_train_with_history.py:34 trains (H in {1, 2, 4, 6, 8}, policy 32-32 / 48-48 /
// 64-64 relu, critic 64-64 tanh).  Rounds 1-5 dropped both networks to PyTorch ops there (7 launches per rollout step +
// autograd: the round-1 path).
//
// The tile core -- row stride, grid size, weight staging, the weight-gradient accumulators and their write-out, the backward
// chain -- is csrc/pds_mlp_tile.h (its header states the design and what the width changes against mlp_kernel of
// csrc/pds_mlp.hip; read that first), shared with the natural-gradient kernels of csrc/pds_npg.hip.  Here: the kernel's own
// forward pass (layer tiles in pairs), the two losses, the statistics, and the dispatch over the input tiles.  The gradient
// forms take dW2 and dW1 on split-bf16 MFMAs (wide_backward<.., true>, round 6; pds_npg.hip runs the f32 chain).
// Bound: MFMA f32, as the narrow kernels.
#include "pds_mlp_tile.h"

namespace pds_mlp_detail {

template <int LOSS, int ACT, int NIN>
__global__ __launch_bounds__(kWideWaves * 64, 1) void mlp_wide_kernel(const Args a) {
  constexpr int S1 = wide_stride<NIN>();
  constexpr int kImg = (LOSS == LOSS_NONE) ? 0 : kTS * S1 + 2 * kTS * kS + kTS * kSY;  // X, H1, H2, dY per wave
  __shared__ __attribute__((aligned(16))) float W1s[kMaxDim * S1];  // [out][in], zero padded
  __shared__ __attribute__((aligned(16))) float W2s[kMaxDim * kS];
  __shared__ __attribute__((aligned(16))) float W3s[kMaxOut * kS];  // 8 rows, see stage_wide
  __shared__ __attribute__((aligned(16))) float b1s[kMaxDim], b2s[kMaxDim], b3s[kTW], mus[kTW * NIN], iss[kTW * NIN];
  __shared__ float isg[kTW], lsg[kTW];
  __shared__ __attribute__((aligned(16))) float images[kImg > 0 ? kWideWaves * kImg : 4];
  const pds_mlp &m = a.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;  // C/D layout: column (sample) n, rows 4 g + q
  constexpr int kThreads = kWideWaves * 64;
  stage_wide<S1>(m, W1s, W2s, W3s, b1s, b2s, b3s, tid, [](float t, int) { return t; });
  for (int i = tid; i < kTW * NIN; i += kThreads) {
    const bool std_on = a.mean != nullptr && i < m.d_in;
    mus[i] = std_on ? a.mean[i] : 0.f;
    iss[i] = std_on ? 1.0f / (a.stdv[i] + a.eps) : 1.f;
  }
  if (tid < kTW) {
    const float ls = (LOSS == LOSS_PPO && tid < m.d_out) ? a.log_std[tid] : 0.f;
    lsg[tid] = ls;
    isg[tid] = expf(-ls);  // 1 / sigma
  }
  float *Ximg = images + wave * kImg;  // [sample][feature] images for the weight-gradient GEMMs
  float *H1img = Ximg + kTS * S1, *H2img = H1img + kTS * kS, *dYimg = H2img + kTS * kS;
  if (LOSS != LOSS_NONE)
    for (int i = lane; i < kImg; i += 64) Ximg[i] = 0.f;
  __syncthreads();

  constexpr int NG1 = (LOSS == LOSS_NONE) ? 1 : NIN;  // (the forward form accumulates nothing)
  WideGrads<NG1> G;
  G.zero();
  float st_loss = 0.f, st_ratio = 0.f, st_kl = 0.f, st_cnt = 0.f;

  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kWideWaves + wave, nw = (long long)gridDim.x * kWideWaves;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;  // source row of this lane's sample, -1: none
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    const bool valid = row >= 0;
    // ---- input: lane (n, g) holds features 16 kt + 4 g + q of its sample = the B operands of layer 1 --
    f32x4 xin[NIN];
#pragma unroll
    for (int kt = 0; kt < NIN; ++kt) {
      const int k0 = kt * kTW + 4 * g;
      const f32x4 mu = lds4(mus + k0), is = lds4(iss + k0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = (valid && k0 + q < m.d_in) ? a.x[row * m.d_in + k0 + q] : mu[q];
        xin[kt][q] = (v - mu[q]) * is[q];
      }
      if (LOSS != LOSS_NONE) sts4(Ximg + n * S1 + kt * kTW + 4 * g, xin[kt]);
    }
    float c_act[4] = {0.f, 0.f, 0.f, 0.f}, c_adv = 0.f, c_old = 0.f, c_tgt = 0.f;
    if (LOSS == LOSS_PPO && valid) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (4 * g + q < m.d_out) c_act[q] = a.act[(s0 + n) * m.d_out + 4 * g + q];
      c_adv = a.adv[s0 + n]; c_old = a.logp_old[s0 + n];
    }
    if (LOSS == LOSS_MSE && valid) c_tgt = a.target[row];
    f32x4 h2r[kNT];
    const f32x4 y = wide_forward<ACT, NIN, LOSS != LOSS_NONE>(W1s, W2s, W3s, b1s, b2s, b3s, xin, H1img, H2img, h2r, n, g);
    if constexpr (LOSS == LOSS_NONE) {
      if (valid) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * g + q < m.d_out) a.y[(s0 + n) * m.d_out + 4 * g + q] = y[q];
      }
    } else {
      // ---- loss and its gradient with respect to the network output (pds_mlp.hip mlp_kernel, same expressions) -------
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
      wide_backward<ACT, NIN, true>(W2s, W3s, Ximg, H1img, H2img, dYimg, dy, h2r, G, n, g);
    }
  }

  if constexpr (LOSS != LOSS_NONE) {
    // ---- this WAVE's partial sums -> partials[wave of the grid][...] (flat parameter layout + statistics) ----------
    float *out = a.partials + wid * a.pstride;
    const Offsets o = offsets(m);
    G.store(m, o, out, n, g);
    store_stats(out, o.total, {st_loss, st_ratio, st_kl, st_cnt}, lane);
  }
}

template <int LOSS, int ACT>
static void launch_nin(int nin, dim3 g, hipStream_t s, const Args &a) {
  const dim3 b(kWideWaves * 64);
  // input tiles in steps of two (d_in <= 96 / 128 / 160 / 192): an all-padding tile costs 4 x 4 MFMAs per layer-1 GEMM
  if (nin <= 6) hipLaunchKernelGGL((mlp_wide_kernel<LOSS, ACT, 6>), g, b, 0, s, a);
  else if (nin <= 8) hipLaunchKernelGGL((mlp_wide_kernel<LOSS, ACT, 8>), g, b, 0, s, a);
  else if (nin <= 10) hipLaunchKernelGGL((mlp_wide_kernel<LOSS, ACT, 10>), g, b, 0, s, a);
  else hipLaunchKernelGGL((mlp_wide_kernel<LOSS, ACT, 12>), g, b, 0, s, a);
}

// -> number of partials written (one per wave of the grid)
int launch_wide(int loss, const Args &a, hipStream_t s) {
  const int nin = (a.m.d_in + kTW - 1) / kTW;
  const int blocks = wide_grid_blocks(a.B);
  const dim3 g(blocks);
  if (loss == LOSS_NONE) { if (a.m.activation == 0) launch_nin<LOSS_NONE, 0>(nin, g, s, a); else launch_nin<LOSS_NONE, 1>(nin, g, s, a); }
  else if (loss == LOSS_PPO) { if (a.m.activation == 0) launch_nin<LOSS_PPO, 0>(nin, g, s, a); else launch_nin<LOSS_PPO, 1>(nin, g, s, a); }
  else { if (a.m.activation == 0) launch_nin<LOSS_MSE, 0>(nin, g, s, a); else launch_nin<LOSS_MSE, 1>(nin, g, s, a); }
  return blocks * kWideWaves;
}

}  // namespace pds_mlp_detail
