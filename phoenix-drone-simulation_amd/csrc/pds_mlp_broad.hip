// pds_mlp_broad.hip -- the trainer's dense kernels for two-hidden-layer networks with a hidden width ABOVE 64, up to 512
// (include/pds_mlp_broad.h): forward, value-regression gradient, Adam step.  Who needs it: the reference's default for DDPG and SAC
// is hidden_sizes (400, 300) (algs/ddpg/defaults.py, algs/sac/defaults.py); csrc/pds_ddpg_broad.hip builds DDPG's update on this.
//
// The design of csrc/pds_mlp.hip does not stretch: it keeps a block's weights in LDS and a wave's whole dW in accumulators, and
// W2 alone is 400 x 300 floats = 480 KB against 160 KB of LDS, dW2 120 000 accumulators.  Here:
//   * the weights stay in global memory.  Both networks of a DDPG update are 1.1 MB, far inside one XCD's 4 MB L2: every block
//     reads its A operands straight from there (broad_gemm), and nothing is staged.
//   * CHAIN kernel (broad_chain_kernel): a block of 8 waves owns 16 samples (32 from B = 512 on, so a weight load serves two
//     MFMAs) and walks the whole network with them -- X, H1, H2 and the output as [sample][feature] images in LDS (71.7 KB for 16
//     samples), the waves sharing the 16-wide output tiles of each layer, a __syncthreads() between layers.  Backward, the same
//     block turns the output gradient into dZ2 and dZ1 IN PLACE over H2 and H1 (dZ = (W^T dOut) * act'(H), A = the weight read
//     transposed).  One launch for the whole chain, which is what counts at the trainer's mini-batch of 128: 8 blocks, launch-bound.
//     For the gradient it writes X, H1, H2, dZ1, dZ2, dY of every sample to the workspace.
//   * WEIGHT-GRADIENT kernel (broad_wgrad_kernel), stationary in the output: a wave owns a 16 x 64 strip of one weight matrix
//     (column K of a strip row is the bias: its B operand is 1) and sums dZ^T In over the samples, four per MFMA, in sample order.
//     Above 512 samples they are split into up to 16 parts of equal size (grid.y); every part writes its own partial.
//   * REDUCE kernel: sums the parts in part order, scales by 1 / B, writes the gradient and may take the Adam step (adam_apply,
//     the arithmetic of pds_adam_step); one more block sums the chain blocks' statistics in a fixed order.
// No atomics anywhere: the same inputs give the same bits.  Three launches for a gradient call, one for a forward.
// Every GEMM is v_mfma_f32_16x16x4_f32; hidden tanh is tanhf.  Registers, LDS, spills: profiles/ddpg_broad_kernel_resources.txt.
#include "pds_mlp_broad_tile.h"

namespace pds_mlp_detail {

struct BroadArgs {
  pds_mlp m;
  const float *x;            // [rows, d_in]
  const int64_t *index;      // optional gather: sample g reads row index[g]
  long long B;
  const float *mean, *stdv;  // optional input standardisation (x - mean) / (std + eps)
  float eps;
  float *y;                  // forward output [B, d_out]
  const float *target;       // MSE: target[row]
  BroadWs ws;
};

template <int NS, int LOSS>
__global__ __launch_bounds__(kBroadThreads) void broad_chain_kernel(const BroadArgs a) {
  __shared__ __attribute__((aligned(16))) BroadLds<NS> L;
  constexpr bool kGrad = LOSS != LOSS_NONE;
  const pds_mlp &m = a.m;
  const int tid = threadIdx.x;
  const long long s0 = (long long)blockIdx.x * (NS * kTS);
  broad_load_x<NS>(a.x, m.d_in, m.d_in, a.index, s0, a.B, a.mean, a.stdv, a.eps, L.X, kGrad ? a.ws.x : nullptr);
  __syncthreads();
  broad_layer<NS>(m.w1, m.b1, m.h1, m.d_in, m.activation, L.X, kS, L.H1, kBS, kGrad ? a.ws.h1 : nullptr, s0, a.B);
  __syncthreads();
  broad_layer<NS>(m.w2, m.b2, m.h2, m.h1, m.activation, L.H1, kBS, L.H2, kBS, kGrad ? a.ws.h2 : nullptr, s0, a.B);
  __syncthreads();
  broad_layer<NS>(m.w3, m.b3, m.d_out, m.h2, -1, L.H2, kBS, L.Y, kSY, nullptr, s0, a.B);
  __syncthreads();
  if constexpr (!kGrad) {
    for (int e = tid; e < NS * kTS * kMaxOut; e += kBroadThreads) {
      const int sl = e / kMaxOut, c = e % kMaxOut;
      if (s0 + sl < a.B && c < m.d_out) a.y[(s0 + sl) * m.d_out + c] = L.Y[sl * kSY + c];
    }
  } else {
    // compute_loss_v: mse_loss(v(obs), target) (algs/iwpg/iwpg.py:272-275); dY of the loss SUM, the reduce scales by 1 / B
    if (tid < NS * kTS) {
      const long long s = s0 + tid;
      float dy = 0.f, se = 0.f, cnt = 0.f;
      if (s < a.B) {
        const long long row = a.index != nullptr ? a.index[s] : s;
        const float d = L.Y[tid * kSY] - a.target[row];
        se = d * d; cnt = 1.f; dy = 2.f * d;
        a.ws.dy[s] = dy;
      }
      L.Y[tid * kSY] = dy;
      L.red[tid][0] = se; L.red[tid][1] = cnt;
    }
    __syncthreads();
    broad_block_stats<NS>(L, a.ws.stat);
    broad_back<NS>(m.w3, m.h2, m.h2, m.d_out, m.activation, L.Y, kSY, L.H2, nullptr, a.ws.dz2, s0, a.B);
    __syncthreads();
    broad_back<NS>(m.w2, m.h1, m.h1, m.h2, m.activation, L.H2, kBS, L.H1, nullptr, a.ws.dz1, s0, a.B);
  }
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------
struct BroadWgLayer {
  const float *dz, *in;  // [B][M], [B][K]
  int M, K, woff, boff;  // W [M][K] at woff, b [M] at boff of the flat layout
  int strips, items;     // 64-wide strips of a row of [W | b], 16 x 64 work items
};
struct BroadWgArgs {
  BroadWgLayer l[3];
  long long B;
  int chunk;      // samples per part (a multiple of 4)
  int items;      // of the three layers
  float *parts;   // [gridDim.y][pstride]
  int pstride;
};

__global__ __launch_bounds__(kBroadWgWaves * 64) void broad_wgrad_kernel(const BroadWgArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
  int item = blockIdx.x * kBroadWgWaves + wave;  // wave-uniform
  if (item >= a.items) return;
  BroadWgLayer L = a.l[0];
  if (item >= L.items) {
    item -= L.items; L = a.l[1];
    if (item >= L.items) { item -= L.items; L = a.l[2]; }
  }
  const int o0 = (item / L.strips) * kTW, i0 = (item % L.strips) * 64;
  const long long c0 = (long long)blockIdx.y * a.chunk;
  const long long c1 = c0 + a.chunk < a.B ? c0 + a.chunk : a.B;
  const bool orow = o0 + n < L.M;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4)(0.f);
#pragma unroll 4
  for (long long s = c0; s < c1; s += 4) {  // k-slot g of the MFMA = sample s + g
    const long long sg = s + g;
    const bool ok = sg < c1;
    const float av = (ok && orow) ? L.dz[sg * L.M + o0 + n] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + kTW * j + n;
      const float bv = !ok ? 0.f : (i < L.K ? L.in[sg * L.K + i] : (i == L.K ? 1.f : 0.f));
      acc[j] = PDS_MFMA(av, bv, acc[j]);
    }
  }
  float *out = a.parts + (long long)blockIdx.y * a.pstride;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + kTW * j + n;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = o0 + 4 * g + q;
      if (o < L.M) {
        if (i < L.K) out[L.woff + o * L.K + i] = acc[j][q];
        else if (i == L.K) out[L.boff + o] = acc[j][q];
      }
    }
  }
}

// grads[p] = scale * (part 0 + part 1 + ...), the Adam step that may ride on it; the LAST block: stats = the chain blocks'
// statistics, thread t summing blocks t, t + 256, ... and a fixed tree over the threads
__global__ __launch_bounds__(256) void broad_reduce_kernel(const float *parts, int pstride, int nparts, int total, float scale,
                                                           float *grads, pds_mlp m, AdamK ad, const float *stat, int nstat,
                                                           float *stats) {
  const int tid = threadIdx.x;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ float red[256][kStats];
#pragma unroll
    for (int c = 0; c < kStats; ++c) {
      float t = 0.f;
      for (int b = tid; b < nstat; b += 256) t += stat[(long long)b * kStats + c];
      red[tid][c] = t;
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w)
#pragma unroll
        for (int c = 0; c < kStats; ++c) red[tid][c] += red[tid + w][c];
      __syncthreads();
    }
    if (tid < kStats) stats[tid] = red[0][tid];
    return;
  }
  const int p = blockIdx.x * 256 + tid;
  if (p >= total) return;
  float t = 0.f;
  for (int k = 0; k < nparts; ++k) t += parts[(long long)k * pstride + p];
  const float gr = t * scale;
  grads[p] = gr;
  if (ad.em != nullptr) adam_apply(ad, p, gr, param_ptr(m, offsets(m), p));
}

// torch.optim.Adam on the flat gradient (adam_apply), one thread per parameter
__global__ __launch_bounds__(256) void broad_adam_kernel(pds_mlp m, const float *g, int total, AdamK ad) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  adam_apply(ad, p, g[p], param_ptr(m, offsets(m), p));
}

int broad_grad_finish(const pds_mlp &m, const BroadWs &ws, long long B, int blocks, float *d_grads, float *d_stats,
                      const pds_adam *opt, hipStream_t s) {
  const Offsets o = offsets(m);
  BroadWgArgs a{};
  const float *dz[3] = {ws.dz1, ws.dz2, ws.dy}, *in[3] = {ws.x, ws.h1, ws.h2};
  const int M[3] = {m.h1, m.h2, m.d_out}, K[3] = {m.d_in, m.h1, m.h2}, woff[3] = {o.w1, o.w2, o.w3}, boff[3] = {o.b1, o.b2, o.b3};
  for (int l = 0; l < 3; ++l) {
    BroadWgLayer &L = a.l[l];
    L.dz = dz[l]; L.in = in[l]; L.M = M[l]; L.K = K[l]; L.woff = woff[l]; L.boff = boff[l];
    L.strips = (K[l] + 1 + 63) / 64;
    L.items = ((M[l] + kTW - 1) / kTW) * L.strips;
    a.items += L.items;
  }
  long long splits = (B + kBroadSplitRows - 1) / kBroadSplitRows;
  if (splits > kBroadMaxSplits) splits = kBroadMaxSplits;
  long long chunk = (B + splits - 1) / splits;
  chunk = (chunk + 3) / 4 * 4;
  splits = (B + chunk - 1) / chunk;  // (no empty part)
  a.B = B; a.chunk = (int)chunk; a.parts = ws.parts; a.pstride = o.total;
  hipLaunchKernelGGL(broad_wgrad_kernel, dim3((a.items + kBroadWgWaves - 1) / kBroadWgWaves, (unsigned)splits),
                     dim3(kBroadWgWaves * 64), 0, s, a);
  hipLaunchKernelGGL(broad_reduce_kernel, dim3((o.total + 255) / 256 + 1), dim3(256), 0, s, ws.parts, a.pstride, (int)splits,
                     o.total, 1.0f / (float)B, d_grads, m, adam_k(opt), ws.stat, blocks, d_stats);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

template <int LOSS>
static int broad_launch_chain(const BroadArgs &a, hipStream_t s) {  // -> blocks of the grid
  const int ns = broad_tiles_per_block(a.B);
  const int blocks = (int)((a.B + ns * kTS - 1) / (ns * kTS));
  if (ns == 1) hipLaunchKernelGGL((broad_chain_kernel<1, LOSS>), dim3(blocks), dim3(kBroadThreads), 0, s, a);
  else hipLaunchKernelGGL((broad_chain_kernel<2, LOSS>), dim3(blocks), dim3(kBroadThreads), 0, s, a);
  return blocks;
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int pds_mlp_broad_supported(const pds_mlp *m) { return broad_check(m) == PDS_OK && m->d_in <= kMaxDim ? 1 : 0; }

extern "C" int pds_mlp_broad_param_count(const pds_mlp *m) {
  if (broad_check(m) != PDS_OK) return PDS_EINVAL;
  return offsets(*m).total;
}

extern "C" int64_t pds_mlp_broad_workspace_floats(const pds_mlp *m) {
  if (broad_check(m) != PDS_OK) return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  return broad_ws_floats(*m, kBroadMaxBatch);
}

extern "C" int pds_mlp_broad_forward(const pds_mlp *m, const float *d_x, const int64_t *d_index, int64_t B, const float *d_mean,
                                     const float *d_std, float eps, float *d_y, void *stream) {
  if (broad_check(m) != PDS_OK || !d_x || !d_y || B < 1 || ((d_mean == nullptr) != (d_std == nullptr))) return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  BroadArgs a{};
  a.m = *m; a.x = d_x; a.index = d_index; a.B = B; a.mean = d_mean; a.stdv = d_std; a.eps = eps; a.y = d_y;
  broad_launch_chain<LOSS_NONE>(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_mlp_broad_value_grad_step(const pds_mlp *m, const float *d_x, const int64_t *d_index, const float *d_target,
                                             int64_t B, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                                             void *stream) {
  if (broad_check(m) != PDS_OK || m->d_out != 1 || !d_x || !d_target || !d_grads || !d_stats || !d_workspace || B < 1 ||
      !adam_ok(opt))
    return PDS_EINVAL;
  if (m->d_in > kMaxDim || B > kBroadMaxBatch) return PDS_EUNSUPPORTED;
  BroadArgs a{};
  a.m = *m; a.x = d_x; a.index = d_index; a.B = B; a.target = d_target;
  a.ws = broad_ws(d_workspace, *m, B);
  const int blocks = broad_launch_chain<LOSS_MSE>(a, (hipStream_t)stream);
  return broad_grad_finish(*m, a.ws, B, blocks, d_grads, d_stats, opt, (hipStream_t)stream);
}

extern "C" int pds_mlp_broad_adam_step(const pds_mlp *m, const float *d_grads, float *d_exp_avg, float *d_exp_avg_sq, int64_t step,
                                       float lr, float beta1, float beta2, float eps, void *stream) {
  const pds_adam opt{d_exp_avg, d_exp_avg_sq, step, lr, beta1, beta2, eps};
  if (broad_check(m) != PDS_OK || !d_grads || !adam_ok(&opt)) return PDS_EINVAL;
  const int total = offsets(*m).total;
  hipLaunchKernelGGL(broad_adam_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, d_grads, total,
                     adam_k(&opt));
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
