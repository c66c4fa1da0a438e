// pds_mlp_broad_tile.h -- what the two translation units for two-hidden-layer networks with a hidden width ABOVE 64 share
// (csrc/pds_mlp_broad.hip: forward, value gradient, Adam; csrc/pds_ddpg_broad.hip: DDPG's policy gradient and Bellman backup),
// each piece written once: the range check, the workspace layout, the tile GEMM against weights in global memory, the forward
// layer and the backward layer of a chain kernel.  The design is stated in the header of csrc/pds_mlp_broad.hip (read that first).
#pragma once
#include "pds_mlp_common.h"

#include "../../include/pds_mlp_broad.h"

namespace pds_api_detail {
void set_thread_error(const char *msg);  // csrc/pds_api.hip: the text pds_last_error(NULL) returns on this thread
}

namespace pds_mlp_detail {

constexpr int kBroadMax = PDS_MLP_BROAD_MAX_HIDDEN;          // h1, h2 <= 512
constexpr long long kBroadMaxBatch = PDS_MLP_BROAD_MAX_BATCH;  // samples of a gradient call
constexpr int kBS = kBroadMax + 4;    // row stride of a hidden image: 16-B aligned rows, 4 * kBS == 16 (mod 32) as kS
constexpr int kBroadWaves = 8;        // waves of a chain block: they share the output tiles of a layer
constexpr int kBroadThreads = kBroadWaves * 64;
constexpr int kBroadPairFrom = 512;   // from this batch size a chain block takes TWO 16-sample tiles (a weight load serves both)
constexpr int kBroadSplitRows = 512;  // samples per part of a weight-gradient sum ...
constexpr int kBroadMaxSplits = 16;   // ... up to this many parts, then the parts grow
constexpr int kBroadWgWaves = 4;      // waves of a weight-gradient block, one 16 x 64 strip of a weight matrix each

// the [sample][feature] images of a chain block in LDS, NS 16-sample tiles: 71 680 B at NS = 1 (two blocks per CU), 143 360 B at 2
template <int NS>
struct BroadLds {
  float X[NS * kTS * kS];    // the standardised input rows (DDPG: [obs | action]); columns past d_in are zero
  float H1[NS * kTS * kBS];  // forward: act(Z1); backward: dZ1 in place
  float H2[NS * kTS * kBS];
  float Y[NS * kTS * kSY];   // the output layer, then its gradient; columns past d_out are zero
  float red[NS * kTS][2];    // per sample: its loss term (sum Q), 1 if it counts
};

// PDS_OK for a network inside the range of include/pds_mlp_broad.h (d_in up to kMaxDimIn: 65 .. 192 is a valid network that the
// kernels do not cover), else PDS_EINVAL
static int broad_check(const pds_mlp *m) {
  if (!m || !m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->w3 || !m->b3) return PDS_EINVAL;
  if (m->d_in < 1 || m->d_in > kMaxDimIn || m->d_out < 1 || m->d_out > kMaxOut || (m->activation != 0 && m->activation != 1) ||
      m->h1 < 1 || m->h2 < 1 || m->h1 > kBroadMax || m->h2 > kBroadMax)
    return PDS_EINVAL;
  if (m->h1 <= kMaxDim && m->h2 <= kMaxDim) {
    pds_api_detail::set_thread_error(
        "pds_mlp_broad: h1, h2 <= 64 is the network of include/pds.h (pds_mlp_forward, pds_value_grad_step, pds_adam_step, "
        "pds_ddpg_policy_grad, pds_ddpg_target, pds_polyak); the broad entry points take a hidden width above 64");
    return PDS_EINVAL;
  }
  return PDS_OK;
}

// ---- the workspace of a gradient call on network m over B samples -------------------------------------------------------------
struct BroadWs {
  float *x, *h1, *h2;      // [B][d_in], [B][h1], [B][h2]: the inputs of the three weight-gradient GEMMs
  float *dz1, *dz2, *dy;   // [B][h1], [B][h2], [B][d_out]: the gradients of the loss SUM with respect to the pre-activations
  float *stat;             // [chain blocks][kStats]
  float *parts;            // [splits][param_count]
};
inline int64_t broad_ws_floats(const pds_mlp &m, long long B) {
  return B * (m.d_in + 2 * (m.h1 + m.h2) + m.d_out) + kStats * ((B + kTS - 1) / kTS) + (int64_t)kBroadMaxSplits * offsets(m).total;
}
inline BroadWs broad_ws(float *p, const pds_mlp &m, long long B) {
  BroadWs w;
  w.x = p; p += B * m.d_in;
  w.h1 = p; p += B * m.h1;
  w.h2 = p; p += B * m.h2;
  w.dz1 = p; p += B * m.h1;
  w.dz2 = p; p += B * m.h2;
  w.dy = p; p += B * m.d_out;
  w.stat = p; p += kStats * ((B + kTS - 1) / kTS);
  w.parts = p;
  return w;
}
inline int broad_tiles_per_block(long long B) { return B >= kBroadPairFrom ? 2 : 1; }

// csrc/pds_mlp_broad.hip: the weight-gradient kernel over the workspace of `m` (written by a chain kernel of `blocks` blocks), the
// fixed-order sum of its parts scaled by 1 / B into d_grads, the statistics into d_stats and the Adam step when opt != nullptr
int broad_grad_finish(const pds_mlp &m, const BroadWs &ws, long long B, int blocks, float *d_grads, float *d_stats,
                      const pds_adam *opt, hipStream_t s);

#ifdef __HIPCC__
__device__ __forceinline__ float broad_act(float v, int act) { return act == 0 ? fmaxf(v, 0.f) : tanhf(v); }
// derivative expressed through the activation's OUTPUT h
__device__ __forceinline__ float broad_act_grad(float h, int act) { return act == 0 ? (h > 0.f ? 1.f : 0.f) : 1.f - h * h; }

// acc[ns] += A B(ns) for the 16 outputs o0 .. o0 + 15 and the NS sample tiles of the block: A[o][k] = W[o * ldw + k] (TRANS:
// W[k * ldw + o]) for o < M and k < K, else 0, read from global memory (the weights stay in L2); B = the image rows
// img[(16 ns + n) * stride + k], whose columns up to the next multiple of 16 past K hold finite values.  Lane (n, g) loads the
// four k-slots 4 g + q of a 16-wide K step, as the LDS kernels do: v_mfma_f32_16x16x4_f32, exact f32.
template <int NS, bool TRANS>
__device__ __forceinline__ void broad_gemm(const float *__restrict__ W, int ldw, int M, int K, int o0, const float *img, int stride,
                                           f32x4 (&acc)[NS], int n, int g) {
  const int o = o0 + n;
  const bool orow = o < M;
  const float *Wo = TRANS ? W + o : W + (long long)o * ldw;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += kTW) {
    const int k = k0 + 4 * g;
    f32x4 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = (orow && k + q < K) ? (TRANS ? Wo[(long long)(k + q) * ldw] : Wo[k + q]) : 0.f;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      const f32x4 b = lds4(img + (ns * kTS + n) * stride + k);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[ns] = PDS_MFMA(a[q], b[q], acc[ns]);
    }
  }
}

// the rows of a chain block: x[row(s)][0 .. d_in) for its samples s0 .. s0 + 16 NS - 1 (row = index[s] or s), standardised when
// mean != nullptr -> the X image (zero for s >= B and for the columns past d_in) and, for the weight gradient, gx[s][.]
template <int NS>
__device__ __forceinline__ void broad_load_x(const float *x, int ldx, int d_in, const int64_t *index, long long s0, long long B,
                                             const float *mean, const float *stdv, float eps, float *Ximg, float *gx) {
  for (int e = threadIdx.x; e < NS * kTS * kMaxDim; e += kBroadThreads) {
    const int sl = e / kMaxDim, c = e % kMaxDim;
    const long long s = s0 + sl;
    float v = 0.f;
    if (s < B && c < d_in) {
      const long long row = index != nullptr ? index[s] : s;
      v = x[row * ldx + c];
      if (mean != nullptr) {
        const float is = 1.0f / (stdv[c] + eps);
        v = (v - mean[c]) * is;
      }
      if (gx != nullptr) gx[s * d_in + c] = v;
    }
    Ximg[sl * kS + c] = v;
  }
}

// out = act(W in + b) for the block's samples: the waves share the 16-wide output tiles.  act < 0: no activation (the output
// layer).  gout != nullptr: also gout[s][0 .. M) for s < B.  The caller puts a __syncthreads() behind it.
template <int NS>
__device__ __forceinline__ void broad_layer(const float *W, const float *b, int M, int K, int act, const float *in, int in_stride,
                                            float *out, int out_stride, float *gout, long long s0, long long B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
  for (int o0 = wave * kTW; o0 < M; o0 += kBroadWaves * kTW) {
    f32x4 bias, acc[NS];
#pragma unroll
    for (int q = 0; q < 4; ++q) bias[q] = o0 + 4 * g + q < M ? b[o0 + 4 * g + q] : 0.f;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) acc[ns] = bias;
    broad_gemm<NS, false>(W, K, M, K, o0, in, in_stride, acc, n, g);
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      f32x4 h;
#pragma unroll
      for (int q = 0; q < 4; ++q) h[q] = act < 0 ? acc[ns][q] : broad_act(acc[ns][q], act);
      sts4(out + (ns * kTS + n) * out_stride + o0 + 4 * g, h);
      const long long s = s0 + ns * kTS + n;
      if (gout != nullptr && s < B) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (o0 + 4 * g + q < M) gout[s * M + o0 + 4 * g + q] = h[q];
      }
    }
  }
}

// dZ = (W^T dOut) * act'(H) through the layer BEHIND the activation: W [K][ldw] is that layer's weight, M the width of H (= the
// outputs here), K the width of dOut (image dimg).  H is read from its image himg [.][kBS] -- or, hglob !=
// nullptr, from global memory hglob[s][0 .. M) where the chain wrote it (an image that another network has overwritten since) --
// and dZ is written over it; gout != nullptr: also gout[s][0 .. M) for s < B.  The caller puts a __syncthreads() behind it.
template <int NS>
__device__ __forceinline__ void broad_back(const float *W, int ldw, int M, int K, int act, const float *dimg, int dstride,
                                           float *himg, const float *hglob, float *gout, long long s0, long long B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
  for (int o0 = wave * kTW; o0 < M; o0 += kBroadWaves * kTW) {
    f32x4 acc[NS];
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) acc[ns] = (f32x4)(0.f);
    broad_gemm<NS, true>(W, ldw, M, K, o0, dimg, dstride, acc, n, g);
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      float *p = himg + (ns * kTS + n) * kBS + o0 + 4 * g;
      const long long s = s0 + ns * kTS + n;
      f32x4 h = (f32x4)(0.f);
      if (hglob == nullptr) {
        h = lds4(p);
      } else if (s < B) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (o0 + 4 * g + q < M) h[q] = hglob[s * M + o0 + 4 * g + q];
      }
      f32x4 dz;
#pragma unroll
      for (int q = 0; q < 4; ++q) dz[q] = acc[ns][q] * broad_act_grad(h[q], act);
      sts4(p, dz);
      if (gout != nullptr && s < B) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (o0 + 4 * g + q < M) gout[s * M + o0 + 4 * g + q] = dz[q];
      }
    }
  }
}

// the block's statistics: the per-sample terms of L.red summed in sample order -> stat[block][kStats] = {sum, 0, 0, count}
template <int NS>
__device__ __forceinline__ void broad_block_stats(const BroadLds<NS> &L, float *stat) {
  if (threadIdx.x == 0) {
    float t = 0.f, c = 0.f;
    for (int i = 0; i < NS * kTS; ++i) { t += L.red[i][0]; c += L.red[i][1]; }
    float *o = stat + (long long)blockIdx.x * kStats;
    o[0] = t; o[1] = 0.f; o[2] = 0.f; o[3] = c;
  }
}
#endif  // __HIPCC__

}  // namespace pds_mlp_detail
