// pds_mlp_tile.h -- the 16-sample-tile core of the K-tiled kernels (csrc/pds_mlp_wide.hip: mlp_wide_kernel; csrc/pds_npg.hip:
// fvp_kernel, surrogate_kernel), each piece written once: grid size, weight staging, the LDS GEMM, the wave's weight-gradient
// accumulators with their write-out, the backward chain from the output gradient, the statistics behind a wave's partial, and
// the fixed-order sum of the waves' partials (the last two also in csrc/pds_mlp.hip).
//
// The design is mlp_kernel's of csrc/pds_mlp.hip (read that first): a wave owns a 16-sample tile, every GEMM of forward and
// backward runs on v_mfma_f32_16x16x4_f32 with the transposed chain (activations stay in registers from layer to layer),
// the weight gradients accumulate in registers over the wave's tiles, a second kernel sums the partials in a fixed order.
// What changes with the width of the first layer (up to twelve 16-wide input tiles):
//   * the accumulators of dW1 are 4 x NIN tiles = up to 192 registers (mlp_kernel: 48), next to 64 of dW2, 16 of dW3 and 36
//     of the bias gradients: ONE wave per SIMD (4 per block, up to 512 registers each) instead of two -- the matrix pipe and the
//     vector ALU no longer overlap between waves;
//   * W1's LDS image and the wave's X image have a row stride of 16 NIN + 4 floats (an odd multiple of 16 B, and 4 x stride ==
//     16 mod 32: the same two bank rules as the 68-float stride of the narrow kernels); 162.1 of 160 x 1024 = 163.8 KB of LDS
//     at NIN = 12 with four waves -- which is why there is no block-level reduction here (its staging area would not fit):
//     every WAVE writes its partial, and the reduce kernel sums 4 x more of them;
//   * bias gradients are always per-lane partial sums (the ones-column trick of the narrow kernels needs a padding column).
// Everything here is inlined into its kernel: moving a statement between this file and a kernel must not reorder the MFMAs of
// any accumulator, or the kernels' results change in the last bit.
#pragma once
#include "pds_mlp_common.h"

namespace pds_mlp_detail {

template <int NIN>
constexpr int wide_stride() { return kTW * NIN + 4; }

// blocks of `waves` waves, one 16-sample tile per wave and round
inline int wide_grid_blocks(long long B, int waves = kWideWaves) {
  const long long tiles = (B + kTS - 1) / kTS;
  const long long blocks = (tiles + waves - 1) / waves;
  return (int)(blocks < kWideMaxBlocks ? blocks : kWideMaxBlocks);  // one persistent block per CU
}

// weight images [out][in] of the network, zero padded, by the THREADS threads of a block; val(t, i) is what is staged
// for the parameter of value t at position i of the flat layout (the identity, or a line-search candidate).
// W3: the 8 rows d_out <= kMaxOut can fill (the narrow kernels keep 16): rows 8..15 of the 16-row MFMA tile ALIAS rows 0..7
// (`& 7` / `n & (kMaxOut - 1)` at the reads) -- outputs 8..15 are never read, and their gradient dY is zero, so the aliased
// rows only ever meet zeros
template <int S1, int THREADS = kWideWaves * 64, class F>
__device__ __forceinline__ void stage_wide(const pds_mlp &m, float *W1s, float *W2s, float *W3s, float *b1s, float *b2s,
                                           float *b3s, int tid, F val) {
  const Offsets o = offsets(m);
  constexpr int kThreads = THREADS;
  for (int i = tid; i < kMaxDim * S1; i += kThreads) {
    const int r = i / S1, k = i - r * S1;
    W1s[i] = (r < m.h1 && k < m.d_in) ? val(m.w1[r * m.d_in + k], o.w1 + r * m.d_in + k) : 0.f;
  }
  for (int i = tid; i < kMaxDim * kS; i += kThreads) {
    const int r = i / kS, k = i - r * kS;
    W2s[i] = (r < m.h2 && k < m.h1) ? val(m.w2[r * m.h1 + k], o.w2 + r * m.h1 + k) : 0.f;
    if (i < kMaxOut * kS) W3s[i] = (r < m.d_out && k < m.h2) ? val(m.w3[r * m.h2 + k], o.w3 + r * m.h2 + k) : 0.f;
  }
  if (tid < kMaxDim) {
    b1s[tid] = tid < m.h1 ? val(m.b1[tid], o.b1 + tid) : 0.f;
    b2s[tid] = tid < m.h2 ? val(m.b2[tid], o.b2 + tid) : 0.f;
  }
  if (tid < kTW) b3s[tid] = tid < m.d_out ? val(m.b3[tid], o.b3 + tid) : 0.f;
}

// c + W[16 it .. +16][:] In^T for an LDS weight image with row stride S (pds_mlp.hip gemm_wt)
template <int NK, int S>
__device__ __forceinline__ f32x4 gemm_lds(const float *Ws, int it, const f32x4 (&in)[NK], int n, int g, f32x4 c) {
  const float *wp = Ws + (it * kTW + n) * S + 4 * g;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt) {
    const f32x4 a = lds4(wp + kt * kTW);
#pragma unroll
    for (int j = 0; j < 4; ++j) c = PDS_MFMA(a[j], in[kt][j], c);
  }
  return c;
}

// Z^T tiles `it`, `it + 1` = W[16 it .. +32][:] In^T, two output tiles per read of the B operands (pds_mlp.hip gemm_wt2)
template <int NK, int S>
__device__ __forceinline__ void gemm_wt2s(const float *Ws, int it, const f32x4 (&in)[NK], int n, int g, f32x4 &c0, f32x4 &c1) {
  c0 = (f32x4)(0.f);
  c1 = (f32x4)(0.f);
  const float *wp = Ws + (it * kTW + n) * S + 4 * g;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt) {
    const f32x4 a0 = lds4(wp + kt * kTW), a1 = lds4(wp + kTW * S + kt * kTW);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c0 = PDS_MFMA(a0[j], in[kt][j], c0);
      c1 = PDS_MFMA(a1[j], in[kt][j], c1);
    }
  }
}

// Forward pass of one tile from xin (lane (n, g): features 16 kt + 4 g + q of sample n = the B operands of layer 1) to
// Y^T = W3 H2^T + b3 (lane (n, g): outputs 4 g + q of sample n; rows >= d_out: 0); activations stay in registers from layer
// to layer.  h2r: this lane's H2 values; IMG: H1 and H2 also go to their [sample][feature] images (for wide_backward)
template <int ACT, int NIN, bool IMG>
__device__ __forceinline__ f32x4 wide_forward(const float *W1s, const float *W2s, const float *W3s, const float *b1s,
                                              const float *b2s, const float *b3s, const f32x4 (&xin)[NIN], float *H1img,
                                              float *H2img, f32x4 (&h2r)[kNT], int n, int g) {
  constexpr int S1 = wide_stride<NIN>();
  f32x4 h1r[kNT], cc[kNT];
#pragma unroll
  for (int it = 0; it < kNT; it += 2) gemm_wt2s<NIN, S1>(W1s, it, xin, n, g, cc[it], cc[it + 1]);
#pragma unroll
  for (int it = 0; it < kNT; ++it) {  // H1^T = act(W1 X^T + b1); rows >= h1: act(0) = 0
    const f32x4 b = lds4(b1s + it * kTW + 4 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) h1r[it][q] = act_fn<ACT>(cc[it][q] + b[q]);
    if (IMG) sts4(H1img + n * kS + it * kTW + 4 * g, h1r[it]);
  }
#pragma unroll
  for (int it = 0; it < kNT; it += 2) gemm_wt2s<kNT, kS>(W2s, it, h1r, n, g, cc[it], cc[it + 1]);
#pragma unroll
  for (int it = 0; it < kNT; ++it) {  // H2^T = act(W2 H1^T + b2)
    const f32x4 b = lds4(b2s + it * kTW + 4 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) h2r[it][q] = act_fn<ACT>(cc[it][q] + b[q]);
    if (IMG) sts4(H2img + n * kS + it * kTW + 4 * g, h2r[it]);
  }
  return gemm_lds<kNT, kS>(W3s, 0, h2r, n & (kMaxOut - 1), g, (f32x4)(0.f)) + lds4(b3s + 4 * g);
}

// the staged images of one network (stride kS throughout)
struct NetLds {
  const float *W1, *W2, *W3, *b1, *b2, *b3;
};

// wide_forward without images, H1 kept next to H2 (this lane's values: what act' of a backward chain without weight gradients
// reads): the Q networks of csrc/pds_actor_critic.h
template <int ACT, int NIN>
__device__ __forceinline__ f32x4 forward_regs(const NetLds &N, const f32x4 (&xin)[NIN], f32x4 (&h1r)[kNT],
                                              f32x4 (&h2r)[kNT], int n, int g) {
  f32x4 cc[kNT];
#pragma unroll
  for (int it = 0; it < kNT; it += 2) gemm_wt2s<NIN, kS>(N.W1, it, xin, n, g, cc[it], cc[it + 1]);
#pragma unroll
  for (int it = 0; it < kNT; ++it) {
    const f32x4 b = lds4(N.b1 + it * kTW + 4 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) h1r[it][q] = act_fn<ACT>(cc[it][q] + b[q]);
  }
#pragma unroll
  for (int it = 0; it < kNT; it += 2) gemm_wt2s<kNT, kS>(N.W2, it, h1r, n, g, cc[it], cc[it + 1]);
#pragma unroll
  for (int it = 0; it < kNT; ++it) {
    const f32x4 b = lds4(N.b2 + it * kTW + 4 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) h2r[it][q] = act_fn<ACT>(cc[it][q] + b[q]);
  }
  return gemm_lds<kNT, kS>(N.W3, 0, h2r, n & (kMaxOut - 1), g, (f32x4)(0.f)) + lds4(N.b3 + 4 * g);
}

// C[it][jt] += A_it^T B_jt over the 16 samples of a tile, operands as three bf16 pieces of the four values (samples 4 h .. 4 h + 3
// of one feature) a lane holds per 16 x 16 block: slot (h, i < 4) = sample 4 h + i with pieces (a, b), slot (h, i >= 4) = the
// same sample with (a', b') -- (lo | mid)(hi | mid), (mid | hi)(hi | lo), (hi | hi)(hi | mid) are the six products.
template <int NA, int NB, class Acc>
__device__ __forceinline__ void outer_bf16(const Quad3 (&qa)[NA], const Quad3 (&qb)[NB], Acc &&acc) {
#pragma unroll
  for (int it = 0; it < NA; ++it)
#pragma unroll
    for (int jt = 0; jt < NB; ++jt) acc(it, jt) = PDS_MFMA_BF(cat8(qa[it].lo, qa[it].mid), cat8(qb[jt].hi, qb[jt].mid), acc(it, jt));
#pragma unroll
  for (int it = 0; it < NA; ++it)
#pragma unroll
    for (int jt = 0; jt < NB; ++jt) acc(it, jt) = PDS_MFMA_BF(cat8(qa[it].mid, qa[it].hi), cat8(qb[jt].hi, qb[jt].lo), acc(it, jt));
#pragma unroll
  for (int it = 0; it < NA; ++it)
#pragma unroll
    for (int jt = 0; jt < NB; ++jt) acc(it, jt) = PDS_MFMA_BF(cat8(qa[it].hi, qa[it].hi), cat8(qb[jt].hi, qb[jt].mid), acc(it, jt));
}

// weight-gradient accumulators of a wave (over all of its tiles), C/D layout: lane (n, g) holds column n and rows 4 g + q of
// every 16 x 16 tile; bias gradients as per-lane partial sums.  NG1: input tiles of dW1
template <int NG1>
struct WideGrads {
  f32x4 W1[kNT][NG1], W2[kNT][kNT], W3[kNT], b1[kNT], b2[kNT], b3;

  __device__ __forceinline__ void zero() {
    b3 = (f32x4)(0.f);
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
      W3[i] = (f32x4)(0.f); b1[i] = (f32x4)(0.f); b2[i] = (f32x4)(0.f);
#pragma unroll
      for (int j = 0; j < kNT; ++j) W2[i][j] = (f32x4)(0.f);
#pragma unroll
      for (int j = 0; j < NG1; ++j) W1[i][j] = (f32x4)(0.f);
    }
  }

  // -> out[flat parameter layout]: this WAVE's partial sums
  __device__ __forceinline__ void store(const pds_mlp &m, const Offsets &o, float *out, int n, int g) const {
#pragma unroll
    for (int it = 0; it < kNT; ++it) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = it * kTW + 4 * g + q;  // row of the C/D layout
#pragma unroll
        for (int jt = 0; jt < NG1; ++jt) {
          const int j = jt * kTW + n;
          if (i < m.h1 && j < m.d_in) out[o.w1 + i * m.d_in + j] = W1[it][jt][q];
        }
#pragma unroll
        for (int jt = 0; jt < kNT; ++jt) {
          const int j = jt * kTW + n;
          if (i < m.h2 && j < m.h1) out[o.w2 + i * m.h1 + j] = W2[it][jt][q];
        }
        float v1 = b1[it][q], v2 = b2[it][q];  // sum of the per-lane partials over the 16 sample columns of the lane group
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) { v1 += __shfl_xor(v1, d); v2 += __shfl_xor(v2, d); }
        if (n == 0) {
          if (i < m.h1) out[o.b1 + i] = v1;
          if (i < m.h2) out[o.b2 + i] = v2;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * g + q;
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) {
        const int j = jt * kTW + n;
        if (i < m.d_out && j < m.h2) out[o.w3 + i * m.h2 + j] = W3[jt][q];
      }
      float v3 = b3[q];
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) v3 += __shfl_xor(v3, d);
      if (n == 0 && i < m.d_out) out[o.b3 + i] = v3;
    }
  }
};

// Backward pass of one tile from the output gradient dy (lane (n, g): outputs 4 g + q of sample n, zero outside the batch and
// the outputs) to the wave's accumulators: dW3 = dY^T H2, dZ2 = (W3^T dY) act'(H2), dW2 = dZ2^T H1, dZ1 = (W2^T dZ2) act'(H1),
// dW1 = dZ1^T X, the bias gradients on the way.  Ximg / H1img / H2img hold the tile's [sample][feature] images of the forward
// pass (H1img and H2img are overwritten with dZ1 and dZ2), h2r this lane's H2 values, dYimg receives dy.
// BF16: dW2 and dW1 (K = the tile's 16 samples) on split-bf16 MFMAs (pds_mlp_common.h), two input tiles at a time; else every
// GEMM on v_mfma_f32_16x16x4_f32.
template <int ACT, int NIN, bool BF16>
__device__ __forceinline__ void wide_backward(const float *W2s, const float *W3s, const float *Ximg, float *H1img, float *H2img,
                                              float *dYimg, const f32x4 dy, const f32x4 (&h2r)[kNT], WideGrads<NIN> &G, int n,
                                              int g) {
  constexpr int S1 = wide_stride<NIN>();
  G.b3 += dy;
  sts4(dYimg + n * kSY + 4 * g, dy);
  PDS_WAVE_SYNC();

  // Weight-gradient GEMMs take K = the tile's 16 samples: k-slot (j, h) carries sample 4 h + j, both operands are dword reads
  // of [sample][feature] images (conflict free).
  const int r = n, h = g;  // A-operand lane roles
  f32x4 cc[kNT];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // dW3 += dY^T H2 (rows = outputs)
    const float av = dYimg[(4 * h + j) * kSY + r];
#pragma unroll
    for (int jt = 0; jt < kNT; ++jt) G.W3[jt] = PDS_MFMA(av, H2img[(4 * h + j) * kS + jt * kTW + n], G.W3[jt]);
  }
  // dZ2^T = (W3^T dY^T) * act'(H2^T); the k-slot (j, h) carries output 4 h + j = register j of dy
  f32x4 dz2[kNT];
#pragma unroll
  for (int it = 0; it < kNT; ++it) cc[it] = (f32x4)(0.f);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int it = 0; it < kNT; ++it) cc[it] = PDS_MFMA(W3s[((4 * h + j) & (kMaxOut - 1)) * kS + it * kTW + r], dy[j], cc[it]);
#pragma unroll
  for (int it = 0; it < kNT; ++it) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dz2[it][q] = cc[it][q] * act_grad<ACT>(h2r[it][q]);
    G.b2[it] += dz2[it];
  }
#pragma unroll
  for (int it = 0; it < kNT; ++it) sts4(H2img + n * kS + it * kTW + 4 * g, dz2[it]);  // after the dW3 reads (in order)
  PDS_WAVE_SYNC();
  if constexpr (BF16) {  // dW2 += dZ2^T H1
    Quad3 qa[kNT], qb[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
      f32x4 va, vb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        va[j] = H2img[(4 * h + j) * kS + i * kTW + r];
        vb[j] = H1img[(4 * h + j) * kS + i * kTW + n];
      }
      qa[i] = split4(va);
      qb[i] = split4(vb);
    }
    outer_bf16<kNT, kNT>(qa, qb, [&](int it, int jt) -> f32x4 & { return G.W2[it][jt]; });
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float av[kNT], bv[kNT];
#pragma unroll
      for (int i = 0; i < kNT; ++i) {
        av[i] = H2img[(4 * h + j) * kS + i * kTW + r];
        bv[i] = H1img[(4 * h + j) * kS + i * kTW + n];
      }
#pragma unroll
      for (int it = 0; it < kNT; ++it)
#pragma unroll
        for (int jt = 0; jt < kNT; ++jt) G.W2[it][jt] = PDS_MFMA(av[it], bv[jt], G.W2[it][jt]);
    }
  }
  // dZ1^T = (W2^T dZ2^T) * act'(H1^T): A = W2^T read column-wise (4 dwords per k-tile)
  f32x4 dz1[kNT];
#pragma unroll
  for (int jt = 0; jt < kNT; ++jt) cc[jt] = (f32x4)(0.f);
#pragma unroll
  for (int kt = 0; kt < kNT; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) cc[jt] = PDS_MFMA(W2s[(kt * kTW + 4 * h + j) * kS + jt * kTW + r], dz2[kt][j], cc[jt]);
#pragma unroll
  for (int jt = 0; jt < kNT; ++jt) {
    const f32x4 hv = lds4(H1img + n * kS + jt * kTW + 4 * g);  // this lane's own H1 values
#pragma unroll
    for (int q = 0; q < 4; ++q) dz1[jt][q] = cc[jt][q] * act_grad<ACT>(hv[q]);
    G.b1[jt] += dz1[jt];
  }
#pragma unroll
  for (int jt = 0; jt < kNT; ++jt) sts4(H1img + n * kS + jt * kTW + 4 * g, dz1[jt]);  // after the dW2 reads
  PDS_WAVE_SYNC();
  if constexpr (BF16) {  // dW1 += dZ1^T X
    Quad3 qa[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
      f32x4 va;
#pragma unroll
      for (int j = 0; j < 4; ++j) va[j] = H1img[(4 * h + j) * kS + i * kTW + r];
      qa[i] = split4(va);
    }
    // two input tiles at a time: the pieces of all NIN of them (6 registers each) next to 16 NIN accumulators do not fit 512
    static_assert(NIN % 2 == 0, "input tiles come in pairs");
#pragma unroll
    for (int k0 = 0; k0 < NIN; k0 += 2) {
      Quad3 qb2[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        f32x4 vb;
#pragma unroll
        for (int j = 0; j < 4; ++j) vb[j] = Ximg[(4 * h + j) * S1 + (k0 + kk) * kTW + n];
        qb2[kk] = split4(vb);
      }
      outer_bf16<kNT, 2>(qa, qb2, [&](int it, int kk) -> f32x4 & { return G.W1[it][k0 + kk]; });
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float av[kNT];
#pragma unroll
      for (int i = 0; i < kNT; ++i) av[i] = H1img[(4 * h + j) * kS + i * kTW + r];
#pragma unroll
      for (int kt = 0; kt < NIN; ++kt) {
        const float bv = Ximg[(4 * h + j) * S1 + kt * kTW + n];
#pragma unroll
        for (int it = 0; it < kNT; ++it) G.W1[it][kt] = PDS_MFMA(av[it], bv, G.W1[it][kt]);
      }
    }
  }
  PDS_WAVE_SYNC();  // the images are rewritten by the next tile
}

// The kStats statistics behind a wave's partial (out[total ..]): the lanes of group 0 hold per-sample sums, lane 0 writes their
// sum over the 16 samples
__device__ __forceinline__ void store_stats(float *out, int total, const float (&s4)[kStats], int lane) {
#pragma unroll
  for (int q = 0; q < kStats; ++q) {
    float v = s4[q];
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) out[total + q] = v;
  }
}

// Sum of element p over the waves' partials in a fixed order (deterministic, no atomics), by a block of 64 elements x 16
// slices of the wave range (16 x fewer dependent loads per thread): four chains per slice, then the slices in order.
// Every thread of the 1024 calls it (`active`: p is inside the partial); the sum is returned to the threads of slice 0.
__device__ __forceinline__ float sum_partials(const float *partials, int pstride, int nwaves, int p, bool active) {
  __shared__ float part[16][64];
  const int px = threadIdx.x & 63, sl = threadIdx.x >> 6;
  float s = 0.f;
  if (active) {
    const int per = (nwaves + 15) / 16, w0 = sl * per, w1 = min(nwaves, w0 + per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int w = w0;
    for (; w + 3 < w1; w += 4) {
      s0 += partials[(long long)w * pstride + p];
      s1 += partials[(long long)(w + 1) * pstride + p];
      s2 += partials[(long long)(w + 2) * pstride + p];
      s3 += partials[(long long)(w + 3) * pstride + p];
    }
    for (; w < w1; ++w) s0 += partials[(long long)w * pstride + p];
    s = (s0 + s1) + (s2 + s3);
  }
  part[sl][px] = s;
  __syncthreads();
  float t = 0.f;
  if (sl == 0 && active) {
#pragma unroll
    for (int q = 0; q < 16; ++q) t += part[q][px];
  }
  return t;
}

}  // namespace pds_mlp_detail
