// pds_mlp_deep_tile.h -- what the two translation units for networks with THREE or FOUR hidden layers share (csrc/pds_mlp_deep.hip:
// mlp_deep_kernel; csrc/pds_npg_deep.hip: fvp_deep_kernel, surrogate_deep_kernel), each piece written once: the flat parameter
// layout, the weight staging with its transform, the forward chain of a tile, the wave's weight-gradient accumulators with their
// write-out, the backward chain from the output gradient, and the range check of struct pds_mlp_deep.
//
// The design is stated in the header of csrc/pds_mlp_deep.hip (read that first); the depth L is a template parameter throughout,
// so every layer loop has constant bounds and is unrolled.  Everything here is inlined into its kernel: moving a statement between
// this file and a kernel must not reorder the MFMAs of any accumulator, or the kernels' results change in the last bit.  The
// forward chain is ONE function for the same reason: the line-search candidate with step fraction 0 must give the bits of
// pds_mlp_deep_forward (its KL against that forward's output is exactly zero), which two statements of the chain would only
// promise as long as the compiler schedules both alike.
#pragma once
#include "pds_mlp_tile.h"

#include "../../include/pds_mlp_deep.h"

namespace pds_api_detail {
void set_thread_error(const char *msg);  // csrc/pds_api.hip: the text pds_last_error(NULL) returns on this thread
}

namespace pds_mlp_detail {

constexpr int kDeepLayers = PDS_MLP_DEEP_MAX_HIDDEN + 1;

// width of activation l: 0 the input, 1 .. n_hidden the hidden layers, n_hidden + 1 the output
__host__ __device__ __forceinline__ int deep_dim(const pds_mlp_deep &m, int l) {
  return l == 0 ? m.d_in : ((l <= m.n_hidden && l <= PDS_MLP_DEEP_MAX_HIDDEN) ? m.hidden[(l - 1) & 3] : m.d_out);
}

// flat parameter layout == torch's nn.Sequential order: W1 [h1][d_in], b1, ..., W(L+1) [d_out][hL], b(L+1)
struct DeepOffsets {
  int w[kDeepLayers], b[kDeepLayers], total;
};
__host__ __device__ __forceinline__ DeepOffsets deep_offsets(const pds_mlp_deep &m) {
  DeepOffsets o{};
  int p = 0;
#pragma unroll
  for (int l = 0; l < kDeepLayers; ++l) {
    if (l <= m.n_hidden) {
      o.w[l] = p; p += deep_dim(m, l + 1) * deep_dim(m, l);
      o.b[l] = p; p += deep_dim(m, l + 1);
    }
  }
  o.total = p;
  return o;
}
// parameter p of the flat layout, as a pointer
__device__ __forceinline__ float *deep_param_ptr(const pds_mlp_deep &m, int p) {
  const float *ptr = nullptr;
  int base = 0;
#pragma unroll
  for (int l = 0; l < kDeepLayers; ++l) {
    if (l <= m.n_hidden) {
      const int nw = deep_dim(m, l + 1) * deep_dim(m, l), nb = deep_dim(m, l + 1);
      if (p >= base && p < base + nw) ptr = m.w[l] + (p - base);
      base += nw;
      if (p >= base && p < base + nb) ptr = m.b[l] + (p - base);
      base += nb;
    }
  }
  return const_cast<float *>(ptr);
}

// weight-gradient accumulators of a wave (over all of its tiles), C/D layout as WideGrads (csrc/pds_mlp_tile.h)
template <int L>
struct DeepGrads {
  f32x4 W[L][kNT][kNT], Wo[kNT], b[L][kNT], bo;

  __device__ __forceinline__ void zero() {
    bo = (f32x4)(0.f);
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
      Wo[i] = (f32x4)(0.f);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        b[l][i] = (f32x4)(0.f);
#pragma unroll
        for (int j = 0; j < kNT; ++j) W[l][i][j] = (f32x4)(0.f);
      }
    }
  }

  // -> out[flat parameter layout]: this WAVE's partial sums
  __device__ __forceinline__ void store(const pds_mlp_deep &m, const DeepOffsets &o, float *out, int n, int g) const {
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const int rows = deep_dim(m, l + 1), cols = deep_dim(m, l);
#pragma unroll
      for (int it = 0; it < kNT; ++it) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = it * kTW + 4 * g + q;  // row of the C/D layout
#pragma unroll
          for (int jt = 0; jt < kNT; ++jt) {
            const int j = jt * kTW + n;
            if (i < rows && j < cols) out[o.w[l] + i * cols + j] = W[l][it][jt][q];
          }
          float v = b[l][it][q];  // sum of the per-lane partials over the 16 sample columns of the lane group
#pragma unroll
          for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d);
          if (n == 0 && i < rows) out[o.b[l] + i] = v;
        }
      }
    }
    const int cols = deep_dim(m, L);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * g + q;
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) {
        const int j = jt * kTW + n;
        if (i < m.d_out && j < cols) out[o.w[L] + i * cols + j] = Wo[jt][q];
      }
      float v = bo[q];
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d);
      if (n == 0 && i < m.d_out) out[o.b[L] + i] = v;
    }
  }
};

// Backward pass of one tile from the output gradient dy (lane (n, g): outputs 4 g + q of sample n, zero outside the batch and the
// outputs) to the wave's accumulators (wide_backward of csrc/pds_mlp_tile.h, its f32 form, down L hidden layers):
// dW(L+1) = dY^T HL, dZL = (W(L+1)^T dY) act'(HL), then per layer l = L .. 1: dWl = dZl^T H(l-1) (H0 = X),
// dZ(l-1) = (Wl^T dZl) act'(H(l-1)); the bias gradients on the way.  img: the tile's [sample][feature] images X, H1 .. HL of the
// forward pass (Hl is overwritten with dZl), then dY's.
template <int ACT, int L>
__device__ __forceinline__ void deep_backward(const float *Ws, const float *Wos, float *img, const f32x4 dy, DeepGrads<L> &G,
                                              int n, int g) {
  constexpr int kI = kTS * kS;
  float *dYimg = img + (L + 1) * kI;
  G.bo += dy;
  sts4(dYimg + n * kSY + 4 * g, dy);
  PDS_WAVE_SYNC();

  // Weight-gradient GEMMs take K = the tile's 16 samples: k-slot (j, h) carries sample 4 h + j, both operands are dword reads
  // of [sample][feature] images (conflict free).
  const int r = n, h = g;  // A-operand lane roles
  f32x4 cc[kNT], dz[kNT];
  {
    float *HL = img + L * kI;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // dW(L+1) += dY^T HL (rows = outputs)
      const float av = dYimg[(4 * h + j) * kSY + r];
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) G.Wo[jt] = PDS_MFMA(av, HL[(4 * h + j) * kS + jt * kTW + n], G.Wo[jt]);
    }
    // dZL^T = (W(L+1)^T dY^T) * act'(HL^T); the k-slot (j, h) carries output 4 h + j = register j of dy
#pragma unroll
    for (int it = 0; it < kNT; ++it) cc[it] = (f32x4)(0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int it = 0; it < kNT; ++it) cc[it] = PDS_MFMA(Wos[((4 * h + j) & (kMaxOut - 1)) * kS + it * kTW + r], dy[j], cc[it]);
#pragma unroll
    for (int it = 0; it < kNT; ++it) {
      const f32x4 hv = lds4(HL + n * kS + it * kTW + 4 * g);  // this lane's own HL values
#pragma unroll
      for (int q = 0; q < 4; ++q) dz[it][q] = cc[it][q] * act_grad<ACT>(hv[q]);
      G.b[L - 1][it] += dz[it];
    }
#pragma unroll
    for (int it = 0; it < kNT; ++it) sts4(HL + n * kS + it * kTW + 4 * g, dz[it]);  // after the dW(L+1) reads (in order)
    PDS_WAVE_SYNC();
  }
#pragma unroll
  for (int l = L - 1; l >= 0; --l) {  // layer l + 1 of the network: its input image l, dZ(l+1) in image l + 1 and in dz
    const float *Zi = img + (l + 1) * kI;
    float *Hi = img + l * kI;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // dW(l+1) += dZ(l+1)^T H(l)
      float av[kNT], bv[kNT];
#pragma unroll
      for (int i = 0; i < kNT; ++i) {
        av[i] = Zi[(4 * h + j) * kS + i * kTW + r];
        bv[i] = Hi[(4 * h + j) * kS + i * kTW + n];
      }
#pragma unroll
      for (int it = 0; it < kNT; ++it)
#pragma unroll
        for (int jt = 0; jt < kNT; ++jt) G.W[l][it][jt] = PDS_MFMA(av[it], bv[jt], G.W[l][it][jt]);
    }
    if (l > 0) {
      // dZ(l)^T = (W(l+1)^T dZ(l+1)^T) * act'(H(l)^T): A = W^T read column-wise (4 dwords per k-tile)
      const float *Wl = Ws + l * kMaxDim * kS;
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) cc[jt] = (f32x4)(0.f);
#pragma unroll
      for (int kt = 0; kt < kNT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int jt = 0; jt < kNT; ++jt) cc[jt] = PDS_MFMA(Wl[(kt * kTW + 4 * h + j) * kS + jt * kTW + r], dz[kt][j], cc[jt]);
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) {
        const f32x4 hv = lds4(Hi + n * kS + jt * kTW + 4 * g);  // this lane's own H(l) values
#pragma unroll
        for (int q = 0; q < 4; ++q) dz[jt][q] = cc[jt][q] * act_grad<ACT>(hv[q]);
        G.b[l - 1][jt] += dz[jt];
      }
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) sts4(Hi + n * kS + jt * kTW + 4 * g, dz[jt]);  // after the dW(l+1) reads
    }
    PDS_WAVE_SYNC();  // (l == 0: the images are rewritten by the next tile)
  }
}

// weight images [out][in] of the network, zero padded, by the THREADS threads of a block (stage_wide of csrc/pds_mlp_tile.h down
// L hidden layers): per hidden layer [64][68] in Ws and its bias in bs, the output layer's 8 rows in Wos (rows 8..15 of the MFMA
// tile alias rows 0..7, see stage_wide) and its bias in bos; val(t, i) is what is staged for the parameter of value t at position
// i of the flat layout (the identity, or a line-search candidate)
template <int L, int THREADS, class F>
__device__ __forceinline__ void deep_stage(const pds_mlp_deep &m, float *Ws, float *Wos, float *bs, float *bos, int tid, F val) {
  const DeepOffsets o = deep_offsets(m);
  constexpr int kThreads = THREADS;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int rows = m.hidden[l], cols = l == 0 ? m.d_in : m.hidden[l > 0 ? l - 1 : 0];
    const float *w = m.w[l], *b = m.b[l];
    float *W = Ws + l * kMaxDim * kS;
    for (int i = tid; i < kMaxDim * kS; i += kThreads) {
      const int r = i / kS, k = i - r * kS;
      W[i] = (r < rows && k < cols) ? val(w[r * cols + k], o.w[l] + r * cols + k) : 0.f;
    }
    if (tid < kMaxDim) bs[l * kMaxDim + tid] = tid < rows ? val(b[tid], o.b[l] + tid) : 0.f;
  }
  {
    const int cols = m.hidden[L - 1];
    for (int i = tid; i < kMaxOut * kS; i += kThreads) {
      const int r = i / kS, k = i - r * kS;
      Wos[i] = (r < m.d_out && k < cols) ? val(m.w[L][r * cols + k], o.w[L] + r * cols + k) : 0.f;
    }
    if (tid < kTW) bos[tid] = tid < m.d_out ? val(m.b[L][tid], o.b[L] + tid) : 0.f;
  }
}

// Forward pass of one tile from cur (lane (n, g): features 16 kt + 4 g + q of sample n = the B operands of layer 1; on return this
// lane's HL values) to Y^T = W(L+1) HL^T + b(L+1) (lane (n, g): outputs 4 g + q of sample n; rows >= d_out: 0); activations stay in
// registers from layer to layer.  IMG: H1 .. HL also go to images 1 .. L of img ([sample][feature], for deep_backward)
template <int ACT, int L, bool IMG>
__device__ __forceinline__ f32x4 deep_forward(const float *Ws, const float *Wos, const float *bs, const float *bos,
                                              f32x4 (&cur)[kNT], float *img, int n, int g) {
  constexpr int kI = kTS * kS;
  // ---- forward: H(l)^T = act(W(l) H(l-1)^T + b(l)), rows >= the layer's width: act(0) = 0; layer tiles in pairs ----
#pragma unroll
  for (int l = 0; l < L; ++l) {
    f32x4 cc[kNT];
#pragma unroll
    for (int it = 0; it < kNT; it += 2) gemm_wt2s<kNT, kS>(Ws + l * kMaxDim * kS, it, cur, n, g, cc[it], cc[it + 1]);
#pragma unroll
    for (int it = 0; it < kNT; ++it) {
      const f32x4 b = lds4(bs + l * kMaxDim + it * kTW + 4 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) cur[it][q] = act_fn<ACT>(cc[it][q] + b[q]);
      if (IMG) sts4(img + (l + 1) * kI + n * kS + it * kTW + 4 * g, cur[it]);
    }
  }
  return gemm_lds<kNT, kS>(Wos, 0, cur, n & (kMaxOut - 1), g, (f32x4)(0.f)) + lds4(bos + 4 * g);
}

// PDS_OK for a network inside the range of include/pds_mlp_deep.h (d_in up to kMaxDimIn: 65 .. 192 is a valid network that the
// kernels do not cover), else PDS_EINVAL
static int deep_check(const pds_mlp_deep *m) {
  if (!m) return PDS_EINVAL;
  if (m->n_hidden == 2) {
    pds_api_detail::set_thread_error(
        "pds_mlp_deep: n_hidden == 2 is struct pds_mlp's network (pds_mlp_forward, pds_ppo_policy_grad_step, "
        "pds_value_grad_step); the deep entry points take n_hidden 3 or 4");
    return PDS_EINVAL;
  }
  if (m->n_hidden < 3 || m->n_hidden > PDS_MLP_DEEP_MAX_HIDDEN || m->d_in < 1 || m->d_in > kMaxDimIn || m->d_out < 1 ||
      m->d_out > kMaxOut || (m->activation != 0 && m->activation != 1))
    return PDS_EINVAL;
  for (int l = 0; l < m->n_hidden; ++l)
    if (m->hidden[l] < 1 || m->hidden[l] > kMaxDim) return PDS_EINVAL;
  for (int l = 0; l <= m->n_hidden; ++l)
    if (!m->w[l] || !m->b[l]) return PDS_EINVAL;
  return PDS_OK;
}

}  // namespace pds_mlp_detail
