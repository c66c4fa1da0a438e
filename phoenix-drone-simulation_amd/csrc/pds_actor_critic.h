// pds_actor_critic.h -- what the off-policy update kernels share (csrc/pds_ddpg.hip: one critic; csrc/pds_sac.hip: twin critics),
// each piece written once on the tile core of csrc/pds_mlp_tile.h (read its header first): an actor's action goes through NQ
// critics on [obs | action], and the gradient of -Q comes back INTO THE ACTION -- the gradient of a network with respect to its
// input, the one operation no on-policy trainer needs.  Per 16-sample tile of a wave:
//   load_obs      the first D columns of the replay row into the wave's X image and the lane's B operands; the actor runs on
//                 them (wide_forward: its staged W1 is zero beyond column D, so ONE X image serves actor and critics)
//   put_action    a = act_limit th (th = the algorithm's squashed action) into columns D .. D + 3 of the X image, and every
//                 lane reads its B operands back; the critics run on them with their activations in registers (forward_regs,
//                 csrc/pds_mlp_tile.h), so a critic needs no image of its own
//   action_grad   the critic's backward chain from dq = -1 (the loss is -Q.mean(); 1 / B at the reduction) WITHOUT weight-gradient
//                 accumulators: dZ2 = -W3q act'(H2q) (one output: no GEMM), dZ1 = (W2q^T dZ2) act'(H1q), da = Wa dZ1 with Wa
//                 the four action columns of W1q staged transposed as an 8-row image (the form of W3's), so da lands in the
//                 lanes and registers the actor's output has.  Twin critics (NQ = 2): the samples of a tile choose their critic
//                 independently, so BOTH critics' operands go through the chain, the other's dZ masked to zero per sample, into
//                 ONE set of accumulator tiles (a masked column adds exact zeros); at NQ = 1 the mask folds to `true`
//   bellman_write the separately rounded backup of the target kernels
// and, per kernel, the argument block, the LDS images of the 1 + NQ networks, a wave's place in the grid, the activation-pair
// launch and the shape check.  What differs between the algorithms (the squashing, the critic selection, the output gradient of
// the actor) stays in their files.  Everything here is inlined into its kernel; the warning of csrc/pds_mlp_tile.h holds: moving a
// statement must not reorder the MFMAs of any accumulator.
#pragma once
#include <type_traits>

#include "pds_mlp_tile.h"

namespace pds_mlp_detail {

constexpr int kAcNin = 4;  // input tiles: D + 4 <= 64
static_assert(wide_stride<kAcNin>() == kS, "the X image shares the 68-float stride");
constexpr int kAcImg = 3 * kTS * kS + kTS * kSY;  // X, H1, H2, dY per wave (gradient kernels; the target kernels hold X only)

struct AcArgs {
  pds_mlp pi, q[2];          // the actor and its critics (DDPG: q[0] only)
  const float *x;            // [rows, ldx]: replay rows [obs | act] (gradient), next observations (target)
  int ldx;
  const int64_t *index;      // optional gather: sample g reads row index[g]
  long long B;
  float limit, alpha;        // act_limit, entropy temperature (SAC)
  unsigned long long seed, call;  // noise contract (SAC)
  float *partials;           // gradient: [waves of the grid][pstride]
  int pstride;
  const float *rew, *done;   // target: [rows]
  float gamma;
  float *target;             // target: [rows], written at the ROW
};

// the staged images of the actor (net 0) and its NQ critics (nets 1 ..), every one at the 68-float stride:
// per network W1 64 x 68 + W2 64 x 68 + W3 8 x 68 + biases 144 floats = 37 568 B.  W1 comes LAST: it is read with b128 loads off
// one per-lane pointer, while W2 and W3 are also read dword by dword in the backward chains -- below 64 KB their constant
// address fits the 16-bit offset field of ds_read_b32 and neighbouring reads pair into ds_read2_b32 (with W1 first, sac_grad_kernel
// lost 48 of those pairs and 11 % of its speed at a mini-batch of 65 536)
template <int NQ>
struct AcLds {
  float W2[1 + NQ][kMaxDim * kS], W3[1 + NQ][kMaxOut * kS];
  float b1[1 + NQ][kMaxDim], b2[1 + NQ][kMaxDim], b3[1 + NQ][kTW];
  float W1[1 + NQ][kMaxDim * kS];

  __device__ __forceinline__ NetLds net(int i) const { return NetLds{W1[i], W2[i], W3[i], b1[i], b2[i], b3[i]}; }
  // by the THREADS threads of the block; the caller's __syncthreads() publishes the images
  template <int THREADS>
  __device__ __forceinline__ void stage(const AcArgs &a) {
    stage_wide<kS, THREADS>(a.pi, W1[0], W2[0], W3[0], b1[0], b2[0], b3[0], threadIdx.x, [](float t, int) { return t; });
#pragma unroll
    for (int c = 0; c < NQ; ++c)
      stage_wide<kS, THREADS>(a.q[c], W1[1 + c], W2[1 + c], W3[1 + c], b1[1 + c], b2[1 + c], b3[1 + c], threadIdx.x,
                              [](float t, int) { return t; });
  }
};

// Wa[r][k] = W1q[k][D + (r & 3)], r < 8: rows as W3's image; rows 4 .. 7 repeat rows 0 .. 3, so lane group 1 holds da as well
template <int THREADS>
__device__ __forceinline__ void stage_wa(const pds_mlp &q, int D, float *Wa) {
  for (int i = threadIdx.x; i < kMaxOut * kS; i += THREADS) {
    const int r = i / kS, k = i - r * kS;
    Wa[i] = k < q.h1 ? q.w1[k * q.d_in + D + (r & 3)] : 0.f;
  }
}

// a wave of a grid of WAVES-wave blocks: lane (n, g) holds column (sample) n and rows 4 g + q of the C/D layout; the wave takes
// the tiles wid, wid + nw, .. of ntiles
struct WaveTiles {
  int lane, wave, n, g;
  long long wid, nw, ntiles;
};
template <int WAVES>
__device__ __forceinline__ WaveTiles wave_tiles(long long B) {
  WaveTiles w;
  w.lane = threadIdx.x & 63; w.wave = threadIdx.x >> 6;
  w.n = w.lane & 15; w.g = w.lane >> 4;
  w.wid = (long long)blockIdx.x * WAVES + w.wave; w.nw = (long long)gridDim.x * WAVES;
  w.ntiles = (B + kTS - 1) / kTS;
  return w;
}
// source row of this lane's sample in tile t, -1: none
__device__ __forceinline__ long long tile_row(const AcArgs &a, long long t, int n) {
  const long long s = t * kTS + n;
  if (s >= a.B) return -1;
  return a.index != nullptr ? a.index[s] : s;
}

// this lane's B operands of the first layer from row `row` of a.x (columns < D; the stored action is not read: 0 x inf), also
// into the wave's X image
__device__ __forceinline__ void load_obs(const AcArgs &a, long long row, float *Ximg, f32x4 (&xin)[kAcNin], int n, int g) {
  const int D = a.pi.d_in;
#pragma unroll
  for (int kt = 0; kt < kAcNin; ++kt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kt * kTW + 4 * g + q;
      xin[kt][q] = (row >= 0 && k < D) ? a.x[row * a.ldx + k] : 0.f;
    }
    sts4(Ximg + n * kS + kt * kTW + 4 * g, xin[kt]);
  }
}

// a = act_limit th into columns D .. D + 3 of the X image (D + 3 <= 63), then every lane's B operands read back
__device__ __forceinline__ void put_action(const AcArgs &a, const f32x4 th, float *Ximg, f32x4 (&xin)[kAcNin], int n, int g) {
  const int D = a.pi.d_in;
  PDS_WAVE_SYNC();
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) Ximg[n * kS + D + q] = a.limit * th[q];
  }
  PDS_WAVE_SYNC();
#pragma unroll
  for (int kt = 0; kt < kAcNin; ++kt) xin[kt] = lds4(Ximg + n * kS + kt * kTW + 4 * g);
}

// da = d(-Q_c) / d(action) of the critic c each sample chose (NQ = 2: c = first ? 0 : 1; NQ = 1: c = 0), in lane groups 0 and 1.
// Q: the critics' images, Wa: their action-column images, h1s / h2s: the CHOSEN critic's activations of this lane's sample
template <int AQ, int NQ>
__device__ __forceinline__ f32x4 action_grad(const NetLds (&Q)[NQ], const float *const (&Wa)[NQ], const f32x4 (&h1s)[kNT],
                                             const f32x4 (&h2s)[kNT], bool valid, bool first, int n, int g) {
  f32x4 dz[NQ][kNT], cc[kNT];
  bool pick[NQ];  // this sample runs through critic c
#pragma unroll
  for (int c = 0; c < NQ; ++c) pick[c] = NQ == 1 || (c == 0) == first;
#pragma unroll
  for (int it = 0; it < kNT; ++it) {  // dZ2 = W3q^T dq * act'(H2q): one output row, no GEMM
    f32x4 w3[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) w3[c] = lds4(Q[c].W3 + it * kTW + 4 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float gr = act_grad<AQ>(h2s[it][q]);
#pragma unroll
      for (int c = 0; c < NQ; ++c) dz[c][it][q] = (valid && pick[c]) ? -w3[c][q] * gr : 0.f;
    }
    cc[it] = (f32x4)(0.f);
  }
#pragma unroll
  for (int kt = 0; kt < kNT; ++kt)  // dZ1^T = (W2q^T dZ2^T) * act'(H1q^T), as wide_backward
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt)
#pragma unroll
        for (int c = 0; c < NQ; ++c) cc[jt] = PDS_MFMA(Q[c].W2[(kt * kTW + 4 * g + j) * kS + jt * kTW + n], dz[c][kt][j], cc[jt]);
#pragma unroll
  for (int jt = 0; jt < kNT; ++jt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v = cc[jt][q] * act_grad<AQ>(h1s[jt][q]);
#pragma unroll
      for (int c = 0; c < NQ; ++c) dz[c][jt][q] = pick[c] ? v : 0.f;
    }
  // da = W1q[:, D : D + 4]^T dZ1: lane groups 2 and 3 hold aliased rows
  f32x4 da = (f32x4)(0.f);
#pragma unroll
  for (int c = 0; c < NQ; ++c) da = gemm_lds<kNT, kS>(Wa[c], 0, dz[c], n & (kMaxOut - 1), g, da);
  return da;
}

// target[row] = rew[row] + gamma (1 - done[row]) v, every product and the sum rounded separately (torch's
// `r + gamma * (1 - d) * v`)
__device__ __forceinline__ void bellman_write(const AcArgs &a, long long row, float v) {
  a.target[row] = __fadd_rn(a.rew[row], __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.f, a.done[row])), v));
}

// f(AP, AQ) with the activations of the actor and of the critics as integral constants: f launches its kernel<AP, AQ>
template <class F>
void for_activations(const AcArgs &a, F f) {
  using A0 = std::integral_constant<int, 0>;
  using A1 = std::integral_constant<int, 1>;
  if (a.pi.activation == 0) {
    if (a.q[0].activation == 0) f(A0{}, A0{}); else f(A0{}, A1{});
  } else {
    if (a.q[0].activation == 0) f(A1{}, A0{}); else f(A1{}, A1{});
  }
}

// PDS_OK, PDS_EINVAL (a network outside every kernel family, the actor's d_out not `d_out`, Q d_out != 1, Q d_in != D + 4) or
// PDS_EUNSUPPORTED (D + 4 > 64)
inline int ac_check(const pds_mlp *pi, const pds_mlp *q, int d_out) {
  if (check(pi) != PDS_OK || check(q) != PDS_OK || pi->d_out != d_out || q->d_out != 1 || q->d_in != pi->d_in + 4) return PDS_EINVAL;
  return q->d_in <= kMaxDim ? PDS_OK : PDS_EUNSUPPORTED;
}

// the id packing of PDS_GAUSSIAN_PHILOX holds sample ids below 2^56: ids id_base .. id_base + n - 1, n >= 1
inline bool sample_ids_ok(uint64_t id_base, int64_t n) {
  return n >= 1 && id_base <= (1ull << 56) && (uint64_t)n <= (1ull << 56) - id_base;
}

}  // namespace pds_mlp_detail
