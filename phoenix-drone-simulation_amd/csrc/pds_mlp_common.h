// pds_mlp_common.h -- what the trainer's dense kernels share (csrc/pds_mlp.hip: d_in <= 64, two waves per SIMD;
// csrc/pds_mlp_wide.hip: 64 < d_in <= 192, the first layer K-tiled; csrc/pds_npg.hip: the natural-gradient step): argument
// block, parameter layout, activations, LDS access helpers.  See pds_mlp.hip for the design; the tile code of the K-tiled
// kernels is csrc/pds_mlp_tile.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pds.h"

namespace pds_mlp_detail {  // named (not anonymous) so that profiler kernel names are readable

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTS = 16;            // samples per wave tile (= N of every activation GEMM)
constexpr int kTW = 16;            // feature tile width
constexpr int kNT = 4;             // 16-wide tiles per 64-wide dimension
constexpr int kS = 68;             // image row stride: 16-B aligned rows (b128 access) and 4 * kS == 16 (mod 32),
                                   // so the sample-slot walk of the dword reads below is bank-conflict free
constexpr int kSY = 20;            // row stride of the [16 samples][16 outputs] output-gradient image (same rule)
constexpr int kMaxDim = 64;        // d_in, h1, h2 <= 64
constexpr int kMaxOut = 8;         // d_out <= 8
constexpr int kWaves = 8;          // waves per block, two per SIMD; 1 block per CU (LDS-bound)
constexpr int kStats = 4;          // loss sum, ratio sum, kl sum, sample count
constexpr int kWaveFloats = 3 * kTS * kS + kTS * kSY;
// the K-tiled kernels (csrc/pds_mlp_tile.h): csrc/pds_mlp_wide.hip for 64 < d_in <= 192, csrc/pds_npg.hip for every d_in
constexpr int kMaxDimIn = 192;     // d_in of the K-tiled kernels (twelve 16-wide input tiles)
constexpr int kWideWaves = 4;      // waves per block there: one per SIMD, up to 512 registers each
constexpr int kWideMaxBlocks = 256;

enum { LOSS_NONE = 0, LOSS_PPO = 1, LOSS_MSE = 2 };

struct Args {
  pds_mlp m;
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

// ACT 0 relu, 1 tanh (branch-free: 1 - 2 / (e^{2v} + 1) on v_exp_f32 / v_rcp_f32, abs error < 3e-7)
template <int ACT>
__device__ __forceinline__ float act_fn(float v) {
  if (ACT == 0) return fmaxf(v, 0.f);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * v) + 1.f);
}
// derivative expressed through the activation's OUTPUT h (relu: h > 0; tanh: 1 - h^2)
template <int ACT>
__device__ __forceinline__ float act_grad(float h) { return ACT == 0 ? (h > 0.f ? 1.f : 0.f) : 1.f - h * h; }

// flat parameter layout == torch's nn.Sequential order: W1 [h1][d_in], b1, W2 [h2][h1], b2, W3 [d_out][h2], b3
struct Offsets {
  int w1, b1, w2, b2, w3, b3, total;
};
__host__ __device__ inline Offsets offsets(const pds_mlp &m) {
  Offsets o;
  o.w1 = 0;
  o.b1 = o.w1 + m.h1 * m.d_in;
  o.w2 = o.b1 + m.h1;
  o.b2 = o.w2 + m.h2 * m.h1;
  o.w3 = o.b2 + m.h2;
  o.b3 = o.w3 + m.d_out * m.h2;
  o.total = o.b3 + m.d_out;
  return o;
}
// parameter p of the flat layout (o = offsets of the network): f(the tensor it lies in, as a member of pds_mlp; its index there)
template <class F>
__device__ __forceinline__ void at_param(const Offsets &o, int p, F f) {
  if (p < o.b1) f(&pds_mlp::w1, p);
  else if (p < o.w2) f(&pds_mlp::b1, p - o.b1);
  else if (p < o.b2) f(&pds_mlp::w2, p - o.w2);
  else if (p < o.w3) f(&pds_mlp::b2, p - o.b2);
  else if (p < o.b3) f(&pds_mlp::w3, p - o.w3);
  else f(&pds_mlp::b3, p - o.b3);
}
// ... of network m, as a pointer
__device__ __forceinline__ float *param_ptr(const pds_mlp &m, const Offsets &o, int p) {
  float *ptr;
  at_param(o, p, [&](const float *pds_mlp::*w, int i) { ptr = const_cast<float *>(m.*w) + i; });
  return ptr;
}

// torch.optim.Adam (no weight decay, no amsgrad), stated once for pds_adam_step (csrc/pds_train.hip adam_kernel) and for the
// step that rides on the partial-sum kernel of a gradient call (csrc/pds_mlp.hip reduce_kernel): same source, same bits.
// The build fuses a * b + c only inside one source expression (-ffp-contract=on), so these expressions stay whole as written.
struct AdamK {
  float *em, *ev;  // exp_avg, exp_avg_sq [total]; em == nullptr: no step
  float lr, b1, b2, eps, bc1, bc2s;
};
// the rule every entry point with a `const pds_adam *opt` applies: no step, or a step with its moments and a count from 1
inline bool adam_ok(const pds_adam *opt) { return opt == nullptr || (opt->d_exp_avg && opt->d_exp_avg_sq && opt->step >= 1); }
inline AdamK adam_k(const pds_adam *opt) {
  AdamK ad{};
  if (opt != nullptr) {
    ad.em = opt->d_exp_avg; ad.ev = opt->d_exp_avg_sq;
    ad.lr = opt->lr; ad.b1 = opt->beta1; ad.b2 = opt->beta2; ad.eps = opt->eps;
    ad.bc1 = 1.0f - powf(opt->beta1, (float)opt->step);
    ad.bc2s = sqrtf(1.0f - powf(opt->beta2, (float)opt->step));
  }
  return ad;
}
// m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; *dst -= lr / (1-b1^t) * m / (sqrt(v) / sqrt(1-b2^t) + eps) for parameter p
__device__ __forceinline__ void adam_apply(const AdamK &ad, int p, float gr, float *dst) {
  const float mm = ad.b1 * ad.em[p] + (1.f - ad.b1) * gr;
  const float vv = ad.b2 * ad.ev[p] + (1.f - ad.b2) * gr * gr;
  ad.em[p] = mm; ad.ev[p] = vv;
  const float denom = sqrtf(vv) / ad.bc2s + ad.eps;
  *dst = *dst - (ad.lr / ad.bc1) * (mm / denom);
}

#define PDS_WAVE_SYNC()                                          \
  do {                                                           \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       \
    __builtin_amdgcn_wave_barrier();                             \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");       \
  } while (0)

#define PDS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ f32x4 lds4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void sts4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// ---- split-bf16 operands (round 6) ------------------------------------------------------------------------------
// x = hi + mid + lo, three bf16 pieces (round to nearest even; the residuals x - hi and (x - hi) - mid are exact in f32), and
// the six products hi hi, hi mid, mid hi, hi lo, lo hi, mid mid on v_mfma_f32_16x16x32_bf16 (16 cycles per K = 32 against
// 8 x 32 for v_mfma_f32_16x16x4_f32): products exact, one f32 rounding per 32 terms -- max error / sum |products| 2^-24.5 ..
// 2^-23.1, below the f32 MFMA's own 2^-22.6 .. 2^-21.8 (profiles/r06_split_bf16.txt).  4.5 vector instructions per element.
typedef float f32x2_ __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_ __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {  // v_cvt_pk_bf16_f32: low half a, high half b
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_){a, b}, bf16x2_));
}
struct Quad3 { u32x2_ hi, mid, lo; };  // four values in three pieces, two dwords per piece
__device__ __forceinline__ Quad3 split4(const f32x4 x) {
  Quad3 s;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t h = pk_bf16(x[2 * p], x[2 * p + 1]);
    const float r0 = x[2 * p] - __uint_as_float(h << 16), r1 = x[2 * p + 1] - __uint_as_float(h & 0xFFFF0000u);
    const uint32_t m = pk_bf16(r0, r1);
    s.hi[p] = h;
    s.mid[p] = m;
    s.lo[p] = pk_bf16(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xFFFF0000u));
  }
  return s;
}
// the 8 k-slots of a lane: slots 0..3 = `a`, slots 4..7 = `b`
__device__ __forceinline__ bf16x8_ cat8(const u32x2_ a, const u32x2_ b) {
  const u32x4_ v = {a[0], a[1], b[0], b[1]};
  return __builtin_bit_cast(bf16x8_, v);
}
#define PDS_MFMA_BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
// C += A B over the 8 k-slots of every lane group, A = (a0 | a1), B = (b0 | b1) in three pieces each: the six products, smallest first
struct Oct3 { bf16x8_ hi, mid, lo; };
__device__ __forceinline__ Oct3 oct3(const Quad3 &a, const Quad3 &b) { return Oct3{cat8(a.hi, b.hi), cat8(a.mid, b.mid), cat8(a.lo, b.lo)}; }

// csrc/pds_mlp_wide.hip: launches mlp_wide_kernel<loss, activation, input tiles> on `s`; returns the number of partials
// (one per wave of the grid) that the reduce kernel has to sum (gradient calls)
int launch_wide(int loss, const Args &a, hipStream_t s);
// csrc/pds_mlp.hip: PDS_OK for a network every kernel family covers between them (d_in <= kMaxDimIn, h1, h2 <= kMaxDim,
// d_out <= kMaxOut, relu or tanh, no null tensor), else PDS_EINVAL
int check(const pds_mlp *m);
// csrc/pds_mlp.hip: launches reduce_kernel on `s` -- grads[p] = scale * the fixed-order sum of element p over the nparts
// partials, stats = the sums of the kStats elements behind them, and the Adam step on `m` when opt != nullptr
int launch_reduce(const float *partials, int pstride, int nparts, int total, float scale, float *grads, float *stats,
                  const pds_mlp &m, const pds_adam *opt, hipStream_t s);

}  // namespace pds_mlp_detail
