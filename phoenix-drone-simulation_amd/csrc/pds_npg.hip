// pds_npg.hip -- the natural-gradient policy step of NPG and TRPO (algs/npg/npg.py:52-160, algs/trpo/trpo.py:16-66,
// algs/utils.py:5-38) on gfx950: the Fisher-vector product, one conjugate-gradient iteration, and the evaluation of the
// line-search candidates.
//
// Fisher-vector product.  The actor's log_std is not trained (algs/core.py:238-240), and at theta_old the gradient of
// KL(p_old || p_theta) with respect to the mean is zero, so the double-backward Hessian of the reference's Fvp is exactly
// the Gauss-Newton form
//     F v = 1 / (B A) sum_i J_i^T diag(exp(-2 log_std)) J_i v,     J_i = d mu(x_i) / d theta,
// for relu and tanh alike: per sample one forward pass with a tangent (J v), a scale, and one backward pass (J^T u).
// The kernels stand on the tile core of csrc/pds_mlp_tile.h (its header states the design; shared with mlp_wide_kernel of
// csrc/pds_mlp_wide.hip): a wave owns a 16-sample tile in LDS, every GEMM runs on v_mfma_f32_16x16x4_f32 with the transposed
// chain, the weight gradients accumulate in registers over the wave's tiles (WideGrads), every wave writes one partial, and a
// second kernel sums the partials in a fixed order (sum_partials: deterministic, no atomics) and applies the 1 / (B A) scale
// and the damping.  One wave per SIMD and the first layer K-tiled over up to twelve input tiles: every shape of the fused PPO
// path (d_in <= 192, h1, h2 <= 64, d_out <= 8).  What this file adds: the forward pass with a tangent, the f32 backward chain
// (wide_backward<.., false>), conjugate gradients, and the candidates' staging transform.  The tangent's weights
// v are read from global memory (L2-resident, 5-17 k floats): LDS holds W1 / W2 / W3 and the four images per wave, as in
// the wide kernel, and would not hold a second copy of W1 at 192 inputs.
//   tangent   dz1 = V1 x + vb1,  dz2 = V2 h1 + W2 (act'(z1) dz1) + vb2,  dmu = V3 h2 + W3 (act'(z2) dz2) + vb3
//   scale     u = dmu exp(-2 log_std)
//   backward  wide_backward from u: dW3 = u^T h2, dZ2 = (W3^T u) act'(z2), dW2 = dZ2^T h1, dZ1 = (W2^T dZ2) act'(z1), dW1 = dZ1^T x
// act' follows torch: relu' = (z > 0) = (h > 0), tanh' = 1 - h^2.
//
// Line-search candidates (TRPO): grid.y = candidate j, whose parameters theta_old + f_j s are formed while the weights are
// staged into LDS -- the product and the sum rounded separately (__fmul_rn / __fadd_rn, as torch's `theta + f * s` with f
// rounded to float32), so the trainer can write the accepted candidate with the same expression, bit for bit.  Per
// candidate: sum(ratio adv), sum of KL(p_old || q) over samples x actions and sum(ratio), in a fixed order.
#include "pds_npg_tile.h"

namespace pds_mlp_detail {

constexpr int kCgThreads = 1024;

struct NpgArgs {
  pds_mlp m;
  const float *x;            // standardised rows [rows, d_in]
  const int64_t *index;      // optional gather (fvp)
  long long B;
  const float *log_std;      // [d_out]
  const float *v;            // fvp: tangent, flat parameter layout;  surrogate: step s
  const float *fracs;        // surrogate: step fractions [J]
  const float *act, *adv, *logp_old, *mu_old;  // surrogate
  float *partials;
  float *theta_out;          // surrogate: optional [J][total] candidate parameters
  int pstride;
};

// layer 1 with the B operand (this lane's own 4 features per input tile) read back from its row of the X image instead of
// held in 4 NK registers: what keeps the fvp kernel at 192 inputs free of spills
template <int NK, int S>
__device__ __forceinline__ f32x4 gemm_lds_x(const float *Ws, int it, const float *xrow, int n, int g, f32x4 c) {
  const float *wp = Ws + (it * kTW + n) * S + 4 * g;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt) {
    const f32x4 a = lds4(wp + kt * kTW), b = lds4(xrow + kt * kTW);
#pragma unroll
    for (int j = 0; j < 4; ++j) c = PDS_MFMA(a[j], b[j], c);
  }
  return c;
}
template <int NK>
__device__ __forceinline__ f32x4 gemm_glb_x(const float *V, int rows, int cols, int it, const float *xrow, int n, int g,
                                            f32x4 c) {
  const int r = it * kTW + n;
  const bool rin = r < rows;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt) {
    const f32x4 b = lds4(xrow + kt * kTW);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kt * kTW + 4 * g + j;
      const float av = (rin && k < cols) ? V[r * cols + k] : 0.f;
      c = PDS_MFMA(av, b[j], c);
    }
  }
  return c;
}

// parameter i of the flat layout, read from the network's six tensors
__device__ __forceinline__ float theta_at(const pds_mlp &m, const Offsets &o, int i) { return *param_ptr(m, o, i); }

template <int ACT, int NIN>
__global__ __launch_bounds__(kWideWaves * 64, 1) void fvp_kernel(const NpgArgs a) {
  constexpr int S1 = wide_stride<NIN>();
  constexpr int kImg = kTS * S1 + 2 * kTS * kS + kTS * kSY;  // X, H1, H2, U per wave
  __shared__ __attribute__((aligned(16))) float W1s[kMaxDim * S1];
  __shared__ __attribute__((aligned(16))) float W2s[kMaxDim * kS];
  __shared__ __attribute__((aligned(16))) float W3s[kMaxOut * kS];
  __shared__ __attribute__((aligned(16))) float b1s[kMaxDim], b2s[kMaxDim], b3s[kTW], isg2[kTW];
  __shared__ __attribute__((aligned(16))) float images[kWideWaves * kImg];
  const pds_mlp &m = a.m;
  const Offsets o = offsets(m);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;  // C/D layout: column (sample) n, rows 4 g + q
  stage_wide<S1>(m, W1s, W2s, W3s, b1s, b2s, b3s, tid, [](float t, int) { return t; });
  if (tid < kTW) {
    const float is = tid < m.d_out ? expf(-a.log_std[tid]) : 0.f;  // 1 / sigma
    isg2[tid] = is * is;
  }
  float *Ximg = images + wave * kImg;
  float *H1img = Ximg + kTS * S1, *H2img = H1img + kTS * kS, *Uimg = H2img + kTS * kS;
  for (int i = lane; i < kImg; i += 64) Ximg[i] = 0.f;
  __syncthreads();
  const float *V1 = a.v + o.w1, *vb1 = a.v + o.b1, *V2 = a.v + o.w2, *vb2 = a.v + o.b2, *V3 = a.v + o.w3, *vb3 = a.v + o.b3;

  WideGrads<NIN> G;
  G.zero();

  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kWideWaves + wave, nw = (long long)gridDim.x * kWideWaves;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    const bool valid = row >= 0;
    float *xrow = Ximg + n * S1 + 4 * g;  // this lane's features 16 kt + 4 g + q (the B operands of layer 1)
#pragma unroll
    for (int kt = 0; kt < NIN; ++kt) {
      f32x4 xv;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kt * kTW + 4 * g + q;
        xv[q] = (valid && k < m.d_in) ? a.x[row * m.d_in + k] : 0.f;
      }
      sts4(xrow + kt * kTW, xv);
    }
    // ---- layer 1: h1 = act(W1 x + b1), its tangent t1 = act'(h1) (V1 x + vb1) ----------------------------------------
    f32x4 h1r[kNT], t1[kNT], h2r[kNT], t2[kNT];
#pragma unroll
    for (int it = 0; it < kNT; ++it) {
      const f32x4 z = gemm_lds_x<NIN, S1>(W1s, it, xrow, n, g, (f32x4)(0.f));
      const f32x4 dz = gemm_glb_x<NIN>(V1, m.h1, m.d_in, it, xrow, n, g, (f32x4)(0.f));
      const f32x4 b = lds4(b1s + it * kTW + 4 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = it * kTW + 4 * g + q;
        h1r[it][q] = act_fn<ACT>(z[q] + b[q]);
        t1[it][q] = act_grad<ACT>(h1r[it][q]) * (dz[q] + (i < m.h1 ? vb1[i] : 0.f));
      }
      sts4(H1img + n * kS + it * kTW + 4 * g, h1r[it]);
    }
    // ---- layer 2: h2 = act(W2 h1 + b2), t2 = act'(h2) (V2 h1 + W2 t1 + vb2) -------------------------------------------
#pragma unroll
    for (int it = 0; it < kNT; ++it) {
      const f32x4 z = gemm_lds<kNT, kS>(W2s, it, h1r, n, g, (f32x4)(0.f));
      f32x4 dz = gemm_lds<kNT, kS>(W2s, it, t1, n, g, (f32x4)(0.f));
      dz = gemm_glb<kNT>(V2, m.h2, m.h1, it, h1r, n, g, dz);
      const f32x4 b = lds4(b2s + it * kTW + 4 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = it * kTW + 4 * g + q;
        h2r[it][q] = act_fn<ACT>(z[q] + b[q]);
        t2[it][q] = act_grad<ACT>(h2r[it][q]) * (dz[q] + (i < m.h2 ? vb2[i] : 0.f));
      }
      sts4(H2img + n * kS + it * kTW + 4 * g, h2r[it]);
    }
    // ---- output tangent dmu = V3 h2 + W3 t2 + vb3, u = dmu / sigma^2 (zero outside the batch and the outputs) --------
    f32x4 u;
    {
      f32x4 dm = gemm_lds<kNT, kS>(W3s, 0, t2, n & (kMaxOut - 1), g, (f32x4)(0.f));
      dm = gemm_glb<kNT>(V3, m.d_out, m.h2, 0, h2r, n, g, dm);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * g + q;
        u[q] = (valid && j < m.d_out) ? (dm[q] + vb3[j]) * isg2[j] : 0.f;
      }
    }
    wide_backward<ACT, NIN, false>(W2s, W3s, Ximg, H1img, H2img, Uimg, u, h2r, G, n, g);
  }

  // ---- this wave's partial -> partials[wave of the grid][flat parameter layout] ------------------------------------------
  G.store(m, o, a.partials + wid * a.pstride, n, g);
}

// out[p] = scale * sum over the waves' partials (sum_partials) + damping v[p].  out may alias v.
__global__ __launch_bounds__(1024) void fvp_reduce_kernel(const float *partials, int pstride, int nwaves, int total, float scale,
                                                          float damping, const float *v, float *out) {
  const int p = blockIdx.x * 64 + (threadIdx.x & 63);
  const float t = sum_partials(partials, pstride, nwaves, p, p < total);
  if ((threadIdx.x >> 6) == 0 && p < total) {
    const float fv = __fmul_rn(t, scale);  // flat_grad_grad_kl + v * cg_damping: two products, one sum
    out[p] = __fadd_rn(fv, __fmul_rn(v[p], damping));
  }
}

// ---- conjugate gradients (algs/utils.py:5-38), one iteration per launch, one workgroup --------------------------------
// dot product over n elements in a fixed order: thread-strided chains, a butterfly inside each wave, the 16 waves in order
__device__ __forceinline__ float cg_dot(const float *a, const float *b, long long n, float *red) {
  const int tid = threadIdx.x;
  float s = 0.f;
  for (long long i = tid; i < n; i += kCgThreads) s = __fadd_rn(s, __fmul_rn(a[i], b[i]));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  __syncthreads();  // (red is reused by consecutive dots)
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < kCgThreads / 64; ++w) t += red[w];
  return t;
}

// st = {r.r, stopped}.  init: x = 0, r = p = b (= z: Avp(0) is 0), st = {b.b, 0}.  Otherwise, with z = Avp(p), unless
// stopped: alpha = r.r / (p.z + eps); x += alpha p; r -= alpha z; stop when |r| < tol (the reference's break: x and r
// updated, p kept); else p = r + (r.r new / (r.r + eps)) p.  Every thread reads st before the first barrier, thread 0
// writes it after the last one.
__global__ __launch_bounds__(kCgThreads) void cg_kernel(long long n, float *x, float *r, float *p, const float *z, float *st,
                                                        float eps, float tol, int init) {
  __shared__ float red[kCgThreads / 64];
  const int tid = threadIdx.x;
  if (init) {
    for (long long i = tid; i < n; i += kCgThreads) {
      const float b = z[i];
      x[i] = 0.f; r[i] = b; p[i] = b;
    }
    __syncthreads();
    const float rr = cg_dot(r, r, n, red);
    if (tid == 0) { st[0] = rr; st[1] = 0.f; }
    return;
  }
  const float rdotr = st[0];
  if (st[1] != 0.f) return;
  const float alpha = rdotr / (cg_dot(p, z, n, red) + eps);
  for (long long i = tid; i < n; i += kCgThreads) {
    x[i] = __fadd_rn(x[i], __fmul_rn(alpha, p[i]));
    r[i] = __fsub_rn(r[i], __fmul_rn(alpha, z[i]));
  }
  __syncthreads();
  const float nr = cg_dot(r, r, n, red);
  if (sqrtf(nr) < tol) {
    if (tid == 0) st[1] = 1.f;
    return;
  }
  const float mu = nr / (rdotr + eps);
  for (long long i = tid; i < n; i += kCgThreads) p[i] = __fadd_rn(r[i], __fmul_rn(mu, p[i]));
  if (tid == 0) st[0] = nr;
}

// ---- line-search candidates: sum(ratio adv) and sum KL(p_old || q) per candidate ---------------------------------------
template <int ACT, int NIN>
__global__ __launch_bounds__(kWideWaves * 64, 1) void surrogate_kernel(const NpgArgs a) {
  constexpr int S1 = wide_stride<NIN>();
  __shared__ __attribute__((aligned(16))) float W1s[kMaxDim * S1];
  __shared__ __attribute__((aligned(16))) float W2s[kMaxDim * kS];
  __shared__ __attribute__((aligned(16))) float W3s[kMaxOut * kS];
  __shared__ __attribute__((aligned(16))) float b1s[kMaxDim], b2s[kMaxDim], b3s[kTW], lsg[kTW], sgg[kTW], vrg[kTW];
  const pds_mlp &m = a.m;
  const Offsets o = offsets(m);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int cj = blockIdx.y;
  const float f = a.fracs[cj];
  // the candidate's parameters theta + f s are formed while the weights are staged
  stage_wide<S1>(m, W1s, W2s, W3s, b1s, b2s, b3s, tid, [&](float t, int i) { return cand(t, f, a.v[i]); });
  if (tid < kTW) {
    const float ls = tid < m.d_out ? a.log_std[tid] : 0.f;
    const float sg = expf(ls);
    lsg[tid] = ls; sgg[tid] = sg; vrg[tid] = sg * sg;
  }
  if (a.theta_out != nullptr && blockIdx.x == 0)
    for (int i = tid; i < o.total; i += kWideWaves * 64) a.theta_out[(long long)cj * o.total + i] = cand(theta_at(m, o, i), f, a.v[i]);
  __syncthreads();

  float st_ra = 0.f, st_kl = 0.f, st_r = 0.f;
  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kWideWaves + wave, nw = (long long)gridDim.x * kWideWaves;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long smp = t * kTS + n;
    const bool valid = smp < a.B;
    f32x4 xin[NIN];
#pragma unroll
    for (int kt = 0; kt < NIN; ++kt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kt * kTW + 4 * g + q;
        xin[kt][q] = (valid && k < m.d_in) ? a.x[smp * m.d_in + k] : 0.f;
      }
    f32x4 h2r[kNT];
    const f32x4 y = wide_forward<ACT, NIN, false>(W1s, W2s, W3s, b1s, b2s, b3s, xin, nullptr, nullptr, h2r, n, g);
    // Normal(mu, sigma).log_prob(act).sum(-1) and kl_divergence(Normal(mu_old, sigma), Normal(mu, sigma)) in torch's
    // expressions: -(a - mu)^2 / (2 var) - log sigma - log sqrt(2 pi);  0.5 (1 + ((mu_old - mu) / sigma)^2 - 1 - log 1)
    float lp = 0.f, kl = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * g + q;
      if (valid && j < m.d_out) {
        const float d = a.act[smp * m.d_out + j] - y[q];
        const float dd = d * d;
        lp += -dd / (2.f * vrg[j]) - lsg[j] - 0.91893853320467274178f;
        const float e = (a.mu_old[smp * m.d_out + j] - y[q]) / sgg[j];
        const float t1 = e * e;
        const float vr = 1.f + t1;
        kl += 0.5f * (vr - 1.f);
      }
    }
    lp += __shfl_xor(lp, 16); lp += __shfl_xor(lp, 32);
    kl += __shfl_xor(kl, 16); kl += __shfl_xor(kl, 32);
    if (valid && g == 0) {
      const float ratio = expf(lp - a.logp_old[smp]);
      st_ra += ratio * a.adv[smp];
      st_kl += kl;
      st_r += ratio;
    }
  }
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) {
    st_ra += __shfl_xor(st_ra, d); st_kl += __shfl_xor(st_kl, d); st_r += __shfl_xor(st_r, d);
  }
  if (lane == 0) {
    float *out = a.partials + ((long long)cj * nw + wid) * 3;
    out[0] = st_ra; out[1] = st_kl; out[2] = st_r;
  }
}

// one wave per candidate: out[j] = {sum ratio adv, sum kl, non-finite, sum ratio} over the waves' partials in a fixed order
__global__ __launch_bounds__(64) void surrogate_reduce_kernel(const float *partials, int nwaves, float *out) {
  const int cj = blockIdx.x, lane = threadIdx.x;
  const float *pp = partials + (long long)cj * nwaves * 3;
  float ra = 0.f, kl = 0.f, rs = 0.f;
  for (int w = lane; w < nwaves; w += 64) { ra += pp[3 * w]; kl += pp[3 * w + 1]; rs += pp[3 * w + 2]; }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { ra += __shfl_xor(ra, d); kl += __shfl_xor(kl, d); rs += __shfl_xor(rs, d); }
  if (lane == 0) {
    out[4 * cj] = ra;
    out[4 * cj + 1] = kl;
    out[4 * cj + 2] = (isfinite(ra) && isfinite(kl)) ? 0.f : 1.f;
    out[4 * cj + 3] = rs;
  }
}

// the launches of the two reduce kernels (declared in pds_npg_tile.h: csrc/pds_npg_deep.hip sums its partials with them too)
void npg_reduce_fvp(hipStream_t s, const float *partials, int pstride, int nwaves, int total, float scale, float damping,
                    const float *v, float *out) {
  hipLaunchKernelGGL(fvp_reduce_kernel, dim3((total + 63) / 64), dim3(1024), 0, s, partials, pstride, nwaves, total, scale, damping,
                     v, out);
}
void npg_reduce_surrogate(hipStream_t s, const float *partials, int nwaves, int num_candidates, float *out) {
  hipLaunchKernelGGL(surrogate_reduce_kernel, dim3(num_candidates), dim3(64), 0, s, partials, nwaves, out);
}

// input tiles: 2 (d_in <= 32), 4 (<= 64), 8 (<= 128), 12 (<= 192)
template <int ACT>
static void launch_fvp(int nin, dim3 g, hipStream_t s, const NpgArgs &a) {
  const dim3 b(kWideWaves * 64);
  if (nin <= 2) hipLaunchKernelGGL((fvp_kernel<ACT, 2>), g, b, 0, s, a);
  else if (nin <= 4) hipLaunchKernelGGL((fvp_kernel<ACT, 4>), g, b, 0, s, a);
  else if (nin <= 8) hipLaunchKernelGGL((fvp_kernel<ACT, 8>), g, b, 0, s, a);
  else hipLaunchKernelGGL((fvp_kernel<ACT, 12>), g, b, 0, s, a);
}
template <int ACT>
static void launch_surrogate(int nin, dim3 g, hipStream_t s, const NpgArgs &a) {
  const dim3 b(kWideWaves * 64);
  if (nin <= 2) hipLaunchKernelGGL((surrogate_kernel<ACT, 2>), g, b, 0, s, a);
  else if (nin <= 4) hipLaunchKernelGGL((surrogate_kernel<ACT, 4>), g, b, 0, s, a);
  else if (nin <= 8) hipLaunchKernelGGL((surrogate_kernel<ACT, 8>), g, b, 0, s, a);
  else hipLaunchKernelGGL((surrogate_kernel<ACT, 12>), g, b, 0, s, a);
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int64_t pds_npg_workspace_floats(const pds_mlp *m, int num_candidates) {
  if (check(m) != PDS_OK || num_candidates < 0) return PDS_EINVAL;
  const int64_t waves = (int64_t)kWideMaxBlocks * kWideWaves;
  const int64_t fvp = waves * offsets(*m).total, ls = waves * 3 * (int64_t)num_candidates;
  return fvp > ls ? fvp : ls;
}

extern "C" int pds_npg_fisher_vector_product(const pds_mlp *m, const float *d_x, const int64_t *d_index, int64_t B,
                                             const float *d_log_std, const float *d_v, float damping, float *d_out,
                                             float *d_workspace, void *stream) {
  if (check(m) != PDS_OK || !d_x || !d_log_std || !d_v || !d_out || !d_workspace || B < 1) return PDS_EINVAL;
  NpgArgs a{};
  a.m = *m; a.x = d_x; a.index = d_index; a.B = B; a.log_std = d_log_std; a.v = d_v; a.partials = d_workspace;
  const Offsets o = offsets(*m);
  a.pstride = o.total;
  const int blocks = wide_grid_blocks(B), nin = (m->d_in + kTW - 1) / kTW;
  hipStream_t s = (hipStream_t)stream;
  if (m->activation == 0) launch_fvp<0>(nin, dim3(blocks), s, a); else launch_fvp<1>(nin, dim3(blocks), s, a);
  const float scale = 1.0f / (float)((double)B * (double)m->d_out);
  npg_reduce_fvp(s, d_workspace, a.pstride, blocks * kWideWaves, o.total, scale, damping, d_v, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_npg_cg_step(int64_t n, float *d_x, float *d_r, float *d_p, const float *d_z, float *d_state, float eps,
                               float residual_tol, int init, void *stream) {
  if (n < 1 || !d_x || !d_r || !d_p || !d_z || !d_state) return PDS_EINVAL;
  hipLaunchKernelGGL(cg_kernel, dim3(1), dim3(kCgThreads), 0, (hipStream_t)stream, (long long)n, d_x, d_r, d_p, d_z, d_state,
                     eps, residual_tol, init);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_npg_surrogate_kl(const pds_mlp *m, const float *d_step, const float *d_fracs, int num_candidates,
                                    const float *d_x, const float *d_act, const float *d_adv, const float *d_logp_old,
                                    const float *d_mu_old, const float *d_log_std, int64_t B, float *d_out, float *d_theta_out,
                                    float *d_workspace, void *stream) {
  if (check(m) != PDS_OK || !d_step || !d_fracs || num_candidates < 1 || num_candidates > 65535 || !d_x || !d_act ||
      !d_adv || !d_logp_old || !d_mu_old || !d_log_std || !d_out || !d_workspace || B < 1)
    return PDS_EINVAL;
  NpgArgs a{};
  a.m = *m; a.x = d_x; a.B = B; a.log_std = d_log_std; a.v = d_step; a.fracs = d_fracs; a.act = d_act; a.adv = d_adv;
  a.logp_old = d_logp_old; a.mu_old = d_mu_old; a.partials = d_workspace; a.theta_out = d_theta_out;
  const int blocks = wide_grid_blocks(B), nin = (m->d_in + kTW - 1) / kTW;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(blocks, num_candidates);
  if (m->activation == 0) launch_surrogate<0>(nin, g, s, a); else launch_surrogate<1>(nin, g, s, a);
  npg_reduce_surrogate(s, d_workspace, blocks * kWideWaves, num_candidates, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}