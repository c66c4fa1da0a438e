// pds_npg_deep.hip -- the natural-gradient policy step of NPG and TRPO for actors with THREE or FOUR hidden layers
// (include/pds_npg_deep.h): the Fisher-vector product and the evaluation of the line-search candidates for struct pds_mlp_deep.
// The conjugate-gradient iteration (cg_kernel of csrc/pds_npg.hip) takes only a length and is used as it is.
//
// Who needs it: the reference's architecture search (experiments/01_find_NN_architecture) trains its (50, 30, 20) and
// (32, 32, 32, 32) actors with --alg trpo.
//
// The two kernels are fvp_kernel and surrogate_kernel of csrc/pds_npg.hip (read its header first: the Gauss-Newton form
// F v = 1 / (B A) sum_i J_i^T diag(exp(-2 log_std)) J_i v, the candidates theta + f s formed while the weights are staged) on the
// tile core of csrc/pds_mlp_deep_tile.h, down L hidden layers (L a template parameter, every layer loop unrolled):
//   tangent   per hidden layer l = 1 .. L:  z = W_l h_(l-1),  dz = W_l t_(l-1) + V_l h_(l-1) + vb_l  (h_0 = x, t_0 = 0: layer 1 is
//             V_1 x + vb_1),  h_l = act(z + b_l),  t_l = act'(h_l) dz;   output  dmu = W_o t_L + V_o h_L + vb_o
//   scale     u = dmu exp(-2 log_std), zero outside the batch and the outputs
//   backward  deep_backward<ACT, L> from u into DeepGrads<L>, as the PPO gradient's
// The tangent's weights V are read from global memory with bounds (gemm_glb, L2-resident: at most 21 k floats); h and t stay in
// registers from layer to layer (two live sets of 16 registers each, beside the 64 L + 16 + 4 L + 4 accumulators: 292 at L = 4,
// one wave per SIMD).  LDS is the budget of mlp_deep_kernel's gradient forms (header of csrc/pds_mlp_deep.hip): L + 1 images and
// dY per wave beside the weight images, four waves per block at L = 3 and THREE at L = 4.  The rows are already standardised
// (the trainer's batch), so there is no mean / std here; the optional index gathers rows as in pds_npg_fisher_vector_product.
// The candidate kernel holds no images and runs four waves at both depths; its forward chain is deep_forward, the function
// pds_mlp_deep_forward runs.
#include "pds_mlp_deep_tile.h"
#include "pds_npg_tile.h"

#include "../../include/pds_npg_deep.h"

namespace pds_mlp_detail {

constexpr int kNpgDeepMaxBlocks = 256;  // one persistent block per CU
constexpr int kNpgDeepMaxWaves = 4;
template <int L>
constexpr int fvp_deep_waves() { return L == 4 ? 3 : kNpgDeepMaxWaves; }

// A layer's widths as values the compiler must take anew in every tile: the offsets and bounds of the tangent's global loads (16 per
// output tile, 64 L + 16 per sample tile) depend on nothing else, so all of them would be formed once in front of the tile loop and
// kept -- more registers than are left beside the accumulators (without this the L = 4 kernel spilled 52 VGPRs)
#define PDS_PER_TILE(x) asm volatile("" : "+s"(x))

struct NpgDeepArgs {
  pds_mlp_deep m;
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

template <int ACT, int L>
__global__ __launch_bounds__((fvp_deep_waves<L>() * 64), 1) void fvp_deep_kernel(const NpgDeepArgs a) {
  constexpr int kW = fvp_deep_waves<L>(), kThreads = kW * 64;
  constexpr int kI = kTS * kS;
  constexpr int kImg = (L + 1) * kI + kTS * kSY;  // X, H1 .. HL, U per wave
  __shared__ __attribute__((aligned(16))) float Ws[L * kMaxDim * kS];  // per hidden layer [out][in], zero padded
  __shared__ __attribute__((aligned(16))) float Wos[kMaxOut * kS];
  __shared__ __attribute__((aligned(16))) float bs[L * kMaxDim], bos[kTW], isg2[kTW];
  __shared__ __attribute__((aligned(16))) float images[kW * kImg];
  const pds_mlp_deep &m = a.m;
  const DeepOffsets o = deep_offsets(m);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;  // C/D layout: column (sample) n, rows 4 g + q
  deep_stage<L, kThreads>(m, Ws, Wos, bs, bos, tid, [](float t, int) { return t; });
  if (tid < kTW) {
    const float is = tid < m.d_out ? expf(-a.log_std[tid]) : 0.f;  // 1 / sigma
    isg2[tid] = is * is;
  }
  float *img = images + wave * kImg;  // [sample][feature] images for the weight-gradient GEMMs
  for (int i = lane; i < kImg; i += 64) img[i] = 0.f;
  __syncthreads();

  DeepGrads<L> G;
  G.zero();

  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kW + wave, nw = (long long)gridDim.x * kW;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long s0 = t * kTS;
    long long row = -1;  // source row of this lane's sample, -1: none
    if (s0 + n < a.B) row = a.index != nullptr ? a.index[s0 + n] : s0 + n;
    const bool valid = row >= 0;
    // ---- input: lane (n, g) holds features 16 kt + 4 g + q of its sample = the B operands of layer 1 ----
    f32x4 hr[kNT], tr[kNT];
#pragma unroll
    for (int kt = 0; kt < kNT; ++kt) {
      f32x4 xv;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kt * kTW + 4 * g + q;
        xv[q] = (valid && k < m.d_in) ? a.x[row * m.d_in + k] : 0.f;
      }
      sts4(img + n * kS + kt * kTW + 4 * g, xv);
      hr[kt] = xv;
      tr[kt] = (f32x4)(0.f);
    }
    // ---- hidden layer l + 1: h = act(W h + b), its tangent t = act'(h) (W t + V h + vb); t_0 = 0 is not multiplied ----
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const float *Wl = Ws + l * kMaxDim * kS;
      const float *Vl = a.v + o.w[l], *vbl = a.v + o.b[l];
      int rows = m.hidden[l], cols = l == 0 ? m.d_in : m.hidden[l > 0 ? l - 1 : 0];
      PDS_PER_TILE(rows); PDS_PER_TILE(cols);
      f32x4 hn[kNT], tn[kNT];
#pragma unroll
      for (int it = 0; it < kNT; ++it) {
        const f32x4 z = gemm_lds<kNT, kS>(Wl, it, hr, n, g, (f32x4)(0.f));
        f32x4 dz = (f32x4)(0.f);
        if (l > 0) dz = gemm_lds<kNT, kS>(Wl, it, tr, n, g, dz);
        dz = gemm_glb<kNT>(Vl, rows, cols, it, hr, n, g, dz);
        const f32x4 b = lds4(bs + l * kMaxDim + it * kTW + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = it * kTW + 4 * g + q;
          hn[it][q] = act_fn<ACT>(z[q] + b[q]);
          tn[it][q] = act_grad<ACT>(hn[it][q]) * (dz[q] + (i < rows ? vbl[i] : 0.f));
        }
        sts4(img + (l + 1) * kI + n * kS + it * kTW + 4 * g, hn[it]);
      }
#pragma unroll
      for (int it = 0; it < kNT; ++it) { hr[it] = hn[it]; tr[it] = tn[it]; }
    }
    // ---- output tangent dmu = W_o t_L + V_o h_L + vb_o, u = dmu / sigma^2 (zero outside the batch and the outputs) ----
    f32x4 u;
    {
      const float *Vo = a.v + o.w[L], *vbo = a.v + o.b[L];
      int rows = m.d_out, cols = m.hidden[L - 1];
      PDS_PER_TILE(rows); PDS_PER_TILE(cols);
      f32x4 dm = gemm_lds<kNT, kS>(Wos, 0, tr, n & (kMaxOut - 1), g, (f32x4)(0.f));
      dm = gemm_glb<kNT>(Vo, rows, cols, 0, hr, n, g, dm);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * g + q;
        u[q] = (valid && j < m.d_out) ? (dm[q] + vbo[j]) * isg2[j] : 0.f;
      }
    }
    deep_backward<ACT, L>(Ws, Wos, img, u, G, n, g);
  }

  // ---- this wave's partial -> partials[wave of the grid][flat parameter layout] (a wave without a tile writes zeros) ----
  G.store(m, o, a.partials + wid * a.pstride, n, g);
}

// ---- line-search candidates: sum(ratio adv) and sum KL(p_old || q) per candidate (surrogate_kernel of csrc/pds_npg.hip) ----
template <int ACT, int L>
__global__ __launch_bounds__(kNpgDeepMaxWaves * 64, 1) void surrogate_deep_kernel(const NpgDeepArgs a) {
  constexpr int kW = kNpgDeepMaxWaves, kThreads = kW * 64;
  __shared__ __attribute__((aligned(16))) float Ws[L * kMaxDim * kS];
  __shared__ __attribute__((aligned(16))) float Wos[kMaxOut * kS];
  __shared__ __attribute__((aligned(16))) float bs[L * kMaxDim], bos[kTW], lsg[kTW], sgg[kTW], vrg[kTW];
  const pds_mlp_deep &m = a.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int cj = blockIdx.y;
  const float f = a.fracs[cj];
  // the candidate's parameters theta + f s are formed while the weights are staged
  deep_stage<L, kThreads>(m, Ws, Wos, bs, bos, tid, [&](float t, int i) { return cand(t, f, a.v[i]); });
  if (tid < kTW) {
    const float ls = tid < m.d_out ? a.log_std[tid] : 0.f;
    const float sg = expf(ls);
    lsg[tid] = ls; sgg[tid] = sg; vrg[tid] = sg * sg;
  }
  if (a.theta_out != nullptr && blockIdx.x == 0) {
    const int total = deep_offsets(m).total;
    for (int i = tid; i < total; i += kThreads) a.theta_out[(long long)cj * total + i] = cand(*deep_param_ptr(m, i), f, a.v[i]);
  }
  __syncthreads();

  float st_ra = 0.f, st_kl = 0.f, st_r = 0.f;
  const long long ntiles = (a.B + kTS - 1) / kTS;
  const long long wid = (long long)blockIdx.x * kW + wave, nw = (long long)gridDim.x * kW;
  for (long long t = wid; t < ntiles; t += nw) {
    const long long smp = t * kTS + n;
    const bool valid = smp < a.B;
    f32x4 cur[kNT];
#pragma unroll
    for (int kt = 0; kt < kNT; ++kt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kt * kTW + 4 * g + q;
        cur[kt][q] = (valid && k < m.d_in) ? a.x[smp * m.d_in + k] : 0.f;
      }
    const f32x4 y = deep_forward<ACT, L, false>(Ws, Wos, bs, bos, cur, nullptr, n, g);
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

// blocks of `waves` waves, one 16-sample tile per wave and round
static int npg_deep_grid_blocks(long long B, int waves) {
  const long long tiles = (B + kTS - 1) / kTS;
  const long long blocks = (tiles + waves - 1) / waves;
  return (int)(blocks < kNpgDeepMaxBlocks ? blocks : kNpgDeepMaxBlocks);
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int64_t pds_npg_deep_workspace_floats(const pds_mlp_deep *m, int num_candidates) {
  if (deep_check(m) != PDS_OK || num_candidates < 0) return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  const int64_t waves = (int64_t)kNpgDeepMaxBlocks * kNpgDeepMaxWaves;  // one partial per WAVE of the largest grid
  const int64_t fvp = waves * deep_offsets(*m).total, ls = waves * 3 * (int64_t)num_candidates;
  return fvp > ls ? fvp : ls;
}

extern "C" int pds_npg_deep_fisher_vector_product(const pds_mlp_deep *m, const float *d_x, const int64_t *d_index, int64_t B,
                                                  const float *d_log_std, const float *d_v, float damping, float *d_out,
                                                  float *d_workspace, void *stream) {
  if (deep_check(m) != PDS_OK || !d_x || !d_log_std || !d_v || !d_out || !d_workspace || B < 1) return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  NpgDeepArgs a{};
  a.m = *m; a.x = d_x; a.index = d_index; a.B = B; a.log_std = d_log_std; a.v = d_v; a.partials = d_workspace;
  const int total = deep_offsets(*m).total;
  a.pstride = total;
  const int waves = m->n_hidden == 4 ? fvp_deep_waves<4>() : fvp_deep_waves<3>();
  const dim3 g(npg_deep_grid_blocks(B, waves)), b(waves * 64);
  hipStream_t s = (hipStream_t)stream;
  if (m->n_hidden == 3) {
    if (m->activation == 0) hipLaunchKernelGGL((fvp_deep_kernel<0, 3>), g, b, 0, s, a);
    else hipLaunchKernelGGL((fvp_deep_kernel<1, 3>), g, b, 0, s, a);
  } else {
    if (m->activation == 0) hipLaunchKernelGGL((fvp_deep_kernel<0, 4>), g, b, 0, s, a);
    else hipLaunchKernelGGL((fvp_deep_kernel<1, 4>), g, b, 0, s, a);
  }
  const float scale = 1.0f / (float)((double)B * (double)m->d_out);
  npg_reduce_fvp(s, d_workspace, a.pstride, (int)g.x * waves, total, scale, damping, d_v, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_npg_deep_surrogate_kl(const pds_mlp_deep *m, const float *d_step, const float *d_fracs, int num_candidates,
                                         const float *d_x, const float *d_act, const float *d_adv, const float *d_logp_old,
                                         const float *d_mu_old, const float *d_log_std, int64_t B, float *d_out,
                                         float *d_theta_out, float *d_workspace, void *stream) {
  if (deep_check(m) != PDS_OK || !d_step || !d_fracs || num_candidates < 1 || num_candidates > 65535 || !d_x || !d_act ||
      !d_adv || !d_logp_old || !d_mu_old || !d_log_std || !d_out || !d_workspace || B < 1)
    return PDS_EINVAL;
  if (m->d_in > kMaxDim) return PDS_EUNSUPPORTED;
  NpgDeepArgs a{};
  a.m = *m; a.x = d_x; a.B = B; a.log_std = d_log_std; a.v = d_step; a.fracs = d_fracs; a.act = d_act; a.adv = d_adv;
  a.logp_old = d_logp_old; a.mu_old = d_mu_old; a.partials = d_workspace; a.theta_out = d_theta_out;
  const int blocks = npg_deep_grid_blocks(B, kNpgDeepMaxWaves);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(blocks, num_candidates), b(kNpgDeepMaxWaves * 64);
  if (m->n_hidden == 3) {
    if (m->activation == 0) hipLaunchKernelGGL((surrogate_deep_kernel<0, 3>), g, b, 0, s, a);
    else hipLaunchKernelGGL((surrogate_deep_kernel<1, 3>), g, b, 0, s, a);
  } else {
    if (m->activation == 0) hipLaunchKernelGGL((surrogate_deep_kernel<0, 4>), g, b, 0, s, a);
    else hipLaunchKernelGGL((surrogate_deep_kernel<1, 4>), g, b, 0, s, a);
  }
  npg_reduce_surrogate(s, d_workspace, blocks * kNpgDeepMaxWaves, num_candidates, d_out);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
