// pds_ddpg_broad.hip -- DDPG's deterministic policy gradient, Bellman backup and polyak step (algs/ddpg/ddpg.py:316-340, 431-464)
// for actor and Q networks with a hidden width ABOVE 64 (include/pds_mlp_broad.h), e.g. the reference's default (400, 300).
//
// Built from the pieces of csrc/pds_mlp_broad_tile.h on the design of csrc/pds_mlp_broad.hip (read its header first): the weights
// of BOTH networks stay in global memory / L2, a chain block of 8 waves owns 16 (from B = 512 on: 32) samples and runs, in ONE
// launch (ddpg_broad_chain_kernel),
//   1  the actor's forward on the first D columns of the replay row [obs | act]     broad_load_x, broad_layer x 3
//   2  a = act_limit tanh(mu) into columns D .. D + 3 of the X image                (tanhf; the stored action is never read)
//   3  Q's forward on [obs | a], over the SAME two hidden images                    broad_layer x 3
//      -- the target form ends here: target[row] = rew + gamma (1 - done) Q
//   4  dZ2q, dZ1q from dQ = -1 in place, da = W1q[:, D : D + 4]^T dZ1q              broad_back x 2, broad_gemm (one tile, wave 0)
//   5  dmu = da act_limit (1 - tanh^2)
//   6  the actor's dZ2, dZ1 from dmu                                                broad_back x 2
// The actor's H1 and H2 went to the workspace in step 1 (the weight-gradient kernel needs them anyway) and Q overwrote their
// images, so step 6 reads act'(H) back from there: written and read by the same block on either side of a __syncthreads().
// Q's parameters are only read; nothing of Q goes to the workspace.  The actor's weight gradients, the sum in a fixed order, 1 / B
// and the Adam step are broad_grad_finish's (csrc/pds_mlp_broad.hip): three launches for the policy gradient, one for the target.
// A zero in every action column of W1q makes da, dmu, dZ and with them every weight gradient exactly zero.
#include "pds_mlp_broad_tile.h"

namespace pds_mlp_detail {

struct DdpgBroadArgs {
  pds_mlp pi, q;
  const float *x;        // [rows, ldx]: the first D columns are the observation
  int ldx;
  const int64_t *index;
  long long B;
  float limit;
  const float *rew, *done;  // the target form
  float gamma;
  float *target;
  BroadWs ws;               // the gradient form: the ACTOR's workspace
};

template <int NS, bool GRAD>
__global__ __launch_bounds__(kBroadThreads) void ddpg_broad_chain_kernel(const DdpgBroadArgs a) {
  __shared__ __attribute__((aligned(16))) BroadLds<NS> L;
  __shared__ float TH[NS * kTS * 4];  // tanh(mu)
  const pds_mlp &P = a.pi, &Q = a.q;
  const int tid = threadIdx.x, D = P.d_in;
  const long long s0 = (long long)blockIdx.x * (NS * kTS);
  broad_load_x<NS>(a.x, a.ldx, D, a.index, s0, a.B, nullptr, nullptr, 0.f, L.X, GRAD ? a.ws.x : nullptr);
  __syncthreads();
  broad_layer<NS>(P.w1, P.b1, P.h1, D, P.activation, L.X, kS, L.H1, kBS, GRAD ? a.ws.h1 : nullptr, s0, a.B);
  __syncthreads();
  broad_layer<NS>(P.w2, P.b2, P.h2, P.h1, P.activation, L.H1, kBS, L.H2, kBS, GRAD ? a.ws.h2 : nullptr, s0, a.B);
  __syncthreads();
  broad_layer<NS>(P.w3, P.b3, 4, P.h2, -1, L.H2, kBS, L.Y, kSY, nullptr, s0, a.B);
  __syncthreads();
  if (tid < NS * kTS * 4) {
    const int sl = tid >> 2, c = tid & 3;
    const float th = tanhf(L.Y[sl * kSY + c]);
    TH[tid] = th;
    L.X[sl * kS + D + c] = a.limit * th;
  }
  __syncthreads();
  broad_layer<NS>(Q.w1, Q.b1, Q.h1, D + 4, Q.activation, L.X, kS, L.H1, kBS, nullptr, s0, a.B);
  __syncthreads();
  broad_layer<NS>(Q.w2, Q.b2, Q.h2, Q.h1, Q.activation, L.H1, kBS, L.H2, kBS, nullptr, s0, a.B);
  __syncthreads();
  broad_layer<NS>(Q.w3, Q.b3, 1, Q.h2, -1, L.H2, kBS, L.Y, kSY, nullptr, s0, a.B);
  __syncthreads();
  if constexpr (!GRAD) {
    // every product and the sum rounded separately (torch's `r + gamma * (1 - d) * v`), as bellman_write of pds_actor_critic.h
    if (tid < NS * kTS && s0 + tid < a.B) {
      const long long row = a.index != nullptr ? a.index[s0 + tid] : s0 + tid;
      a.target[row] = __fadd_rn(a.rew[row], __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.f, a.done[row])), L.Y[tid * kSY]));
    }
  } else {
    // the loss SUM -sum Q: dQ = -1 per sample (the reduce scales by 1 / B); statistics: sum Q, count
    if (tid < NS * kTS) {
      const bool valid = s0 + tid < a.B;
      L.red[tid][0] = valid ? L.Y[tid * kSY] : 0.f;
      L.red[tid][1] = valid ? 1.f : 0.f;
      L.Y[tid * kSY] = valid ? -1.f : 0.f;
    }
    __syncthreads();
    broad_block_stats<NS>(L, a.ws.stat);
    broad_back<NS>(Q.w3, Q.h2, Q.h2, 1, Q.activation, L.Y, kSY, L.H2, nullptr, nullptr, s0, a.B);
    __syncthreads();
    broad_back<NS>(Q.w2, Q.h1, Q.h1, Q.h2, Q.activation, L.H2, kBS, L.H1, nullptr, nullptr, s0, a.B);
    __syncthreads();
    if (tid < 64) {  // da^T = W1q[:, D : D + 4]^T dZ1q^T: rows 0 .. 3 of one output tile, in lane group 0
      const int n = tid & 15, g = tid >> 4;
      f32x4 da[NS];
#pragma unroll
      for (int ns = 0; ns < NS; ++ns) da[ns] = (f32x4)(0.f);
      broad_gemm<NS, true>(Q.w1 + D, D + 4, 4, Q.h1, 0, L.H1, kBS, da, n, g);
      if (g == 0) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
          const int sl = ns * kTS + n;
          const bool valid = s0 + sl < a.B;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float th = TH[sl * 4 + c];
            const float dmu = valid ? da[ns][c] * a.limit * (1.f - th * th) : 0.f;
            L.Y[sl * kSY + c] = dmu;  // (columns 4 .. 15 are zero since Q's output layer wrote them)
            if (valid) a.ws.dy[(s0 + sl) * 4 + c] = dmu;
          }
        }
      }
    }
    __syncthreads();
    broad_back<NS>(P.w3, P.h2, P.h2, 4, P.activation, L.Y, kSY, L.H2, a.ws.h2, a.ws.dz2, s0, a.B);
    __syncthreads();
    broad_back<NS>(P.w2, P.h1, P.h1, P.h2, P.activation, L.H2, kBS, L.H1, a.ws.h1, a.ws.dz1, s0, a.B);
  }
}

// t = rn(rn(rho t) + rn(omr s)) over the six tensors of a network (polyak_kernel of csrc/pds_ddpg.hip)
__global__ __launch_bounds__(256) void polyak_broad_kernel(pds_mlp t, pds_mlp s, int total, float rho, float omr) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const Offsets o = offsets(t);
  float *dst;
  const float *src;
  at_param(o, p, [&](const float *pds_mlp::*w, int i) { dst = const_cast<float *>(t.*w) + i; src = s.*w + i; });
  *dst = __fadd_rn(__fmul_rn(rho, *dst), __fmul_rn(omr, *src));
}

// PDS_OK, PDS_EINVAL (a network outside the range, the actor's d_out not 4, Q d_out != 1, Q d_in != D + 4) or PDS_EUNSUPPORTED
// (D + 4 > 64)
static int ddpg_broad_check(const pds_mlp *pi, const pds_mlp *q) {
  if (broad_check(pi) != PDS_OK || broad_check(q) != PDS_OK || pi->d_out != 4 || q->d_out != 1 || q->d_in != pi->d_in + 4)
    return PDS_EINVAL;
  return q->d_in <= kMaxDim ? PDS_OK : PDS_EUNSUPPORTED;
}

template <bool GRAD>
static int ddpg_broad_launch(const DdpgBroadArgs &a, hipStream_t s) {  // -> blocks of the grid
  const int ns = broad_tiles_per_block(a.B);
  const int blocks = (int)((a.B + ns * kTS - 1) / (ns * kTS));
  if (ns == 1) hipLaunchKernelGGL((ddpg_broad_chain_kernel<1, GRAD>), dim3(blocks), dim3(kBroadThreads), 0, s, a);
  else hipLaunchKernelGGL((ddpg_broad_chain_kernel<2, GRAD>), dim3(blocks), dim3(kBroadThreads), 0, s, a);
  return blocks;
}

}  // namespace pds_mlp_detail
using namespace pds_mlp_detail;

extern "C" int pds_ddpg_broad_supported(const pds_mlp *pi, const pds_mlp *q) { return ddpg_broad_check(pi, q) == PDS_OK ? 1 : 0; }

extern "C" int64_t pds_ddpg_broad_workspace_floats(const pds_mlp *pi, const pds_mlp *q) {
  const int rc = ddpg_broad_check(pi, q);
  if (rc != PDS_OK) return rc;
  return broad_ws_floats(*pi, kBroadMaxBatch);
}

extern "C" int pds_ddpg_broad_policy_grad(const pds_mlp *pi, const pds_mlp *q, const float *d_oa, const int64_t *d_index, int64_t B,
                                          float act_limit, float *d_grads, float *d_stats, float *d_workspace, const pds_adam *opt,
                                          void *stream) {
  if (!pi || !q || !d_oa || !d_grads || !d_stats || !d_workspace || B < 1 || !adam_ok(opt)) return PDS_EINVAL;
  const int rc = ddpg_broad_check(pi, q);
  if (rc != PDS_OK) return rc;
  if (B > kBroadMaxBatch) return PDS_EUNSUPPORTED;
  DdpgBroadArgs a{};
  a.pi = *pi; a.q = *q; a.x = d_oa; a.ldx = q->d_in; a.index = d_index; a.B = B; a.limit = act_limit;
  a.ws = broad_ws(d_workspace, *pi, B);
  const int blocks = ddpg_broad_launch<true>(a, (hipStream_t)stream);
  return broad_grad_finish(*pi, a.ws, B, blocks, d_grads, d_stats, opt, (hipStream_t)stream);
}

extern "C" int pds_ddpg_broad_target(const pds_mlp *pi_targ, const pds_mlp *q_targ, const float *d_obs2, const int64_t *d_index,
                                     int64_t B, const float *d_rew, const float *d_done, float gamma, float act_limit,
                                     float *d_target_rows, void *stream) {
  if (!pi_targ || !q_targ || !d_obs2 || !d_rew || !d_done || !d_target_rows || B < 1) return PDS_EINVAL;
  const int rc = ddpg_broad_check(pi_targ, q_targ);
  if (rc != PDS_OK) return rc;
  DdpgBroadArgs a{};
  a.pi = *pi_targ; a.q = *q_targ; a.x = d_obs2; a.ldx = pi_targ->d_in; a.index = d_index; a.B = B; a.limit = act_limit;
  a.rew = d_rew; a.done = d_done; a.gamma = gamma; a.target = d_target_rows;
  ddpg_broad_launch<false>(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_polyak_broad(const pds_mlp *targ, const pds_mlp *src, double polyak, void *stream) {
  if (broad_check(targ) != PDS_OK || broad_check(src) != PDS_OK || targ->d_in != src->d_in || targ->h1 != src->h1 ||
      targ->h2 != src->h2 || targ->d_out != src->d_out || !(polyak >= 0.0 && polyak <= 1.0))
    return PDS_EINVAL;
  const int total = offsets(*targ).total;
  hipLaunchKernelGGL(polyak_broad_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, *targ, *src, total,
                     (float)polyak, (float)(1.0 - polyak));
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
