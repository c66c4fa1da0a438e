// pds_explore.h -- the two exploration rules of the off-policy trainers as device functions, stated once for the elementwise
// entry points (pds_sac_sample in csrc/pds_sac.hip, pds_ddpg_explore in csrc/pds_ddpg.hip), the SAC update kernels and the
// network waves of the fused collection (csrc/pds_collect.h): same source, same instructions, same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pds_device.h"

namespace pds_explore {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kLogStdMin = -20.f, kLogStdMax = 2.f;  // LOG_STD_MIN / LOG_STD_MAX, algs/sac/sac.py:31-32

// softplus(x) = log(1 + e^x) in its stable form
__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// The squashed-Gaussian sample of one row, stated once for the three kernels (SquashedGaussianMLPActor.forward,
// algs/sac/sac.py:47-76): ls = clamp(log_std), sig = exp(ls), u = mu + sig eps, th = tanh(u) and
// logp = sum_j (-0.5 eps_j^2 - ls_j - 0.5 log 2 pi) - sum_j 2 (log 2 - u_j - softplus(-2 u_j)).
// eps: the noise contract; deterministic: eps = 0 (u = mu).
struct SacDraw {
  f32x4 eps, ls, sig, u, th;
  float logp;
};
// The four standard normals pds_gaussian_sample draws for sample `id`, block 0, in `call` under `seed`.
__device__ __forceinline__ f32x4 gaussian_draw4(unsigned long long id, unsigned long long call, unsigned long long seed) {
  const pds::U4 r = PDS_GAUSSIAN_PHILOX(id, 0u, call, seed);
  float z0, z1, z2, z3;
  pds::box_muller(r.x, r.y, z0, z1);
  pds::box_muller(r.z, r.w, z2, z3);
  return (f32x4){z0, z1, z2, z3};
}

// (sac_squash: the sample at a GIVEN eps -- the network waves of csrc/pds_collect.h draw eps while the env wave steps)
__device__ __forceinline__ SacDraw sac_squash(const f32x4 mu, const f32x4 log_std, const f32x4 eps) {
  SacDraw d;
  d.eps = eps;
  float gauss = 0.f, corr = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    d.ls[j] = fminf(fmaxf(log_std[j], kLogStdMin), kLogStdMax);
    d.sig[j] = expf(d.ls[j]);
    d.u[j] = fmaf(d.sig[j], d.eps[j], mu[j]);
    d.th[j] = tanhf(d.u[j]);
    gauss += PDS_GAUSSIAN_LOGP_TERM(d.eps[j], d.ls[j]);
    corr += 2.f * (0.69314718055994530942f - d.u[j] - softplus(-2.f * d.u[j]));
  }
  d.logp = gauss - corr;
  return d;
}
__device__ __forceinline__ SacDraw sac_draw(const f32x4 mu, const f32x4 log_std, unsigned long long id, unsigned long long call,
                                            unsigned long long seed, bool deterministic) {
  return sac_squash(mu, log_std, deterministic ? (f32x4)(0.f) : gaussian_draw4(id, call, seed));
}

// DDPG's exploration action (get_action, algs/ddpg/ddpg.py:342-345) from the actor's pre-activation output `net`:
// a = clamp(fma(exp(log_std), z, act_limit tanh(net)), +-act_limit).  The product is rounded before the fma.
__device__ __forceinline__ f32x4 ddpg_explore(const f32x4 net, const f32x4 log_std, const f32x4 z, float limit) {
  f32x4 a;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float m = __fmul_rn(limit, tanhf(net[j]));
    a[j] = fminf(fmaxf(fmaf(expf(log_std[j]), z[j], m), -limit), limit);
  }
  return a;
}

}  // namespace pds_explore
