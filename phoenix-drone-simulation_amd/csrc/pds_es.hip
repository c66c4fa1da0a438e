// pds_es.hip -- the two device pieces of an evolution strategy over actor weights (es.py ESTrainer):
//   pds_es_perturb    theta[2 i] = mu + sigma eps_i, theta[2 i + 1] = mu - sigma eps_i for the antithetic pairs i
//   pds_es_gradient   scale sum_i w_i eps_i + l2 mu, with eps REGENERATED from its counters (never stored, never read back)
// The noise contract: element j = 8 q + r of eps_i is variate r (of d_out = 8) that pds_gaussian_sample
// (csrc/pds_train.hip sample_kernel) draws for sample id i * Q + q, Q = ceil(n / 8), in call `generation` under `seed`.
// One lane works on 4 consecutive parameters of one pair: one Philox4x32-10 block, two Box-Muller pairs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pds.h"
#include "pds_device.h"

#define PDS_ES_CHUNK 32  // pairs per partial slab of pds_es_gradient

namespace pds_es_detail {  // named (not anonymous) so that profiler kernel names are readable

// eps_pair[4 b4 .. 4 b4 + 3]: block b4 & 1 of sample id pair * Q + (b4 >> 1)
PDS_DEV void noise4(unsigned long long pair, long long b4, unsigned long long Q, uint64_t generation, uint64_t seed, float z[4]) {
  const unsigned long long id = pair * Q + (unsigned long long)(b4 >> 1);
  const pds::U4 r = PDS_GAUSSIAN_PHILOX(id, (uint32_t)(b4 & 1), generation, seed);
  pds::box_muller(r.x, r.y, z[0], z[1]);
  pds::box_muller(r.z, r.w, z[2], z[3]);
}

// v[0 .. valid) -> p[0 .. valid) with the widest stores the address allows.  ALIGNED (n % 4 == 0: every row starts on 16 bytes and
// no block is partial): one dwordx4.  Otherwise the lane looks at its own address: dwordx4, two dwordx2 or four dwords for a full
// block (the lanes of a wave still cover one contiguous span), dwords for the partial block that ends a row.
// (vector types, not float4 / float2: a struct store is taken apart into scalar stores before the branches are merged, and the
// common tails of the three cases are then sunk into dword stores)
typedef float v2f __attribute__((ext_vector_type(2)));
template <bool ALIGNED>
PDS_DEV void store4(float *p, const float v[4], int valid) {
  const pds::pds_v4f q = {v[0], v[1], v[2], v[3]};
  if (ALIGNED) {
    *reinterpret_cast<pds::pds_v4f *>(p) = q;
    return;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (valid == 4 && (a & 15) == 0) {
    *reinterpret_cast<pds::pds_v4f *>(p) = q;
  } else if (valid == 4 && (a & 7) == 0) {
    *reinterpret_cast<v2f *>(p) = q.xy;
    *reinterpret_cast<v2f *>(p + 2) = q.zw;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < valid) p[k] = v[k];
  }
}

// work item w = pair * B4 + b4 (B4 = ceil(n / 4) blocks per row): consecutive lanes take consecutive blocks of one row, so the
// stores of a wave are contiguous along n.  The grid strides over the items; (pair, b4) advance by the stride's quotient and
// remainder instead of a division per item.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void perturb_kernel(const float *__restrict__ mu, long long n, long long pairs, float sigma,
                                                      uint64_t seed, uint64_t generation, unsigned long long pair_base,
                                                      float *__restrict__ theta) {
  const long long B4 = (n + 3) >> 2;
  const unsigned long long Q = (unsigned long long)((n + 7) >> 3);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long sq = stride / B4, sr = stride % B4;  // (the same for every lane)
  const long long w0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long pair = w0 / B4, b4 = w0 % B4;
  while (pair < pairs) {
    float z[4];
    noise4(pair_base + (unsigned long long)pair, b4, Q, generation, seed, z);
    const long long j = b4 << 2;
    const int valid = ALIGNED ? 4 : (int)(n - j < 4 ? n - j : 4);
    float m[4], plus[4], minus[4];
    if (ALIGNED) {
      const float4 t = *reinterpret_cast<const float4 *>(mu + j);
      m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = k < valid ? mu[j + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      plus[k] = fmaf(sigma, z[k], m[k]);
      minus[k] = fmaf(-sigma, z[k], m[k]);
    }
    float *row = theta + 2 * pair * n + j;
    store4<ALIGNED>(row, plus, valid);
    store4<ALIGNED>(row + n, minus, valid);
    pair += sq; b4 += sr;
    if (b4 >= B4) { b4 -= B4; ++pair; }
  }
}

// slab[c][j] = sum over the pairs k of chunk c, in the order k = 0, 1, ..: w[k] eps_k[j].  One WAVE takes 64 consecutive blocks of
// one chunk, so the chunk -- and with it every load of a pair weight -- is wave-uniform, and a lane keeps its 4 sums in registers
// over the chunk.  Which wave computes an item depends on the grid, what it computes does not.
__global__ __launch_bounds__(256) void gradient_partial_kernel(const float *__restrict__ wts, long long n, long long pairs,
                                                               uint64_t seed, uint64_t generation, unsigned long long pair_base,
                                                               float *__restrict__ slab) {
  const long long B4 = (n + 3) >> 2;
  const unsigned long long Q = (unsigned long long)((n + 7) >> 3);
  const long long W64 = (B4 + 63) >> 6;  // wave tiles per chunk
  const long long chunks = (pairs + PDS_ES_CHUNK - 1) / PDS_ES_CHUNK;
  const long long tiles = chunks * W64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool aligned = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(slab) & 15) == 0;
  for (long long t = (long long)blockIdx.x * 4 + wave; t < tiles; t += (long long)gridDim.x * 4) {
    const long long c = t / W64, b4 = (t % W64) * 64 + lane;
    if (b4 >= B4) continue;
    const long long k0 = c * PDS_ES_CHUNK;
    const int len = (int)(pairs - k0 < PDS_ES_CHUNK ? pairs - k0 : PDS_ES_CHUNK);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < len; ++k) {
      const float wk = wts[k0 + k];
      float z[4];
      noise4(pair_base + (unsigned long long)(k0 + k), b4, Q, generation, seed, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(wk, z[e], acc[e]);
    }
    const long long j = b4 << 2;
    float *dst = slab + c * n + j;
    if (aligned) store4<true>(dst, acc, 4);
    else store4<false>(dst, acc, (int)(n - j < 4 ? n - j : 4));
  }
}

// grad[j] = scale (slab[0][j] + slab[1][j] + ..) + l2 mu[j]: the slabs in chunk order
__global__ __launch_bounds__(256) void gradient_sum_kernel(const float *__restrict__ slab, const float *__restrict__ mu,
                                                           long long n, long long chunks, float scale, float l2,
                                                           float *__restrict__ grad) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    float s = 0.f;
    for (long long c = 0; c < chunks; ++c) s += slab[c * n + j];
    grad[j] = mu != nullptr ? fmaf(l2, mu[j], scale * s) : scale * s;
  }
}

// the id packing of PDS_GAUSSIAN_PHILOX holds sample ids below 2^56
static bool ids_fit(int64_t n, int64_t pairs, uint64_t pair_base) {
  const unsigned __int128 Q = (unsigned __int128)((n + 7) / 8);
  return ((unsigned __int128)pair_base + (unsigned __int128)pairs) * Q < ((unsigned __int128)1 << 56);
}

static unsigned capped_grid(long long blocks) { return (unsigned)(blocks < 2048 ? (blocks < 1 ? 1 : blocks) : 2048); }

}  // namespace pds_es_detail
using namespace pds_es_detail;

extern "C" int64_t pds_es_workspace_floats(int64_t n, int64_t pairs) {
  if (n < 1 || pairs < 1) return PDS_EINVAL;
  return ((pairs + PDS_ES_CHUNK - 1) / PDS_ES_CHUNK) * n;
}

extern "C" int pds_es_perturb(const float *d_mu, int64_t n, int64_t pairs, float sigma, uint64_t seed, uint64_t generation,
                              uint64_t pair_base, float *d_theta, void *stream) {
  if (!d_mu || !d_theta || n < 1 || pairs < 1 || !isfinite(sigma) || !(sigma > 0.f)) return PDS_EINVAL;
  if (!ids_fit(n, pairs, pair_base)) return PDS_EINVAL;
  const unsigned __int128 blocks = ((unsigned __int128)pairs * ((n + 3) / 4) + 255) / 256;
  const unsigned grid = capped_grid(blocks > 2048 ? 2048 : (long long)blocks);
  // the branch-free form needs rows AND base pointers on 16 bytes (a caller may pass a view into a larger tensor)
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(d_mu) | reinterpret_cast<uintptr_t>(d_theta)) & 15) == 0)
    hipLaunchKernelGGL(perturb_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_mu, (long long)n, (long long)pairs,
                       sigma, seed, generation, (unsigned long long)pair_base, d_theta);
  else
    hipLaunchKernelGGL(perturb_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_mu, (long long)n, (long long)pairs,
                       sigma, seed, generation, (unsigned long long)pair_base, d_theta);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}

extern "C" int pds_es_gradient(const float *d_pair_weights, const float *d_mu, int64_t n, int64_t pairs, float scale, float l2,
                               uint64_t seed, uint64_t generation, uint64_t pair_base, float *d_grad, float *d_workspace,
                               void *stream) {
  if (!d_pair_weights || !d_grad || !d_workspace || n < 1 || pairs < 1 || !isfinite(scale) || !isfinite(l2)) return PDS_EINVAL;
  if (!ids_fit(n, pairs, pair_base)) return PDS_EINVAL;
  const long long B4 = (n + 3) / 4, W64 = (B4 + 63) / 64;
  const long long chunks = (pairs + PDS_ES_CHUNK - 1) / PDS_ES_CHUNK;
  const unsigned __int128 tiles = (unsigned __int128)chunks * W64;
  const unsigned grid = capped_grid(tiles > 4 * 2048 ? 2048 : (long long)((tiles + 3) / 4));
  hipLaunchKernelGGL(gradient_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_pair_weights, (long long)n,
                     (long long)pairs, seed, generation, (unsigned long long)pair_base, d_workspace);
  hipLaunchKernelGGL(gradient_sum_kernel, dim3(capped_grid((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_workspace,
                     d_mu, (long long)n, chunks, scale, l2, d_grad);
  return hipGetLastError() == hipSuccess ? PDS_OK : PDS_EHIP;
}
