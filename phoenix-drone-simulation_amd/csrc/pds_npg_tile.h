// pds_npg_tile.h -- what the natural-gradient kernels of both depths share (csrc/pds_npg.hip: struct pds_mlp; csrc/pds_npg_deep.hip:
// struct pds_mlp_deep), each piece written once: the tangent's GEMM from global memory, the candidate transform of the line search,
// and the launches of the two reduce kernels.  fvp_reduce_kernel, surrogate_reduce_kernel and cg_kernel take no network struct
// (a partial is `total` floats per wave, or three per wave and candidate); they live in csrc/pds_npg.hip and the deep unit reaches
// the first two through the launch functions below, so the rule `scale * sum + damping * v` (two products and one sum, each
// rounded once) and the {sum ratio adv, sum KL, non-finite flag, sum ratio} row exist once.
#pragma once
#include "pds_mlp_tile.h"

namespace pds_mlp_detail {

// gemm_lds (pds_mlp_tile.h) with the A operand read from a row-major [rows][cols] matrix in global memory (zero outside it)
template <int NK>
__device__ __forceinline__ f32x4 gemm_glb(const float *V, int rows, int cols, int it, const f32x4 (&in)[NK], int n, int g,
                                          f32x4 c) {
  const int r = it * kTW + n;
  const bool rin = r < rows;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kt * kTW + 4 * g + j;
      const float av = (rin && k < cols) ? V[r * cols + k] : 0.f;
      c = PDS_MFMA(av, in[kt][j], c);
    }
  return c;
}

// candidate parameter theta + f s: product and sum rounded separately (no FMA contraction)
__device__ __forceinline__ float cand(float theta, float f, float s) { return __fadd_rn(theta, __fmul_rn(f, s)); }

// out[p] = scale * (sum of element p over the nwaves partials, in a fixed order) + damping * v[p], p < total (fvp_reduce_kernel of
// csrc/pds_npg.hip; out may alias v)
void npg_reduce_fvp(hipStream_t s, const float *partials, int pstride, int nwaves, int total, float scale, float damping,
                    const float *v, float *out);
// out[j] = {sum ratio adv, sum kl, non-finite, sum ratio} over partials[j][nwaves][3] (surrogate_reduce_kernel of csrc/pds_npg.hip)
void npg_reduce_surrogate(hipStream_t s, const float *partials, int nwaves, int num_candidates, float *out);

}  // namespace pds_mlp_detail
