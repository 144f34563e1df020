// Per-voxel arithmetic and boundary folding shared by the tiled-inference kernels (elementwise.hip, tiles_sym.hip).
#pragma once
#include "tem_common.h"

// The per-voxel arithmetic of every uint8 <-> float boundary (whole-array, 3-D tiles, 2-D tiles): one definition, so
// the kernel pairs cannot drift apart.  Correctly rounded float32 ops as in the reference (datasets.py, utils.py:109),
// with one exception: y * std + mean is ONE fused multiply-add (hipcc contracts the __fmul_rn / __fadd_rn pair into
// v_fma_f32, and every release of these kernels has computed it so; it is spelled out here so that it no longer
// depends on the compiler).  Next to a rounding boundary the reference's two roundings can land one step away: the
// oracle comparisons allow 1 LSB on under 1 % of the voxels.
__device__ __forceinline__ float u8_std(float x, float mean, float std) {
  x = __fsub_rn(__fdiv_rn(x, 127.5f), 1.f);          // datasets.py:200
  return __fdiv_rn(__fsub_rn(x, mean), std);         // datasets.py:161-162
}

__device__ __forceinline__ uint8_t unstd_u8(float v, float mean, float std) {
  v = __fmul_rn(__fadd_rn(__fmaf_rn(v, std, mean), 1.f), 127.5f);             // utils.py:109
  const int q = (int)rintf(v);                                                  // np.around: half to even
  return (uint8_t)(q & 0xFF);                                                   // astype(uint8) wraps
}

// Index that coordinate i of an axis of extent n >= 1 reads under a boundary mode: clamp (edge) or mirror without
// repeating the face voxel (reflect, period 2(n-1): numpy.pad's modes for any pad width, extent 1 included).  reflect is
// even in i, so one bounce costs no division; only a coordinate further than n-1 past a face pays the modulo.
template <int MODE>
__device__ __forceinline__ int bc_fold(int i, int n) {
  if constexpr (MODE == TEM_BOUNDARY_EDGE) {
    return min(max(i, 0), n - 1);
  } else {
    if (n == 1) return 0;
    const int m = 2 * (n - 1);
    i = i < 0 ? -i : i;
    if (i >= m) i %= m;
    return i < n ? i : m - i;
  }
}
