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

// Spread of the self-ensemble: the members' population standard deviation at a voxel, from moments about the first
// member r (the shift keeps fp32 sufficient: the members lie close to each other, not to 0).  Every operation is one
// individually rounded fp32 operation, so numpy float32 reproduces every bit.  contract(off): hipcc fuses a multiply
// and the addition that follows it into v_fma_f32 even when they are spelled __fmul_rn / __fadd_rn.
//   per member m >= 1:  d = y_m - r;  s1 += d;  s2 += d * d
__device__ __forceinline__ void spread_update(float y, float r, float &s1, float &s2) {
#pragma clang fp contract(off)
  const float d = __fsub_rn(y, r);
  s1 = __fadd_rn(s1, d);
  const float p = d * d;
  s2 = s2 + p;
}

//   sd = sqrt(max(s2 - s1^2 / k, 0) / k)  (sqrtf: correctly rounded under the build's flags, __fsqrt_rn is not);
//   u8 = rint(min(sd |std_y| 127.5 gain, 255)): grey levels of the output times the gain, saturating
__device__ __forceinline__ uint8_t spread_u8(float s1, float s2, float k, float absstd, float gain) {
#pragma clang fp contract(off)
  const float sq = s1 * s1;
  const float t = __fdiv_rn(sq, k);
  const float v = __fdiv_rn(fmaxf(__fsub_rn(s2, t), 0.f), k);
  const float sd = sqrtf(v);
  const float g = (sd * absstd) * 127.5f;
  return (uint8_t)(int)rintf(fminf(g * gain, 255.f));
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
