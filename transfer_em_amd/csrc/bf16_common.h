// Shared pieces of the bf16 kernels: vector types, the scalar conversions, and the host code every bf16 convolution
// dispatch needs -- the alignment predicate and the translation of tem_epilogue into a kernel's own Ep struct.
// (Kernel-argument structs stay per kernel: a field more or less changes the schedule of the kernels that take them.)
#pragma once
#include "tem_common.h"

namespace tem_bf16 {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }   // round to nearest even

// x / d for 0 <= x < 2^31 with magic = magic_for(d) = ceil(2^32 / d) (d == 1: the magic does not fit 32 bits)
__device__ __forceinline__ int fdiv(int x, int d, uint32_t magic) { return d == 1 ? x : (int)__umulhi((uint32_t)x, magic); }

// bf16 tensors travel behind the float* fields of the C ABI (strides in elements)
static inline const u16 *as_u16(const float *q) { return reinterpret_cast<const u16 *>(q); }

// Origin and strides of `v` are multiples of n bf16 elements (n = 8: 16-byte channel chunks, n = 4: 8-byte accesses).
// d3 == false leaves out the depth stride: the 2-D kernels never read it, and their depth-1 views may carry any.
static inline bool aligned(const tem_view &v, int n, bool d3) {
  return ((uintptr_t)v.ptr & (uintptr_t)(2 * n - 1)) == 0 && v.sW % n == 0 && v.sH % n == 0 && (!d3 || v.sD % n == 0) && v.sN % n == 0;
}

// tem_epilogue -> the Ep struct of a bf16 convolution kernel (everything but `bias`, which the transposed kernels lack):
// gate and skip-gradient views, Philox key, keep mask, dropout frame, and the byte ranges of the three buffers the epilogue
// loads through descriptors.  o0 is the output view the epilogue applies to.
//   D3:  Ep has the depth fields (gD, aD, aoz, aDd); a 2-D Ep takes depth-1 views (o0.D == 1: checked by the caller)
//        and no depth offset.
//   FWD: the rules of conv_bf16_k / conv2d_bf16_k, whose lanes own 4 channels where C_out allows: gate / add need
//        C_out % 4 == 0 (a view with another channel count is not tested for alignment), Dropout needs C_out % 8 == 0.
//        The transposed kernels (FWD == false) test every view and need C_out % 8 == 0 only where a keep mask is used.
template <bool D3, bool FWD, typename Ep>
static int fill_epilogue(Ep &q, const tem_epilogue &e, const tem_view &o0) {
  auto al8 = [](const tem_view &v) { return (FWD && v.C % 4 != 0) || aligned(v, 4, D3); };
  q.slope = e.slope; q.gate_slope = e.gate_slope;
  if (e.gate.ptr) {
    const tem_view &g = e.gate;
    if (g.N != o0.N || g.D != o0.D || g.H != o0.H || g.W != o0.W || g.C < o0.C) return TEM_ESHAPE;
    if (!fits32(g) || !al8(g) || (FWD && o0.C % 4)) return TEM_EUNSUPPORTED;
    q.gate = as_u16(g.ptr); q.gN = (int)g.sN; q.gH = (int)g.sH; q.gW = (int)g.sW;
    if constexpr (D3) q.gD = (int)g.sD;
  }
  if (e.add.ptr) {
    const tem_view &ad = e.add;
    if (ad.C < o0.C || ad.N != o0.N || (!D3 && (ad.D != 1 || e.add_off[0] != 0))) return TEM_ESHAPE;
    if (!fits32(ad) || !al8(ad) || (FWD && o0.C % 4)) return TEM_EUNSUPPORTED;
    q.add = as_u16(ad.ptr); q.aN = (int)ad.sN; q.aH = (int)ad.sH; q.aW = (int)ad.sW;
    q.aoy = e.add_off[1]; q.aox = e.add_off[2];
    q.aHh = ad.H; q.aWw = ad.W;
    if constexpr (D3) { q.aD = (int)ad.sD; q.aoz = e.add_off[0]; q.aDd = ad.D; }
  }
  q.dropout = e.dropout;
  q.ds.k0 = (uint32_t)e.seed; q.ds.k1 = (uint32_t)(e.seed >> 32); q.ds.site = e.site; q.ds.step = e.step;
  q.step_dev = e.step_dev;
  q.keep_mask = (e.dropout && e.keep_mask) ? e.keep_mask : nullptr;
  q.keep_mode = q.keep_mask ? e.keep_mode : 0;
  if ((FWD ? e.dropout : q.keep_mode) && o0.C % 8) return TEM_EUNSUPPORTED;
  q.doz = e.drop_org[0]; q.doy = e.drop_org[1]; q.dox = e.drop_org[2];
  q.dD = e.drop_dims[0] ? e.drop_dims[0] : o0.D; q.dH = e.drop_dims[0] ? e.drop_dims[1] : o0.H;
  q.dW = e.drop_dims[0] ? e.drop_dims[2] : o0.W;
  const int64_t melems = (int64_t)o0.N * q.dD * q.dH * q.dW * o0.C;
  if (melems >= ((int64_t)1 << 33)) return TEM_EUNSUPPORTED;
  q.mbytes = (int)((melems + 7) / 8);
  if ((e.gate.ptr && view_span(e.gate) >= ((int64_t)1 << 30)) || (e.add.ptr && view_span(e.add) >= ((int64_t)1 << 30)))
    return TEM_EUNSUPPORTED;                       // byte offsets of the epilogue's buffer loads stay below 2^31
  q.gbytes = e.gate.ptr ? (int)(view_span(e.gate) * 2) : 0;
  q.abytes = e.add.ptr ? (int)(view_span(e.add) * 2) : 0;
  return TEM_OK;
}

}  // namespace tem_bf16
