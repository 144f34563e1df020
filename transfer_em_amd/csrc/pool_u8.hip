// pool_u8.hip -- one level of a mip pyramid of a uint8 block: dst = src pooled by (fz, 2, 2) over (z, y, x), the mean
// of the children that lie inside the valid extents, rounded half up in integers.
//   src[D][H][W] dense, valid extents (vD, vH, vW);  dst[ceil(D/fz)][ceil(H/2)][ceil(W/2)] dense
//   dst[z][y][x] = (sum + (cnt >> 1)) >> log2(cnt) over the children (fz z + a, 2y + b, 2x + c) inside the valid
//   extents; cnt in {1, 2, 4, 8}; no valid child: 0
//
// A bandwidth kernel: every source byte is read once, 1/8 (fz = 2) or 1/4 (fz = 1) as many are written.  Lanes run
// along x.  A thread owns one group: 4 consecutive outputs of one dst row, i.e. 8 consecutive bytes of each of its
// 2 fz source rows.  The 8 bytes of a row travel as one 64-bit word; the pair sums are formed on the whole word (even
// bytes + odd bytes: four 16-bit lanes of at most 510), the rows are added in the same form (at most 4 x 510 = 2040 per
// lane), and the 4 results leave as one dword.
//
// Row starts are only as aligned as W allows (W even in the pipeline, e.g. 222 k for the 260 model: 2-byte aligned
// rows), so a row's 8 bytes are fetched by the widest form its address allows, chosen per row:
//   8-byte aligned          one dwordx2 load
//   2-byte aligned          four ushort loads
//   odd address, or a group that crosses the end of the row (W % 8 != 0): byte loads of the valid bytes only
// The wide forms read all 8 bytes -- they lie inside the row -- and clear the ones at x >= vW; all three give the same
// word.  A row outside (vD, vH) and a group wholly at x >= vW is not read at all.  The store is one dword where the 4
// outputs lie inside the dst row on a 4-byte boundary, bytes otherwise (the row's tail, unaligned rows).  Every dst
// byte belongs to exactly one group, so it is written exactly once.  No LDS, no atomics, no scratch.
#include "tem_common.h"

namespace {

// bytes [0, nv) of the 8 bytes at p, as a little-endian word; the others 0.  `full`: all 8 lie inside the row.
__device__ __forceinline__ uint64_t load_row8(const uint8_t *p, int nv, bool full) {
  const uintptr_t a = (uintptr_t)p;
  uint64_t w = 0;
  if (full && (a & 7) == 0) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    w = (uint64_t)v.x | ((uint64_t)v.y << 32);
  } else if (full && (a & 1) == 0) {
    const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
    w = (uint64_t)q[0] | ((uint64_t)q[1] << 16) | ((uint64_t)q[2] << 32) | ((uint64_t)q[3] << 48);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nv) w |= (uint64_t)p[i] << (8 * i);
    return w;
  }
  return nv >= 8 ? w : (w & ((1ull << (8 * nv)) - 1ull));            // 1 <= nv here
}

template <int FZ>
__global__ __launch_bounds__(256) void u8_pool2_k(const uint8_t *src, int H, int W, int vD, int vH, int vW,
                                                  uint8_t *dst, int oH, int oW, int gpr, int64_t ngroup) {
  const int64_t g = (int64_t)xcd_contiguous_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= ngroup) return;
  const int64_t r = g / gpr;                                           // dst row
  const int gx = (int)(g - r * gpr);
  const int z = (int)(r / oH), y = (int)(r - (int64_t)z * oH);
  const int x0 = 8 * gx;                                               // first source byte of the group
  const int nv = min(max(vW - x0, 0), 8);                              // valid source bytes of the group
  const bool full = x0 + 8 <= W;
  const int nz = min(max(vD - FZ * z, 0), FZ), ny = min(max(vH - 2 * y, 0), 2);   // valid children along z, y
  uint64_t acc = 0;                                                    // four 16-bit sums
  if (nv > 0) {
#pragma unroll
    for (int a = 0; a < FZ; ++a) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (a < nz && b < ny) {
          const uint64_t w = load_row8(src + ((int64_t)(FZ * z + a) * H + (2 * y + b)) * W + x0, nv, full);
          acc += (w & 0x00FF00FF00FF00FFull) + ((w >> 8) & 0x00FF00FF00FF00FFull);
        }
      }
    }
  }
  const int szy = (nz == 2) + (ny == 2);                               // log2 of the z, y children
  uint32_t q = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nx = min(max(vW - (x0 + 2 * j), 0), 2);
    const int cnt = nz * ny * nx, sh = szy + (nx == 2);                // cnt == 0: the sum is 0 as well
    const uint32_t s = (uint32_t)(acc >> (16 * j)) & 0xFFFFu;
    q |= ((s + (uint32_t)(cnt >> 1)) >> sh) << (8 * j);
  }
  uint8_t *o = dst + r * oW + 4 * gx;
  const int n = min(4, oW - 4 * gx);
  if (n == 4 && ((uintptr_t)o & 3) == 0) {
    *reinterpret_cast<uint32_t *>(o) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) o[j] = (uint8_t)(q >> (8 * j));
  }
}

}  // namespace

extern "C" int tem_u8_pool2(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t vD, int32_t vH, int32_t vW,
                            int32_t fz, uint8_t *dst, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || D < 1 || H < 1 || W < 1 || vD < 0 || vD > D || vH < 0 || vH > H || vW < 0 || vW > W ||
      (fz != 1 && fz != 2))
    return TEM_EINVAL;
  const int oD = (D + fz - 1) / fz, oH = (H + 1) / 2, oW = (W + 1) / 2, gpr = (oW + 3) / 4;
  const int64_t ngroup = (int64_t)oD * oH * gpr;
  const int64_t nblk = (ngroup + 255) / 256;
  if (nblk > 0x7fffffff) return TEM_EUNSUPPORTED;
  if (fz == 2)
    hipLaunchKernelGGL(u8_pool2_k<2>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, src, H, W, vD, vH, vW,
                       dst, oH, oW, gpr, ngroup);
  else
    hipLaunchKernelGGL(u8_pool2_k<1>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, src, H, W, vD, vH, vW,
                       dst, oH, oW, gpr, ngroup);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
