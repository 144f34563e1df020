// resamplez_u8.hip -- a uint8 volume resampled along z through a table of taps, one (z0, w) per output section
// (utils.volume_resample_z: sections of measured, uneven spacing brought onto an even grid):
//   tem_u8_resample_z    dst[o] = ((256 - w) V[z0] + w V[min(z0 + 1, VZ - 1)] + 128) >> 8,  nearest: w < 128 ? V[z0] : V[z0 + 1]
// The definition is in include/tem_hip.h.
//
// A plane is the same flat run of H W bytes on both sides.  A thread owns one 16-byte piece of it -- bytes
// [16 i, min(16 i + 16, H W)) of every plane -- and marches a RUN of output planes with two source planes' words of its
// piece in registers: A of plane `ha`, B of plane `hb`.  The next output's tap is the same for every thread (one read
// through readfirstlane, so the choice below is a scalar branch):
//   z0 == ha                 both planes are reused
//   z0 == hb                 A = B, and only plane z0 + 1 is loaded
//   otherwise                both are loaded
// and B is loaded only for w > 0.  That is right for any table; a table that does not decrease reads every source plane
// once per run.  Every z0 read from the device is clamped into the block, so a table that disagrees with the host's
// copy gives wrong bytes and never a fault.
//
// Loads are zc_load's (zc_pieces.h): only naturally aligned words that hold a byte of the piece.  Stores are one
// dwordx4 where the piece is whole and starts on a 16-byte boundary; otherwise the bytes up to the first 4-byte
// boundary, the aligned words, and the bytes behind them: every byte of the piece exactly once, nothing else.  src and
// dst may differ in alignment, and H W need not be a multiple of anything.
#include "zc_pieces.h"

namespace {

constexpr int RZ_MAX_RUN = 32;                   // output planes per run, at most
constexpr int RZ_WANT_GRID = 2048;               // workgroups the run length aims at
constexpr int64_t RZ_MAX_WGS = (int64_t)1 << 24; // workgroups of one launch: their 256 threads stay below 2^32

__device__ __forceinline__ void rz_store(uint8_t *p, int n, const uint32_t (&w)[4]) {
  if (n == 16 && !((uintptr_t)p & 15)) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
  const int h = min(n, (int)((4 - ((uintptr_t)p & 3)) & 3));            // bytes up to the first 4-byte boundary
  const int nw = (n - h) >> 2;                                           // whole aligned words behind them
  uint32_t *q = reinterpret_cast<uint32_t *>(p + h);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nw) q[j] = __builtin_amdgcn_alignbyte(j < 3 ? w[j + 1] : 0u, w[j], (uint32_t)h);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if ((j < h || j >= h + 4 * nw) && j < n) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}

// Two bytes per multiply: the even bytes and the odd bytes of a word as two 16-bit lanes each.  A lane holds
// (256 - w) a + w b + 128 <= 255 x 256 + 128 = 65408 < 2^16: nothing carries from one lane into the next.
__device__ __forceinline__ uint32_t rz_blend(uint32_t a, uint32_t b, uint32_t w) {
  const uint32_t m = 0x00FF00FFu, u = 256u - w;
  const uint32_t even = (a & m) * u + (b & m) * w + 0x00800080u;
  const uint32_t odd = ((a >> 8) & m) * u + ((b >> 8) & m) * w + 0x00800080u;
  return ((even >> 8) & m) | (odd & ~m);
}

// Block b = run * pblocks + pb: pieces [256 pb, 256 pb + 256) of output planes [run * zr, min((run + 1) * zr, OD)).
__global__ __launch_bounds__(ZC_THREADS) void u8_resample_z_k(const uint8_t *src, int32_t D, int64_t plane, int32_t sz0,
                                                              uint8_t *dst, int32_t OD, int32_t oz0,
                                                              const int32_t *taps, int32_t nearest, uint32_t pblocks,
                                                              int32_t zr) {
  const uint32_t pb = blockIdx.x % pblocks, run = blockIdx.x / pblocks;
  const int64_t at = 16 * ((int64_t)pb * ZC_THREADS + threadIdx.x);
  if (at >= plane) return;
  const int n = (int)min((int64_t)16, plane - at);
  const int32_t o0 = (int32_t)run * zr, o1 = min(o0 + zr, OD);
  int32_t ha = -1, hb = -1;                                             // the block's planes held in A and B
  uint32_t A[4] = {0, 0, 0, 0}, B[4] = {0, 0, 0, 0};
  for (int32_t o = o0; o < o1; ++o) {
    const int32_t *t = taps + 2 * ((int64_t)oz0 + o);
    const int32_t za = min(max(__builtin_amdgcn_readfirstlane(t[0]), sz0), sz0 + D - 1) - sz0, zb = min(za + 1, D - 1);
    const uint32_t w = (uint32_t)min(max(__builtin_amdgcn_readfirstlane(t[1]), 0), 255);
    if (za != ha) {
      if (za == hb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) A[j] = B[j];
      } else {
        zc_load(src + (int64_t)za * plane + at, n, A);
      }
      ha = za;
    }
    if (w && zb != hb) {
      if (zb == ha) {                                                   // only where the table left the block: clamped
#pragma unroll
        for (int j = 0; j < 4; ++j) B[j] = A[j];
      } else {
        zc_load(src + (int64_t)zb * plane + at, n, B);
      }
      hb = zb;
    }
    uint32_t r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = nearest ? (w < 128 ? A[j] : B[j]) : rz_blend(A[j], B[j], w);
    rz_store(dst + (int64_t)o * plane + at, n, r);
  }
}

}  // namespace

extern "C" int tem_u8_resample_z(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t VZ,
                                 uint8_t *dst, int32_t OD, int32_t oz0, int32_t NZ, const int32_t *taps_host,
                                 const int32_t *taps_dev, int32_t nearest, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || !taps_host || !taps_dev || D < 1 || H < 1 || W < 1 || OD < 1 || VZ < 1 || NZ < 1 || sz0 < 0 ||
      (int64_t)sz0 + D > VZ || oz0 < 0 || (int64_t)oz0 + OD > NZ || nearest < 0 || nearest > 1)
    return TEM_EINVAL;
  for (int64_t o = oz0; o < (int64_t)oz0 + OD; ++o) {                    // the block's rows of the table
    const int32_t z0 = taps_host[2 * o], w = taps_host[2 * o + 1];
    if (z0 < 0 || z0 > VZ - 1 || w < 0 || w > 255) return TEM_EINVAL;
    const int32_t last = w ? (z0 + 1 < VZ ? z0 + 1 : VZ - 1) : z0;       // a tap of weight 0 is no tap
    if (z0 < sz0 || last >= sz0 + D) return TEM_EINVAL;
  }
  const int64_t plane = (int64_t)H * W;
  const int64_t pblocks = (plane + 16 * ZC_THREADS - 1) / (16 * ZC_THREADS);   // < 2^50
  int64_t zr = (int64_t)OD * pblocks / RZ_WANT_GRID;
  zr = zr < 1 ? 1 : (zr > RZ_MAX_RUN ? RZ_MAX_RUN : zr);
  const int64_t nruns = (OD + zr - 1) / zr;
  if (pblocks >= RZ_MAX_WGS || pblocks * nruns >= RZ_MAX_WGS) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_resample_z_k, dim3((unsigned)(pblocks * nruns)), dim3(ZC_THREADS), 0, (hipStream_t)stream, src,
                     D, plane, sz0, dst, OD, oz0, taps_dev, nearest, (uint32_t)pblocks, (int32_t)zr);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
