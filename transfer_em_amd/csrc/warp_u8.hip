// warp_u8.hip -- tem_u8_warp_affine: every section of a dense uint8 block resampled through its own affine map, bilinear
// (or nearest) in 1/256 px fixed point with ONE rounding per voxel (include/tem_hip.h has the definition).  A voxel
// depends on its section and its map alone, all in volume coordinates: not on the slab, ROI or rank it is computed in.
//
// Tile.  A workgroup of 256 threads owns WARP_TY x WARP_TX = 16 x 64 outputs of one plane, four x-consecutive outputs
// per thread.  The source position is affine in (y, x), so the extremes of the tile's taps sit at its corners:
//   1. hull: from the corners (uniform per workgroup, 64-bit scalar work) the rows [min iy, max iy + 1] and columns
//      [min ix, max ix + 1] the tile can read, clipped to the section.  The coefficient limit |a - I| <= 1/8 bounds the
//      hull by 27 rows x 75 bytes: sy varies by at most 15 (1 + 1/8) + 63 / 8 = 24.75 px over a tile, sx by 72.75.
//   2. stage: the hull goes to LDS as bytes, by naturally aligned dword loads -- 32 lanes per row, each row from the
//      aligned word that holds its first byte (rows of any alignment: a row's bytes sit `shift` = address & 3 bytes
//      into its LDS row).  Only words that hold at least one byte of the hull are loaded.
//   3. resample: a thread forms its four positions relative to the hull's origin in 32 bits (the hull lies within
//      32 px of the tile's taps wherever one voxel of the tile is inside), reads 2 x 2 bytes of LDS per output, blends
//      in integers and stores its four bytes as one dword where the address is aligned, else byte by byte.
// A tile none of whose voxels can be inside skips 1 and 2 and writes `fill`.
//
// Safety.  The kernel reads the maps from device memory, the host validated its own copy.  The kernel clamps every
// coefficient to the limits, the hull to the source block and to the LDS array, and every tap to the staged hull: a
// device table that disagrees with the host's gives wrong bytes, never a load outside the block or LDS.  With a table
// that agrees every clamp is the identity.
#include <algorithm>

#include "tem_common.h"

namespace {

constexpr int WARP_TY = 16, WARP_TX = 64;              // outputs per workgroup, (y, x): four along x per thread
constexpr int WARP_THREADS = WARP_TY * WARP_TX / 4;
constexpr int WARP_ONE = 1 << 16, WARP_DEV = 1 << 13;  // the unit, and how far a matrix coefficient may sit from I
constexpr int64_t WARP_MAX_B = ((int64_t)1 << 47) - 1;
constexpr int WARP_HY = 27, WARP_HX = 75;              // the hull of a tile's taps at the coefficient limits
constexpr int WARP_HDW = (3 + WARP_HX + 3) / 4;        // dwords of an LDS row: a shift of up to 3 bytes ahead of it
constexpr int64_t WARP_MAX_WGS = (1 << 24) - 1;        // x 256 threads stays below 2^32, the launch's limit

struct warp_args {
  const uint8_t *src;
  int64_t H, W;                                        // the source block's rows and the section's columns
  int sy0, VY;
  uint8_t *dst;
  int OH, OW, oy0, ox0;
  int tiles_x, tiles;                                  // tiles along x, tiles per plane
  const long long *maps;                               // device: [D][6] = a_yy, a_yx, b_y, a_xy, a_xx, b_x in 2^-16
  int fill;
};

__host__ __device__ inline int64_t wp_min(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t wp_max(int64_t a, int64_t b) { return a > b ? a : b; }
__host__ __device__ inline int64_t wp_clamp(int64_t v, int64_t lo, int64_t hi) { return wp_min(wp_max(v, lo), hi); }

// s = a_y y + a_x x + b over the rectangle [y0, y0 + ny) x [x0, x0 + nx): its least and largest value (at corners)
__host__ __device__ inline void warp_range(int64_t ay, int64_t ax, int64_t b, int64_t y0, int64_t ny, int64_t x0, int64_t nx,
                                           int64_t &lo, int64_t &hi) {
  const int64_t s = ay * y0 + ax * x0 + b, ey = ay * (ny - 1), ex = ax * (nx - 1);
  lo = s + wp_min(ey, 0) + wp_min(ex, 0), hi = s + wp_max(ey, 0) + wp_max(ex, 0);
}

template <bool NEAREST>
__global__ __launch_bounds__(WARP_THREADS) void u8_warp_affine_k(warp_args g) {
  __shared__ uint32_t hull[WARP_HY * WARP_HDW];
  const uint8_t *hb = (const uint8_t *)hull;

  const int tid = threadIdx.x;
  const int d = blockIdx.x / g.tiles, tile = blockIdx.x - d * g.tiles;
  const int tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
  const int by0 = tyi * WARP_TY, bx0 = txi * WARP_TX;                    // the tile's first output in the block
  const int nyv = min(WARP_TY, g.OH - by0), nxv = min(WARP_TX, g.OW - bx0);

  // the plane's map, every coefficient clamped to the limits the host checked on its copy
  const long long *m = g.maps + 6 * (int64_t)d;
  const int ayy = (int)wp_clamp(m[0], WARP_ONE - WARP_DEV, WARP_ONE + WARP_DEV), ayx = (int)wp_clamp(m[1], -WARP_DEV, WARP_DEV);
  const int axy = (int)wp_clamp(m[3], -WARP_DEV, WARP_DEV), axx = (int)wp_clamp(m[4], WARP_ONE - WARP_DEV, WARP_ONE + WARP_DEV);
  const int64_t bsy = wp_clamp(m[2], -WARP_MAX_B, WARP_MAX_B), bsx = wp_clamp(m[5], -WARP_MAX_B, WARP_MAX_B);

  // the tile's source range (uniform): is any voxel inside, and the hull of the taps
  int64_t sylo, syhi, sxlo, sxhi;
  warp_range(ayy, ayx, bsy, (int64_t)g.oy0 + by0, nyv, (int64_t)g.ox0 + bx0, nxv, sylo, syhi);
  warp_range(axy, axx, bsx, (int64_t)g.oy0 + by0, nyv, (int64_t)g.ox0 + bx0, nxv, sxlo, sxhi);
  const int64_t FY = 256 * ((int64_t)g.VY - 1), FX = 256 * (g.W - 1);
  const bool any = ((syhi + 128) >> 8) >= 0 && ((sylo + 128) >> 8) <= FY && ((sxhi + 128) >> 8) >= 0 && ((sxlo + 128) >> 8) <= FX;
  const int64_t top = g.sy0 + g.H - 1;
  const int64_t hy0 = wp_clamp(wp_clamp((sylo + 128) >> 16, 0, g.VY - 1), g.sy0, top);
  const int64_t hy1 = wp_clamp(wp_clamp(((syhi + 128) >> 16) + 1, 0, g.VY - 1), hy0, top);
  const int64_t hx0 = wp_clamp((sxlo + 128) >> 16, 0, g.W - 1);
  const int64_t hx1 = wp_clamp(((sxhi + 128) >> 16) + 1, hx0, g.W - 1);
  const int nr = (int)wp_min(hy1 - hy0 + 1, WARP_HY), nc = (int)wp_min(hx1 - hx0 + 1, WARP_HX);

  const uint8_t *row0 = g.src + ((int64_t)d * g.H + (hy0 - g.sy0)) * g.W + hx0;   // the hull's first byte
  const int a0 = (int)((uintptr_t)row0 & 3), w3 = (int)(g.W & 3);                // a row's shift: (a0 + r w3) & 3
  if (any) {
    const int k = tid & 31;
    for (int r = tid >> 5; r < nr; r += WARP_THREADS / 32) {
      const int sh = (a0 + r * w3) & 3;
      if (4 * k < sh + nc) hull[r * WARP_HDW + k] = *(const uint32_t *)(row0 + (int64_t)r * g.W - sh + 4 * k);
    }
    __syncthreads();
  }

  // positions relative to the hull's origin: 32 bits hold them wherever a voxel of the tile is inside
  const int64_t S0y = (int64_t)ayy * (g.oy0 + by0) + (int64_t)ayx * (g.ox0 + bx0) + bsy;
  const int64_t S0x = (int64_t)axy * (g.oy0 + by0) + (int64_t)axx * (g.ox0 + bx0) + bsx;
  constexpr int64_t FAR = (int64_t)1 << 28;
  const int rely = (int)wp_clamp(S0y - hy0 * 65536, -FAR, FAR), relx = (int)wp_clamp(S0x - hx0 * 65536, -FAR, FAR);
  // inside: 0 <= fy <= 256 (VY - 1), stated for fy - 256 hy0 (an empty interval where nothing is inside)
  const int ylo = any ? (int)wp_max(-256 * hy0, -FAR) : 1, yhi = any ? (int)wp_min(FY - 256 * hy0, FAR) : 0;
  const int xlo = (int)wp_max(-256 * hx0, -FAR), xhi = (int)wp_min(FX - 256 * hx0, FAR);
  const int ylast = (int)wp_min(g.VY - 1 - hy0, FAR), xlast = (int)wp_min(g.W - 1 - hx0, FAR);   // the section's last row, column

  const int ly = tid >> 4, lx = (tid & 15) * 4;
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int fy = (rely + ayy * ly + ayx * (lx + j) + 128) >> 8, fx = (relx + axy * ly + axx * (lx + j) + 128) >> 8;
    const bool inside = fy >= ylo && fy <= yhi && fx >= xlo && fx <= xhi;
    uint32_t v;
    if (NEAREST) {
      const int r = min(max((fy + 128) >> 8, 0), nr - 1), c = min(max((fx + 128) >> 8, 0), nc - 1);
      v = hb[r * (4 * WARP_HDW) + ((a0 + r * w3) & 3) + c];
    } else {
      const int iy = fy >> 8, ix = fx >> 8;
      const uint32_t ty = fy & 255, tx = fx & 255;
      const int r0 = min(max(iy, 0), nr - 1), r1 = min(max(min(iy + 1, ylast), 0), nr - 1);
      const int c0 = min(max(ix, 0), nc - 1), c1 = min(max(min(ix + 1, xlast), 0), nc - 1);
      const uint8_t *p0 = hb + r0 * (4 * WARP_HDW) + ((a0 + r0 * w3) & 3), *p1 = hb + r1 * (4 * WARP_HDW) + ((a0 + r1 * w3) & 3);
      const uint32_t top2 = (256 - tx) * p0[c0] + tx * p0[c1], bot2 = (256 - tx) * p1[c0] + tx * p1[c1];
      v = ((256 - ty) * top2 + ty * bot2 + (1u << 15)) >> 16;             // at most 2^24 before the shift
    }
    packed |= (inside ? v : (uint32_t)g.fill) << (8 * j);
  }
  if (ly >= nyv || lx >= nxv) return;
  uint8_t *o = g.dst + ((int64_t)d * g.OH + (by0 + ly)) * g.OW + (bx0 + lx);
  if (lx + 3 < nxv && ((uintptr_t)o & 3) == 0) {
    *(uint32_t *)o = packed;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lx + j < nxv) o[j] = (uint8_t)(packed >> (8 * j));
  }
}

}  // namespace

extern "C" int tem_u8_warp_affine(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY, uint8_t *dst,
                                  int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
                                  const int64_t *maps_dev, int32_t fill, int32_t nearest, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || !maps_host || !maps_dev || D < 1 || H < 1 || W < 1 || VY < 1 || OD != D || OH < 1 || OW < 1 || sy0 < 0 ||
      oy0 < 0 || ox0 < 0 || fill < 0 || fill > 255 || (nearest != 0 && nearest != 1))
    return TEM_EINVAL;
  if ((int64_t)sy0 + H > VY || (int64_t)oy0 + OH > VY || (int64_t)ox0 + OW > W) return TEM_EINVAL;
  const int64_t tiles_x = ((int64_t)OW + WARP_TX - 1) / WARP_TX, tiles_y = ((int64_t)OH + WARP_TY - 1) / WARP_TY;
  if (tiles_x * tiles_y > WARP_MAX_WGS || tiles_x * tiles_y * D > WARP_MAX_WGS) return TEM_EINVAL;
  const int64_t FY = 256 * ((int64_t)VY - 1), FX = 256 * ((int64_t)W - 1);
  for (int64_t d = 0; d < D; ++d) {
    const int64_t *m = maps_host + 6 * d;
    if (m[0] < WARP_ONE - WARP_DEV || m[0] > WARP_ONE + WARP_DEV || m[4] < WARP_ONE - WARP_DEV || m[4] > WARP_ONE + WARP_DEV ||
        m[1] < -WARP_DEV || m[1] > WARP_DEV || m[3] < -WARP_DEV || m[3] > WARP_DEV || m[2] < -WARP_MAX_B || m[2] > WARP_MAX_B ||
        m[5] < -WARP_MAX_B || m[5] > WARP_MAX_B)
      return TEM_EINVAL;
    // the rows that the block's inside voxels read with a weight above 0, bounded from its corners
    int64_t sylo, syhi, sxlo, sxhi;
    warp_range(m[0], m[1], m[2], oy0, OH, ox0, OW, sylo, syhi);
    warp_range(m[3], m[4], m[5], oy0, OH, ox0, OW, sxlo, sxhi);
    const int64_t fylo = wp_max((sylo + 128) >> 8, 0), fyhi = wp_min((syhi + 128) >> 8, FY);
    if (fylo > fyhi || wp_max((sxlo + 128) >> 8, 0) > wp_min((sxhi + 128) >> 8, FX)) continue;    // every voxel is outside
    const int64_t lo = nearest ? (fylo + 128) >> 8 : fylo >> 8;
    const int64_t hi = nearest ? (fyhi + 128) >> 8 : (fyhi >> 8) + ((fyhi & 255) ? 1 : 0);
    if (lo < sy0 || hi >= (int64_t)sy0 + H) return TEM_EINVAL;
  }
  warp_args g;
  g.src = src, g.H = H, g.W = W, g.sy0 = sy0, g.VY = VY;
  g.dst = dst, g.OH = OH, g.OW = OW, g.oy0 = oy0, g.ox0 = ox0;
  g.tiles_x = (int)tiles_x, g.tiles = (int)(tiles_x * tiles_y);
  g.maps = (const long long *)maps_dev, g.fill = fill;
  const unsigned wgs = (unsigned)(g.tiles * (int64_t)D);
  if (nearest)
    hipLaunchKernelGGL(u8_warp_affine_k<true>, dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, g);
  else
    hipLaunchKernelGGL(u8_warp_affine_k<false>, dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, g);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
