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
//
// Box.  tem_u8_warp_box runs the same kernels with BOX = true: the source is a block cut in x as well, the columns
// [sx0, sx0 + BW) of the section, with the row stride BW.  The hull is then clamped to the block on all four sides, a row
// is BW bytes from the one above it (the shift (a0 + r (BW & 3)) & 3), and nothing else changes: the section's width
// still decides what is inside.  With BOX = false both are compiled out and the block is whole rows of the section.
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
  int64_t BW;                                          // BOX kernels: the block's columns [sx0, sx0 + BW), its row stride
  int sx0;
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

template <bool NEAREST, bool BOX>
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
  const int64_t sx0 = BOX ? g.sx0 : 0, BW = BOX ? g.BW : g.W;                     // the block's first column, its row stride
  const int64_t hy0 = wp_clamp(wp_clamp((sylo + 128) >> 16, 0, g.VY - 1), g.sy0, top);
  const int64_t hy1 = wp_clamp(wp_clamp(((syhi + 128) >> 16) + 1, 0, g.VY - 1), hy0, top);
  int64_t hx0 = wp_clamp((sxlo + 128) >> 16, 0, g.W - 1);
  int64_t hx1 = wp_clamp(((sxhi + 128) >> 16) + 1, hx0, g.W - 1);
  if (BOX) hx0 = wp_clamp(hx0, sx0, sx0 + BW - 1), hx1 = wp_clamp(hx1, hx0, sx0 + BW - 1);
  const int nr = (int)wp_min(hy1 - hy0 + 1, WARP_HY), nc = (int)wp_min(hx1 - hx0 + 1, WARP_HX);

  const uint8_t *row0 = g.src + ((int64_t)d * g.H + (hy0 - g.sy0)) * BW + (hx0 - sx0);   // the hull's first byte
  const int a0 = (int)((uintptr_t)row0 & 3), w3 = (int)(BW & 3);                 // a row's shift: (a0 + r w3) & 3
  if (any) {
    const int k = tid & 31;
    for (int r = tid >> 5; r < nr; r += WARP_THREADS / 32) {
      const int sh = (a0 + r * w3) & 3;
      if (4 * k < sh + nc) hull[r * WARP_HDW + k] = *(const uint32_t *)(row0 + (int64_t)r * BW - sh + 4 * k);
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

// ------------------------------------------------------------------------------------------------ tem_u8_warp_field
// tem_u8_warp_field: the affine map plus a displacement field on a lattice of 2^ky x 2^kx pixels (include/tem_hip.h has
// the definition).  The form is the affine kernel's, with the same tile, staging, blend and store:
//   1. hull: the affine extremes from the tile's corners, widened by the field's range over the tile.  The field is
//      evaluated once (uniform, 64-bit) at the tile's middle voxel c = (y0 + nyv / 2, x0 + nxv / 2).  Inside a cell the
//      exact bilinear value has |du/dy| <= max node difference along y / Sy <= 2^13 per pixel and likewise along x, it is
//      continuous across cells, and the floor shift moves a value by less than 1: |u(p) - u(c)| <= 2^13 (|dy| + |dx|)
//      + 1 with |dy| <= 8 and |dx| <= 32 over the tile.  So sy varies by at most 15 (1 + 1/8) + 63 / 8 = 24.75 px from
//      the matrix and 2 x 40 / 8 = 10 px from the field, 34.75 px: floor(hi) - floor(lo) <= 35, and with the row below
//      the last tap 37 rows; sx by 72.75 + 10 = 82.75 px: 85 bytes.  37 rows of 88 bytes are 3,256 B of LDS.
//   2. stage: the hull as in the affine kernel, and the nodes of the cells the tile meets -- 16 rows meet at most two
//      cell rows (Sy >= 16), 64 columns at most five cell columns (Sx >= 16, any origin): 3 x 6 nodes, stored 3 x 7 so
//      that a thread in the last cell column may read one column further -- clamped to |U| <= 2^21, in LDS.
//   3. resample: a thread's four outputs share the row, so it blends its three node columns along y once, and each
//      output blends two of them along x.  All of it in 32 bits with 24-bit operands (__mul24, full rate), by splitting
//      a node value U = 2^11 h + l, h = U >> 11 in [-2^10, 2^10], l = U & 2047 in [0, 2^11): the weights are at most
//      2^10 and sum to Sy (Sx), so |Ch| = |(Sy - ry) h0 + ry h1| <= 2^20, 0 <= Cl < 2^21, |Nh| = |(Sx - rx) Ch0 + rx Ch1|
//      <= 2^30, 0 <= Nl <= 2^20 (2^11 - 1) < 2^31, every factor below 2^23 in magnitude.  The definition's numerator is
//      N = 2^11 Nh + Nl exactly (the blend is linear in U), and with K = ky + kx (8...20)
//        N >> K = (Nh + (Nl >> 11)) >> (K - 11)   for K >= 11   (nested floor division, Nh an integer)
//               = Nh 2^(11 - K) + (Nl >> K)       for K < 11    (2^11 Nh is a multiple of 2^K; |Nh| <= 2^(K + 10))
//      The position relative to the hull's origin then gains |u| <= 2^21 on the affine kernel's |rel| < 2^29: 32 bits.
// Safety as the affine kernel's: coefficients and node values are clamped to the limits as they are read, lattice
// indices come from the arguments (which the host validated) and are clamped to the lattice, LDS node indices are
// bounded by the tile's geometry, and every tap is clamped to the staged hull.  A device table that breaks the
// difference limit only makes the hull miss taps: wrong bytes, no load outside the block or LDS.
namespace {

constexpr int FLD_MAX = 1 << 21;                       // |U| in 2^-16 px: 32 px
constexpr int FLD_KMIN = 4, FLD_KMAX = 10;             // spacings 16...1024
constexpr int FLD_HY = 37, FLD_HX = 85;                // the hull of a tile's taps at the limits of matrix and field
constexpr int FLD_HDW = (3 + FLD_HX + 3) / 4;
constexpr int FLD_NR = 3, FLD_NC = 7;                  // node rows and columns a tile keeps in LDS
constexpr int64_t FLD_SPREAD = (int64_t)(WARP_TY / 2 + WARP_TX / 2) * WARP_DEV + 1;   // |u(p) - u(middle)| over a tile
static_assert(FLD_HDW <= 32, "a hull row is staged by 32 lanes");
static_assert(FLD_NR * FLD_NC * 2 <= WARP_THREADS, "one thread per node component");

struct field_args {
  warp_args w;
  const int *field;                                    // device: [D][ny][nx][2] = (u_y, u_x) in 2^-16 px
  int ny, nx, ky, kx;
};

__device__ inline int fld_clamp(int v) { return min(max(v, -FLD_MAX), FLD_MAX); }

// the definition, in 64 bits: component `c` of the field of plane `U` at (y, x) -- uniform work, once per workgroup
__device__ inline int64_t fld_at(const int *U, int ny, int nx, int ky, int kx, int64_t y, int64_t x, int c) {
  const int i0 = (int)wp_clamp(y >> ky, 0, ny - 1), i1 = min(i0 + 1, ny - 1);
  const int j0 = (int)wp_clamp(x >> kx, 0, nx - 1), j1 = min(j0 + 1, nx - 1);
  const int64_t Sy = (int64_t)1 << ky, Sx = (int64_t)1 << kx, ry = y & (Sy - 1), rx = x & (Sx - 1);
  const int64_t u00 = fld_clamp(U[((int64_t)i0 * nx + j0) * 2 + c]), u01 = fld_clamp(U[((int64_t)i0 * nx + j1) * 2 + c]);
  const int64_t u10 = fld_clamp(U[((int64_t)i1 * nx + j0) * 2 + c]), u11 = fld_clamp(U[((int64_t)i1 * nx + j1) * 2 + c]);
  return ((Sy - ry) * ((Sx - rx) * u00 + rx * u01) + ry * ((Sx - rx) * u10 + rx * u11)) >> (ky + kx);
}

struct fld_plane {                                     // a workgroup's plane: its clamped map and its tile
  int ayy, ayx, axy, axx;
  int64_t bsy, bsx, y0, x0;                            // the tile's first output in volume coordinates
  int nyv, nxv, d, by0, bx0;
  const int *U;
};

__device__ inline fld_plane fld_setup(const field_args &f) {
  const warp_args &g = f.w;
  fld_plane p;
  p.d = blockIdx.x / g.tiles;
  const int tile = blockIdx.x - p.d * g.tiles, tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
  p.by0 = tyi * WARP_TY, p.bx0 = txi * WARP_TX;
  p.nyv = min(WARP_TY, g.OH - p.by0), p.nxv = min(WARP_TX, g.OW - p.bx0);
  p.y0 = (int64_t)g.oy0 + p.by0, p.x0 = (int64_t)g.ox0 + p.bx0;
  const long long *m = g.maps + 6 * (int64_t)p.d;
  p.ayy = (int)wp_clamp(m[0], WARP_ONE - WARP_DEV, WARP_ONE + WARP_DEV), p.ayx = (int)wp_clamp(m[1], -WARP_DEV, WARP_DEV);
  p.axy = (int)wp_clamp(m[3], -WARP_DEV, WARP_DEV), p.axx = (int)wp_clamp(m[4], WARP_ONE - WARP_DEV, WARP_ONE + WARP_DEV);
  p.bsy = wp_clamp(m[2], -WARP_MAX_B, WARP_MAX_B), p.bsx = wp_clamp(m[5], -WARP_MAX_B, WARP_MAX_B);
  p.U = f.field + (int64_t)p.d * f.ny * f.nx * 2;
  return p;
}

__device__ inline void fld_store(const warp_args &g, const fld_plane &p, int ly, int lx, uint32_t packed) {
  if (ly >= p.nyv || lx >= p.nxv) return;
  uint8_t *o = g.dst + ((int64_t)p.d * g.OH + (p.by0 + ly)) * g.OW + (p.bx0 + lx);
  if (lx + 3 < p.nxv && ((uintptr_t)o & 3) == 0) {
    *(uint32_t *)o = packed;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lx + j < p.nxv) o[j] = (uint8_t)(packed >> (8 * j));
  }
}

template <bool NEAREST, bool BOX>
__global__ __launch_bounds__(WARP_THREADS) void u8_warp_field_k(field_args f) {
  __shared__ uint32_t hull[FLD_HY * FLD_HDW];
  __shared__ int nodes[FLD_NR * FLD_NC * 2];
  const uint8_t *hb = (const uint8_t *)hull;
  const warp_args &g = f.w;
  const int tid = threadIdx.x;
  const fld_plane p = fld_setup(f);
  const int ky = f.ky, kx = f.kx, Sy = 1 << ky, Sx = 1 << kx;
  const int i0 = (int)(p.y0 >> ky), j0 = (int)(p.x0 >> kx);               // the tile's first cell

  // the tile's source range (uniform): the affine extremes plus the field's range about its value at the middle
  const int64_t cy = p.y0 + (p.nyv >> 1), cx = p.x0 + (p.nxv >> 1);
  const int64_t ucy = fld_at(p.U, f.ny, f.nx, ky, kx, cy, cx, 0), ucx = fld_at(p.U, f.ny, f.nx, ky, kx, cy, cx, 1);
  int64_t sylo, syhi, sxlo, sxhi;
  warp_range(p.ayy, p.ayx, p.bsy, p.y0, p.nyv, p.x0, p.nxv, sylo, syhi);
  warp_range(p.axy, p.axx, p.bsx, p.y0, p.nyv, p.x0, p.nxv, sxlo, sxhi);
  sylo += ucy - FLD_SPREAD, syhi += ucy + FLD_SPREAD, sxlo += ucx - FLD_SPREAD, sxhi += ucx + FLD_SPREAD;
  const int64_t FY = 256 * ((int64_t)g.VY - 1), FX = 256 * (g.W - 1);
  const bool any = ((syhi + 128) >> 8) >= 0 && ((sylo + 128) >> 8) <= FY && ((sxhi + 128) >> 8) >= 0 && ((sxlo + 128) >> 8) <= FX;
  const int64_t top = g.sy0 + g.H - 1;
  const int64_t sx0 = BOX ? g.sx0 : 0, BW = BOX ? g.BW : g.W;                       // the block's first column, its row stride
  const int64_t hy0 = wp_clamp(wp_clamp((sylo + 128) >> 16, 0, g.VY - 1), g.sy0, top);
  const int64_t hy1 = wp_clamp(wp_clamp(((syhi + 128) >> 16) + 1, 0, g.VY - 1), hy0, top);
  int64_t hx0 = wp_clamp((sxlo + 128) >> 16, 0, g.W - 1);
  int64_t hx1 = wp_clamp(((sxhi + 128) >> 16) + 1, hx0, g.W - 1);
  if (BOX) hx0 = wp_clamp(hx0, sx0, sx0 + BW - 1), hx1 = wp_clamp(hx1, hx0, sx0 + BW - 1);
  const int nr = (int)wp_min(hy1 - hy0 + 1, FLD_HY), nc = (int)wp_min(hx1 - hx0 + 1, FLD_HX);

  const uint8_t *row0 = g.src + ((int64_t)p.d * g.H + (hy0 - g.sy0)) * BW + (hx0 - sx0);   // the hull's first byte
  const int a0 = (int)((uintptr_t)row0 & 3), w3 = (int)(BW & 3);                   // a row's shift: (a0 + r w3) & 3
  if (any) {
    if (tid < FLD_NR * FLD_NC * 2) {                                               // the nodes of the cells the tile meets
      const int r = tid / (FLD_NC * 2), c = (tid >> 1) % FLD_NC;
      const int i = min(i0 + r, f.ny - 1), j = min(j0 + c, f.nx - 1);
      nodes[tid] = fld_clamp(p.U[((int64_t)i * f.nx + j) * 2 + (tid & 1)]);
    }
    const int k = tid & 31;
    for (int r = tid >> 5; r < nr; r += WARP_THREADS / 32) {
      const int sh = (a0 + r * w3) & 3;
      if (4 * k < sh + nc) hull[r * FLD_HDW + k] = *(const uint32_t *)(row0 + (int64_t)r * BW - sh + 4 * k);
    }
    __syncthreads();
  }
  const int ly = tid >> 4, lx = (tid & 15) * 4;
  if (!any) {                                                                      // uniform: nothing of the tile is inside
    fld_store(g, p, ly, lx, (uint32_t)g.fill * 0x01010101u);
    return;
  }

  // positions relative to the hull's origin, as the affine kernel's
  const int64_t S0y = (int64_t)p.ayy * p.y0 + (int64_t)p.ayx * p.x0 + p.bsy;
  const int64_t S0x = (int64_t)p.axy * p.y0 + (int64_t)p.axx * p.x0 + p.bsx;
  constexpr int64_t FAR = (int64_t)1 << 28;
  const int rely = (int)wp_clamp(S0y - hy0 * 65536, -FAR, FAR), relx = (int)wp_clamp(S0x - hx0 * 65536, -FAR, FAR);
  const int ylo = (int)wp_max(-256 * hy0, -FAR), yhi = (int)wp_min(FY - 256 * hy0, FAR);
  const int xlo = (int)wp_max(-256 * hx0, -FAR), xhi = (int)wp_min(FX - 256 * hx0, FAR);
  const int ylast = (int)wp_min(g.VY - 1 - hy0, FAR), xlast = (int)wp_min(g.W - 1 - hx0, FAR);

  // the thread's row of the lattice: its three node columns blended along y, high and low parts (the proof is above)
  const int64_t y = p.y0 + ly, x = p.x0 + lx;
  const int ri = (int)(y >> ky) - i0, ry = (int)y & (Sy - 1), c0 = (int)(x >> kx) - j0;   // ri in {0, 1}, c0 in 0...4
  int Ch[3][2], Cl[3][2];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int a = nodes[((ri * FLD_NC) + c0 + c) * 2 + e], b = nodes[(((ri + 1) * FLD_NC) + c0 + c) * 2 + e];
      Ch[c][e] = __mul24(Sy - ry, a >> 11) + __mul24(ry, b >> 11);
      Cl[c][e] = __mul24(Sy - ry, a & 2047) + __mul24(ry, b & 2047);
    }
  const int K = ky + kx;
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int rx = (int)(x + j) & (Sx - 1);
    const bool next = (int)((x + j) >> kx) - j0 != c0;                                // the thread's second cell column
    int u[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int h0 = next ? Ch[1][e] : Ch[0][e], h1 = next ? Ch[2][e] : Ch[1][e];
      const int l0 = next ? Cl[1][e] : Cl[0][e], l1 = next ? Cl[2][e] : Cl[1][e];
      const int Nh = __mul24(Sx - rx, h0) + __mul24(rx, h1), Nl = __mul24(Sx - rx, l0) + __mul24(rx, l1);
      u[e] = K >= 11 ? (Nh + (Nl >> 11)) >> (K - 11) : Nh * (1 << (11 - K)) + (Nl >> K);
    }
    const int fy = (rely + p.ayy * ly + p.ayx * (lx + j) + u[0] + 128) >> 8;
    const int fx = (relx + p.axy * ly + p.axx * (lx + j) + u[1] + 128) >> 8;
    const bool inside = fy >= ylo && fy <= yhi && fx >= xlo && fx <= xhi;
    uint32_t v;
    if (NEAREST) {
      const int r = min(max((fy + 128) >> 8, 0), nr - 1), c = min(max((fx + 128) >> 8, 0), nc - 1);
      v = hb[r * (4 * FLD_HDW) + ((a0 + r * w3) & 3) + c];
    } else {
      const int iy = fy >> 8, ix = fx >> 8;
      const uint32_t ty = fy & 255, tx = fx & 255;
      const int r0 = min(max(iy, 0), nr - 1), r1 = min(max(min(iy + 1, ylast), 0), nr - 1);
      const int q0 = min(max(ix, 0), nc - 1), q1 = min(max(min(ix + 1, xlast), 0), nc - 1);
      const uint8_t *p0 = hb + r0 * (4 * FLD_HDW) + ((a0 + r0 * w3) & 3), *p1 = hb + r1 * (4 * FLD_HDW) + ((a0 + r1 * w3) & 3);
      const uint32_t top2 = (256 - tx) * p0[q0] + tx * p0[q1], bot2 = (256 - tx) * p1[q0] + tx * p1[q1];
      v = ((256 - ty) * top2 + ty * bot2 + (1u << 15)) >> 16;
    }
    packed |= (inside ? v : (uint32_t)g.fill) << (8 * j);
  }
  fld_store(g, p, ly, lx, packed);
}

// The baseline: the same tile and store, every output's position from the definition in 64 bits, its taps as byte loads
// from global memory (clamped to the block), its nodes from global memory (clamped to the lattice).  No LDS.
template <bool NEAREST>
__global__ __launch_bounds__(WARP_THREADS) void u8_warp_field_direct_k(field_args f) {
  const warp_args &g = f.w;
  const int tid = threadIdx.x, ly = tid >> 4, lx = (tid & 15) * 4;
  const fld_plane p = fld_setup(f);
  const int64_t FY = 256 * ((int64_t)g.VY - 1), FX = 256 * (g.W - 1), top = g.sy0 + g.H - 1;
  const uint8_t *plane = g.src + (int64_t)p.d * g.H * g.W;
  const int64_t y = wp_min(p.y0 + ly, g.VY - 1);
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t x = wp_min(p.x0 + lx + j, g.W - 1);
    const int64_t sy = p.ayy * y + p.ayx * x + p.bsy + fld_at(p.U, f.ny, f.nx, f.ky, f.kx, y, x, 0);
    const int64_t sx = p.axy * y + p.axx * x + p.bsx + fld_at(p.U, f.ny, f.nx, f.ky, f.kx, y, x, 1);
    const int64_t fy = (sy + 128) >> 8, fx = (sx + 128) >> 8;
    const bool inside = fy >= 0 && fy <= FY && fx >= 0 && fx <= FX;
    const int64_t gy = wp_clamp(fy, 0, FY), gx = wp_clamp(fx, 0, FX);
    uint32_t v;
    if (NEAREST) {
      v = plane[(wp_clamp((gy + 128) >> 8, g.sy0, top) - g.sy0) * g.W + ((gx + 128) >> 8)];
    } else {
      const int64_t iy = gy >> 8, ix = gx >> 8;
      const uint32_t ty = gy & 255, tx = gx & 255;
      const uint8_t *p0 = plane + (wp_clamp(iy, g.sy0, top) - g.sy0) * g.W;
      const uint8_t *p1 = plane + (wp_clamp(wp_min(iy + 1, g.VY - 1), g.sy0, top) - g.sy0) * g.W;
      const int64_t ix1 = wp_min(ix + 1, g.W - 1);
      const uint32_t top2 = (256 - tx) * p0[ix] + tx * p0[ix1], bot2 = (256 - tx) * p1[ix] + tx * p1[ix1];
      v = ((256 - ty) * top2 + ty * bot2 + (1u << 15)) >> 16;
    }
    packed |= (inside ? v : (uint32_t)g.fill) << (8 * j);
  }
  fld_store(g, p, ly, lx, packed);
}

// The checks of every entry, and the launch arguments.  The source block is the rows [sy0, sy0 + BH) and the columns
// [sx0, sx0 + BW) of D sections of VY x VX; the entries that take whole rows give sx0 = 0 and BW = VX, for which the
// column rule below holds by itself (fx is cut to the section).  `field`: the map plus a displacement field, else
// field_host, field_dev, ny, nx, ky and kx are not looked at.
int warp_check(const uint8_t *src, int32_t D, int32_t BH, int32_t BW, int32_t sy0, int32_t sx0, int32_t VY, int32_t VX,
               uint8_t *dst, int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
               const int64_t *maps_dev, bool field, const int32_t *field_host, const int32_t *field_dev, int32_t ny, int32_t nx,
               int32_t ky, int32_t kx, int32_t fill, int32_t nearest, field_args &f) {
  if (!src || !dst || !maps_host || !maps_dev || D < 1 || BH < 1 || BW < 1 || VY < 1 || VX < 1 || OD != D || OH < 1 || OW < 1 ||
      sy0 < 0 || sx0 < 0 || oy0 < 0 || ox0 < 0 || fill < 0 || fill > 255 || (nearest != 0 && nearest != 1))
    return TEM_EINVAL;
  if ((int64_t)sy0 + BH > VY || (int64_t)sx0 + BW > VX || (int64_t)oy0 + OH > VY || (int64_t)ox0 + OW > VX) return TEM_EINVAL;
  if (field) {
    if (!field_host || !field_dev) return TEM_EINVAL;
    if (ky < FLD_KMIN || ky > FLD_KMAX || kx < FLD_KMIN || kx > FLD_KMAX) return TEM_EINVAL;
    if (ny != ((VY - 1) >> ky) + 2 || nx != ((VX - 1) >> kx) + 2) return TEM_EINVAL;
  }
  const int64_t tiles_x = ((int64_t)OW + WARP_TX - 1) / WARP_TX, tiles_y = ((int64_t)OH + WARP_TY - 1) / WARP_TY;
  if (tiles_x * tiles_y > WARP_MAX_WGS || tiles_x * tiles_y * D > WARP_MAX_WGS) return TEM_EINVAL;
  const int64_t FY = 256 * ((int64_t)VY - 1), FX = 256 * ((int64_t)VX - 1);
  for (int64_t d = 0; d < D; ++d) {
    const int64_t *m = maps_host + 6 * d;
    if (m[0] < WARP_ONE - WARP_DEV || m[0] > WARP_ONE + WARP_DEV || m[4] < WARP_ONE - WARP_DEV || m[4] > WARP_ONE + WARP_DEV ||
        m[1] < -WARP_DEV || m[1] > WARP_DEV || m[3] < -WARP_DEV || m[3] > WARP_DEV || m[2] < -WARP_MAX_B || m[2] > WARP_MAX_B ||
        m[5] < -WARP_MAX_B || m[5] > WARP_MAX_B)
      return TEM_EINVAL;
    int64_t ulo[2] = {0, 0}, uhi[2] = {0, 0};
    if (field) {
      const int64_t dymax = (int64_t)WARP_DEV << ky, dxmax = (int64_t)WARP_DEV << kx;
      const int32_t *U = field_host + d * ny * nx * 2;
      for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j)
          for (int e = 0; e < 2; ++e) {
            const int64_t u = U[((int64_t)i * nx + j) * 2 + e];
            if (u < -FLD_MAX || u > FLD_MAX) return TEM_EINVAL;
            if (i + 1 < ny && std::llabs((int64_t)U[((int64_t)(i + 1) * nx + j) * 2 + e] - u) > dymax) return TEM_EINVAL;
            if (j + 1 < nx && std::llabs((int64_t)U[((int64_t)i * nx + j + 1) * 2 + e] - u) > dxmax) return TEM_EINVAL;
          }
      // the least and largest node of the cells the block meets (the interpolated value lies between them; every shift
      // is monotone)
      const int ia = oy0 >> ky, ib = ((oy0 + OH - 1) >> ky) + 1, ja = ox0 >> kx, jb = ((ox0 + OW - 1) >> kx) + 1;
      ulo[0] = ulo[1] = FLD_MAX, uhi[0] = uhi[1] = -FLD_MAX;
      for (int i = ia; i <= ib; ++i)
        for (int j = ja; j <= jb; ++j)
          for (int e = 0; e < 2; ++e) {
            const int64_t u = U[((int64_t)i * nx + j) * 2 + e];
            ulo[e] = wp_min(ulo[e], u), uhi[e] = wp_max(uhi[e], u);
          }
    }
    // the rows and columns that the block's inside voxels can read with a weight above 0: the affine extremes at its
    // corners plus the field's range, cut to the section
    int64_t sylo, syhi, sxlo, sxhi;
    warp_range(m[0], m[1], m[2], oy0, OH, ox0, OW, sylo, syhi);
    warp_range(m[3], m[4], m[5], oy0, OH, ox0, OW, sxlo, sxhi);
    sylo += ulo[0], syhi += uhi[0], sxlo += ulo[1], sxhi += uhi[1];
    const int64_t fylo = wp_max((sylo + 128) >> 8, 0), fyhi = wp_min((syhi + 128) >> 8, FY);
    const int64_t fxlo = wp_max((sxlo + 128) >> 8, 0), fxhi = wp_min((sxhi + 128) >> 8, FX);
    if (fylo > fyhi || fxlo > fxhi) continue;                                                     // every voxel is outside
    const int64_t lo = nearest ? (fylo + 128) >> 8 : fylo >> 8;
    const int64_t hi = nearest ? (fyhi + 128) >> 8 : (fyhi >> 8) + ((fyhi & 255) ? 1 : 0);
    if (lo < sy0 || hi >= (int64_t)sy0 + BH) return TEM_EINVAL;
    const int64_t cl = nearest ? (fxlo + 128) >> 8 : fxlo >> 8;
    const int64_t ch = nearest ? (fxhi + 128) >> 8 : (fxhi >> 8) + ((fxhi & 255) ? 1 : 0);
    if (cl < sx0 || ch >= (int64_t)sx0 + BW) return TEM_EINVAL;
  }
  warp_args &g = f.w;
  g.src = src, g.H = BH, g.W = VX, g.sy0 = sy0, g.VY = VY, g.BW = BW, g.sx0 = sx0;
  g.dst = dst, g.OH = OH, g.OW = OW, g.oy0 = oy0, g.ox0 = ox0;
  g.tiles_x = (int)tiles_x, g.tiles = (int)(tiles_x * tiles_y);
  g.maps = (const long long *)maps_dev, g.fill = fill;
  f.field = field ? field_dev : nullptr, f.ny = ny, f.nx = nx, f.ky = ky, f.kx = kx;
  return TEM_OK;
}

}  // namespace

extern "C" int tem_u8_warp_affine(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY, uint8_t *dst,
                                  int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
                                  const int64_t *maps_dev, int32_t fill, int32_t nearest, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  field_args f;
  const int rc = warp_check(src, D, H, W, sy0, 0, VY, W, dst, OD, OH, OW, oy0, ox0, maps_host, maps_dev, false, nullptr, nullptr,
                            0, 0, 0, 0, fill, nearest, f);
  if (rc != TEM_OK) return rc;
  const unsigned wgs = (unsigned)(f.w.tiles * (int64_t)D);
  if (nearest)
    hipLaunchKernelGGL((u8_warp_affine_k<true, false>), dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, f.w);
  else
    hipLaunchKernelGGL((u8_warp_affine_k<false, false>), dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, f.w);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_warp_field(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY, uint8_t *dst,
                                 int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
                                 const int64_t *maps_dev, const int32_t *field_host, const int32_t *field_dev, int32_t ny,
                                 int32_t nx, int32_t ky, int32_t kx, int32_t fill, int32_t nearest, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  field_args f;
  const int rc = warp_check(src, D, H, W, sy0, 0, VY, W, dst, OD, OH, OW, oy0, ox0, maps_host, maps_dev, true, field_host,
                            field_dev, ny, nx, ky, kx, fill, nearest, f);
  if (rc != TEM_OK) return rc;
  const unsigned wgs = (unsigned)(f.w.tiles * (int64_t)D);
  if (nearest)
    hipLaunchKernelGGL((u8_warp_field_k<true, false>), dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, f);
  else
    hipLaunchKernelGGL((u8_warp_field_k<false, false>), dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, f);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_warp_field_direct(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY,
                                        uint8_t *dst, int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0,
                                        const int64_t *maps_host, const int64_t *maps_dev, const int32_t *field_host,
                                        const int32_t *field_dev, int32_t ny, int32_t nx, int32_t ky, int32_t kx, int32_t fill,
                                        int32_t nearest, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  field_args f;
  const int rc = warp_check(src, D, H, W, sy0, 0, VY, W, dst, OD, OH, OW, oy0, ox0, maps_host, maps_dev, true, field_host,
                            field_dev, ny, nx, ky, kx, fill, nearest, f);
  if (rc != TEM_OK) return rc;
  const unsigned wgs = (unsigned)(f.w.tiles * (int64_t)D);
  if (nearest)
    hipLaunchKernelGGL(u8_warp_field_direct_k<true>, dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, f);
  else
    hipLaunchKernelGGL(u8_warp_field_direct_k<false>, dim3(wgs), dim3(WARP_THREADS), 0, (hipStream_t)stream, f);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_warp_box(const uint8_t *src, int32_t D, int32_t BH, int32_t BW, int32_t sy0, int32_t sx0, int32_t VY,
                               int32_t VX, uint8_t *dst, int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0,
                               const int64_t *maps_host, const int64_t *maps_dev, const int32_t *field_host,
                               const int32_t *field_dev, int32_t ny, int32_t nx, int32_t ky, int32_t kx, int32_t fill,
                               int32_t nearest, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  const bool field = field_host || field_dev;                  // both null: the affine definition; one null is refused
  field_args f;
  const int rc = warp_check(src, D, BH, BW, sy0, sx0, VY, VX, dst, OD, OH, OW, oy0, ox0, maps_host, maps_dev, field, field_host,
                            field_dev, ny, nx, ky, kx, fill, nearest, f);
  if (rc != TEM_OK) return rc;
  const dim3 wgs((unsigned)(f.w.tiles * (int64_t)D)), threads(WARP_THREADS);
  if (field && nearest)
    hipLaunchKernelGGL((u8_warp_field_k<true, true>), wgs, threads, 0, (hipStream_t)stream, f);
  else if (field)
    hipLaunchKernelGGL((u8_warp_field_k<false, true>), wgs, threads, 0, (hipStream_t)stream, f);
  else if (nearest)
    hipLaunchKernelGGL((u8_warp_affine_k<true, true>), wgs, threads, 0, (hipStream_t)stream, f.w);
  else
    hipLaunchKernelGGL((u8_warp_affine_k<false, true>), wgs, threads, 0, (hipStream_t)stream, f.w);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
