// clahe_u8.hip -- contrast-limited adaptive histogram equalisation of uint8 sections, the two device passes:
//   tem_u8_hist_tiles   counts[z][i][j][v] += occurrences of byte value v in tile (i, j) of section z
//   tem_u8_clahe        buf[z][y][x] = bilinear interpolation, between the four nearest tile centres, of the tiles'
//                       tables at buf[z][y][x], in place, in integers
// The tables between the two (clip, redistribute, cumulate) are host work on a few kilobytes per tile.  The tile grid
// is anchored at (0, 0) of the caller's VOLUME; a call covers a dense block of it whose voxel (d, y, x) sits at
// in-plane volume coordinates (y_org + y, x_org + x), so a voxel's result never depends on how the volume was cut.
//
// Both kernels walk rows the way hist_u8.hip does: a row piece is cut at 16-byte ADDRESS boundaries, a segment that
// lies wholly inside the piece travels as one dwordx4, its cut head and tail byte by byte, the valid bytes only.  A piece never crosses a
// tile (histograms) or an interpolation cell (remap), so a 16-byte line that spans two of them is split into two cut
// segments.  Nothing outside the block is read, and the remap writes exactly the bytes it read.
//
// tem_u8_hist_tiles.  A unit of work is (section, tile, run of rows of that tile); the units, that run fastest, are
// dealt in contiguous ranges to at most HT_MAX_GRID workgroups.  Counters are private to the workgroup, u8_hist_k's
// scheme: 32 copies of a 256-bin histogram in LDS laid out [bin][copy], a lane adding into copy (lane & 31), so the 32
// lanes of a half wave hit 32 different banks whatever the bytes are -- a constant tile costs what a random one does.
// The workgroup flushes where the (section, tile) of its units changes and at its end: thread t sums the 32 copies of
// bin t and, if the sum is not zero, adds it to counts with ONE 32-bit global atomic (an ordinary vector atomic);
// the flush clears the copies for the next tile.  Calls add, and two workgroups may share a tile, so slabs that cut a
// tile between rows accumulate into the same counters.  A 32-bit counter cannot wrap within a call: a tile holds at
// most 2048 x 2048 voxels.
//
// tem_u8_clahe.  The centres of the tiles cut a section into interpolation cells: cell (cy, cx) holds the voxels whose
// four nearest centres are those of tiles (cy - 1 | cy, cx - 1 | cx), clamped to the grid (cells 0 and gy / gx are the
// half tiles along the faces), rows [(cy - 1) th + th / 2, cy th + th / 2).  A workgroup takes a run of rows of one
// cell of one section.  It stages the four tables in LDS once as ONE packed word per value, a | b << 8 | c << 16 |
// d << 24 (1 KiB), so a voxel costs one ds_read_b32, then
//   num = (2 th - wy) ((2 tw - wx) a + wx b) + wy ((2 tw - wx) c + wx d) + D / 2,   D = 4 th tw,   out = num / D.
// num < 2^32 for th, tw <= 2048 (at most 255 D + D / 2 = 4 286 578 688).  The division is a multiplication by
// M = ceil(2^56 / D) and a shift by 56: num M / 2^56 - num / D < num / 2^56 < 1 / D (num D < 2^56), and num / D falls
// short of the next integer by at least 1 / D, so the floor is exact for every num below 2^32 and every D up to 2^24.
// M has up to 55 bits; the product is taken in two halves, (num Mhi + umulhi(num, Mlo)) >> 24.  Tiles whose sides are
// powers of two (the default, 128) divide by a shift instead.
// The LDS read is data dependent: word v lies in bank v mod 32, so the lanes of a half wave conflict where their
// bytes differ by a multiple of 32, and equal bytes broadcast (see DESIGN.md for why one copy is kept).
#include "tem_common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int HT_COPIES = 32;
constexpr int HT_MAX_GRID = 1024;          // 4 workgroups of 32 KiB LDS on each of 256 CUs
constexpr int CL_MAX_TILE = 2048;
constexpr int HT_ITEMS = 4096;             // 16-byte segments per unit of the histogram, about
constexpr int CL_ITEMS = 2048;             // 16-byte segments per workgroup of the remap, about

// The n < 16 valid bytes of a cut segment at p, packed like the dwordx4 of a whole one (the rest zero): 16 predicated
// byte loads that are all in flight at once, where a loop over the bytes would wait for each in turn -- tiles and cells
// cut two segments out of every row piece, far more than the one head and tail of a section.
__device__ __forceinline__ void load_cut(const uint8_t *p, int n, uint32_t (&w)[4]) {
  w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < n) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}

__device__ __forceinline__ void ht_add(uint32_t *h, uint32_t byte, uint32_t copy) {
  atomicAdd(&h[byte * HT_COPIES + copy], 1u);
}

// thread t: bin t of the workgroup's copies -> counts[t]; `clear` leaves the copies zero for the next tile
__device__ __forceinline__ void ht_flush(uint32_t *h, uint32_t *counts, bool clear) {
  __syncthreads();
  const uint32_t t = threadIdx.x;
  uint32_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < HT_COPIES; ++j) {
    const uint32_t a = t * HT_COPIES + ((j + t) & (HT_COPIES - 1));
    s += h[a];
    if (clear) h[a] = 0;
  }
  if (s) atomicAdd(counts + t, s);
  if (clear) __syncthreads();
}

// Unit u = key * parts + part, key = (d * nty + ti) * ntx + tj: rows [part * rpp, (part + 1) * rpp) of the part of tile
// (ti0 + ti, tj0 + tj) that lies in section d of the block.  S: segments per row piece, an upper bound of
// ceil(((address & 15) + width) / 16) over all alignments; magicS = magic_for(S).
__global__ __launch_bounds__(CL_THREADS) void u8_hist_tiles_k(const uint8_t *src, int64_t H, int64_t W, int64_t y_org,
                                                              int64_t x_org, int64_t th, int64_t tw, int64_t gy,
                                                              int64_t gx, int64_t ti0, int64_t tj0, int64_t nty,
                                                              int64_t ntx, int64_t parts, int64_t rpp, uint32_t S,
                                                              uint32_t magicS, int64_t nunits, int64_t upw,
                                                              uint32_t *counts) {
  __shared__ uint32_t h[256 * HT_COPIES];
  for (int i = threadIdx.x; i < 256 * HT_COPIES; i += CL_THREADS) h[i] = 0;
  __syncthreads();
  const uint32_t copy = threadIdx.x & (HT_COPIES - 1);
  const int64_t u1 = min(((int64_t)blockIdx.x + 1) * upw, nunits);
  int64_t cur = -1;                                                      // the key the copies count for
  uint32_t *dst = counts;
  for (int64_t u = (int64_t)blockIdx.x * upw; u < u1; ++u) {
    const int64_t key = u / parts, part = u - key * parts;
    const int64_t dt = key / ntx, tj = tj0 + (key - dt * ntx), d = dt / nty, ti = ti0 + (dt - d * nty);
    if (key != cur) {
      if (cur >= 0) ht_flush(h, dst, true);
      cur = key;
      dst = counts + ((d * gy + ti) * gx + tj) * 256;
    }
    const int64_t ya = max(ti * th - y_org, (int64_t)0) + part * rpp;
    const int64_t yb = min(min((ti + 1) * th - y_org, H), ya + rpp);
    const int64_t xa = max(tj * tw - x_org, (int64_t)0), xb = min((tj + 1) * tw - x_org, W);
    if (ya >= yb || xa >= xb) continue;                                  // the tail part of a tile the block cuts
    const int64_t width = xb - xa;
    const uint8_t *first = src + (d * H + ya) * W + xa;
    const uint32_t total = (uint32_t)(yb - ya) * S;                      // <= 2048 rows of <= 130 segments
    for (uint32_t i = threadIdx.x; i < total; i += CL_THREADS) {
      const uint32_t ri = S == 1 ? i : __umulhi(i, magicS), s = i - ri * S;
      const uint8_t *row = first + (int64_t)ri * W;
      const int64_t m = (int64_t)((uintptr_t)row & 15);                  // the piece starts m bytes into a 16-byte line
      const int64_t lo = max((int64_t)16 * s - m, (int64_t)0), hi = min((int64_t)16 * s + 16 - m, width);
      const int n = (int)(hi - lo);
      uint32_t w[4];
      if (n == 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + lo);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else {
        load_cut(row + lo, n, w);
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < n) ht_add(h, (w[k >> 2] >> (8 * (k & 3))) & 255u, copy);
    }
  }
  if (cur >= 0) ht_flush(h, dst, false);
}

// ------------------------------------------------------------------------------------------------------------ remap
struct ClaheDiv { uint32_t mhi, mlo, half, shift; };      // M = ceil(2^56 / D) in two halves, D / 2, log2(D)

// one voxel: t = the packed tables at its value, A = 2 th - wy, B = wy, Q = wx, tw2 = 2 tw.  Every factor is below 2^24
// (weights <= 4096, table entries <= 255, the inner sums <= 4096 * 255) and every product below 2^32, so the six
// multiplications are the full-rate 24-bit ones.  POW2: th and tw are powers of two, and so is D: a shift divides.
template <bool POW2>
__device__ __forceinline__ uint32_t clahe_px(uint32_t t, uint32_t A, uint32_t B, uint32_t Q, uint32_t tw2, ClaheDiv dv) {
  const uint32_t P = tw2 - Q;
  const uint32_t top = __umul24(P, t & 255u) + __umul24(Q, (t >> 8) & 255u);
  const uint32_t bot = __umul24(P, (t >> 16) & 255u) + __umul24(Q, t >> 24);
  const uint32_t num = __umul24(A, top) + __umul24(B, bot) + dv.half;
  if (POW2) return num >> dv.shift;
  return (uint32_t)(((uint64_t)num * dv.mhi + __umulhi(num, dv.mlo)) >> 24);
}

// Block b = ((d * ncy + cyi) * ncx + cxi) * parts + part: rows [part * rpp, (part + 1) * rpp) of the part of cell
// (cy0 + cyi, cx0 + cxi) that lies in section d of the block.
template <bool POW2>
__global__ __launch_bounds__(CL_THREADS) void u8_clahe_k(uint8_t *buf, int64_t H, int64_t W, int64_t zsec0, int64_t y_org,
                                                         int64_t x_org, const uint8_t *tables, int64_t gy, int64_t gx,
                                                         int64_t th, int64_t tw, int64_t cy0, int64_t cx0, uint32_t ncy,
                                                         uint32_t ncx, uint32_t parts, int64_t rpp, uint32_t S,
                                                         uint32_t magicS, ClaheDiv dv) {
  __shared__ uint32_t t4[256];
  uint32_t b = blockIdx.x;
  const uint32_t part = b % parts;
  b /= parts;
  const uint32_t cxi = b % ncx;
  b /= ncx;
  const uint32_t cyi = b % ncy;
  const int64_t d = b / ncy, cy = cy0 + cyi, cx = cx0 + cxi;
  const int64_t ya = max((cy - 1) * th + th / 2 - y_org, (int64_t)0) + (int64_t)part * rpp;
  const int64_t yb = min(min(cy * th + th / 2 - y_org, H), ya + rpp);
  const int64_t xa = max((cx - 1) * tw + tw / 2 - x_org, (int64_t)0), xb = min(cx * tw + tw / 2 - x_org, W);
  if (ya >= yb || xa >= xb) return;                                      // the whole workgroup: nothing staged
  {
    const int64_t i0 = min(max(cy - 1, (int64_t)0), gy - 1), i1 = min(cy, gy - 1);
    const int64_t j0 = min(max(cx - 1, (int64_t)0), gx - 1), j1 = min(cx, gx - 1);
    const uint8_t *sec = tables + (zsec0 + d) * gy * gx * 256 + threadIdx.x;
    t4[threadIdx.x] = (uint32_t)sec[(i0 * gx + j0) * 256] | ((uint32_t)sec[(i0 * gx + j1) * 256] << 8) |
                      ((uint32_t)sec[(i1 * gx + j0) * 256] << 16) | ((uint32_t)sec[(i1 * gx + j1) * 256] << 24);
  }
  __syncthreads();
  const int64_t width = xb - xa;
  uint8_t *first = buf + (d * H + ya) * W + xa;
  const uint32_t th2 = (uint32_t)(2 * th), tw2 = (uint32_t)(2 * tw);
  const uint32_t wy0 = (uint32_t)(2 * (y_org + ya) + 1 - th - (cy - 1) * 2 * th);     // in [0, 2 th): row ya of the cell
  const uint32_t wx0 = (uint32_t)(2 * (x_org + xa) + 1 - tw - (cx - 1) * 2 * tw);     // in [0, 2 tw): column xa
  const uint32_t total = (uint32_t)(yb - ya) * S;
  for (uint32_t i = threadIdx.x; i < total; i += CL_THREADS) {
    const uint32_t ri = S == 1 ? i : __umulhi(i, magicS), s = i - ri * S;
    uint8_t *row = first + (int64_t)ri * W;
    const int64_t m = (int64_t)((uintptr_t)row & 15);
    const int64_t lo = max((int64_t)16 * s - m, (int64_t)0), hi = min((int64_t)16 * s + 16 - m, width);
    const uint32_t B = wy0 + 2 * ri, A = th2 - B, q0 = wx0 + 2 * (uint32_t)lo;
    const int n = (int)(hi - lo);
    uint32_t w[4];
    if (n == 16) {
      const uint4 v = *reinterpret_cast<const uint4 *>(row + lo);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
      load_cut(row + lo, n, w);                                          // the bytes past n: zeros, mapped and dropped
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o |= clahe_px<POW2>(t4[(w[j] >> (8 * k)) & 255u], A, B, q0 + 2 * (4 * j + k), tw2, dv) << (8 * k);
      w[j] = o;
    }
    if (n == 16) {
      *reinterpret_cast<uint4 *>(row + lo) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < n) row[lo + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// what both entry points refuse: the geometry of a block on a tile grid
bool clahe_geometry_ok(int32_t D, int32_t H, int32_t W, int32_t y_org, int32_t x_org, int32_t th, int32_t tw, int32_t gy,
                       int32_t gx) {
  return D >= 1 && H >= 1 && W >= 1 && th >= 1 && th <= CL_MAX_TILE && tw >= 1 && tw <= CL_MAX_TILE && gy >= 1 &&
         gx >= 1 && y_org >= 0 && x_org >= 0 && (int64_t)y_org + H <= (int64_t)gy * th &&
         (int64_t)x_org + W <= (int64_t)gx * tw;
}

}  // namespace

extern "C" int tem_u8_hist_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t y_org, int32_t x_org,
                                 int32_t th, int32_t tw, int32_t gy, int32_t gx, uint32_t *counts, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !counts || ((uintptr_t)counts & 3) || !clahe_geometry_ok(D, H, W, y_org, x_org, th, tw, gy, gx))
    return TEM_EINVAL;
  const int64_t ti0 = y_org / th, tj0 = x_org / tw;
  const int64_t nty = ((int64_t)y_org + H - 1) / th - ti0 + 1, ntx = ((int64_t)x_org + W - 1) / tw - tj0 + 1;
  const int64_t rows = th < H ? th : H, width = tw < W ? tw : W;        // of a tile's part in the block, at most
  const int64_t S = (width + 30) / 16;                                   // segments per row piece, any alignment
  const int64_t rpp = HT_ITEMS / S > 1 ? HT_ITEMS / S : 1;
  const int64_t parts = (rows + rpp - 1) / rpp;
  const int64_t nunits = (int64_t)D * nty * ntx * parts;                 // < 2^31 * 2^31 * 2^11
  const int64_t grid0 = nunits < HT_MAX_GRID ? nunits : HT_MAX_GRID;
  const int64_t upw = (nunits + grid0 - 1) / grid0;
  const int64_t grid = (nunits + upw - 1) / upw;
  hipLaunchKernelGGL(u8_hist_tiles_k, dim3((unsigned)grid), dim3(CL_THREADS), 0, (hipStream_t)stream, src, (int64_t)H,
                     (int64_t)W, (int64_t)y_org, (int64_t)x_org, (int64_t)th, (int64_t)tw, (int64_t)gy, (int64_t)gx, ti0,
                     tj0, nty, ntx, parts, rpp, (uint32_t)S, magic_for((int)S), nunits, upw, counts);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_clahe(uint8_t *buf, int32_t D, int32_t H, int32_t W, int32_t zsec0, int32_t y_org, int32_t x_org,
                            const uint8_t *tables, int32_t gy, int32_t gx, int32_t th, int32_t tw, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!buf || !tables || zsec0 < 0 || !clahe_geometry_ok(D, H, W, y_org, x_org, th, tw, gy, gx)) return TEM_EINVAL;
  // cell of row y: floor((2 y + 1 - th) / (2 th)) + 1 = (2 y + 1 + th) / (2 th), in [0, gy]
  const int64_t cy0 = (2 * (int64_t)y_org + 1 + th) / (2 * (int64_t)th);
  const int64_t cx0 = (2 * (int64_t)x_org + 1 + tw) / (2 * (int64_t)tw);
  const int64_t ncy = (2 * ((int64_t)y_org + H - 1) + 1 + th) / (2 * (int64_t)th) - cy0 + 1;
  const int64_t ncx = (2 * ((int64_t)x_org + W - 1) + 1 + tw) / (2 * (int64_t)tw) - cx0 + 1;
  const int64_t rows = th < H ? th : H, width = tw < W ? tw : W;        // of a cell's part in the block, at most
  const int64_t S = (width + 30) / 16;
  const int64_t rpp = CL_ITEMS / S > 1 ? CL_ITEMS / S : 1;
  const int64_t parts = (rows + rpp - 1) / rpp;
  if (ncy * ncx > 0x7fffffff || (int64_t)D * parts > 0x7fffffff || (int64_t)D * ncy * ncx * parts > 0x7fffffff)
    return TEM_EUNSUPPORTED;
  const uint64_t Dv = 4ull * (uint64_t)th * (uint64_t)tw;
  const uint64_t M = ((1ull << 56) + Dv - 1) / Dv;
  const bool pow2 = !(Dv & (Dv - 1));
  const ClaheDiv dv{(uint32_t)(M >> 32), (uint32_t)M, (uint32_t)(Dv / 2), (uint32_t)__builtin_ctzll(Dv)};
  const auto kernel = pow2 ? u8_clahe_k<true> : u8_clahe_k<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((int64_t)D * ncy * ncx * parts)), dim3(CL_THREADS), 0,
                     (hipStream_t)stream, buf, (int64_t)H, (int64_t)W, (int64_t)zsec0, (int64_t)y_org, (int64_t)x_org,
                     tables, (int64_t)gy, (int64_t)gx, (int64_t)th, (int64_t)tw, cy0, cx0, (uint32_t)ncy, (uint32_t)ncx,
                     (uint32_t)parts, rpp, (uint32_t)S, magic_for((int)S), dv);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
