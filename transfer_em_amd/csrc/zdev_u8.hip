// zdev_u8.hip -- damaged voxels below the tile: how far a voxel of a uint8 section lies outside the range of the voxels
// below and above it in the nearest good sections (utils.section_outlier_sums -> outlier_thresholds ->
// volume_outliers -> find_debris).  The definition is in include/tem_hip.h:
//   e = |v - median(a, v, b)|,  a = V[lo][y][x], v = V[z][y][x], b = V[hi][y][x], (lo, hi) = nbr[z];  0 without a verdict
//   tem_u8_zdev_tiles    sums[d - c0][i][j][0..1] += sum e, count over the voxels of tile (i, j) of core plane d
//   tem_u8_zdev_mask     dst = 1 where 256 Ws > thr[i][j] c, Ws the sum of e over a (2 r + 1)^2 window cut to the
//                        section and c the window's voxels, or where tiles[z][i][j] is set; else 0
//
// The median of three bytes is min(max(v, min(a, b)), max(a, b)).  A word's four bytes are taken as two pairs of 16-bit
// lanes (the even bytes, the odd bytes), so that the median of two voxels costs four packed 16-bit min / max
// (v_pk_min_u16, v_pk_max_u16); sum |v - m| over a pair of lanes is one v_sad_u8 (the lanes' high bytes are zero).
//
// tem_u8_zdev_tiles is tem_u8_zcorr_tiles' kernel (zcorr_u8.hip) with another body: the same parts -- up to ZD_ITEMS
// 16-byte pieces of the part of one tile that lies in the block, ZD_K pieces per thread -- the same runs of up to `zr`
// core planes, the same loads (zc_pieces.h) and the same reduction: wave sums, widened in LDS, ONE 64-bit global atomic
// add (an ordinary vector atomic) per workgroup, plane and quantity.  A thread holds three planes' words of its pieces:
// A of plane `ha`, V of `hv`, B of `hb`.  The next plane's (lo, z, hi) is the same for every thread (read through
// readfirstlane, so the choices are scalar branches), and a plane that is already held is moved, not loaded: a table
// of consecutive sections loads one plane per plane counted, and two more per run.  Every plane index read from the
// device's table is clamped into the block, so a table that disagrees with the host's gives other sums and never a
// read outside the block.  A thread sums at most 64 voxels of a plane, each at most 255: below 2^14; a wave below 2^20.
//
// tem_u8_zdev_mask has tem_u8_ssim's shape (ssim_u8.hip).  A workgroup of 256 threads owns a run of up to ZDM_MAX_RUN
// tiles of ZDM_TY x ZDM_TX = 8 x 32 outputs of one plane, and per tile one output per thread:
//   1. stage: e of the (8 + 2 r) x (32 + 2 r) patch under the tile's windows goes to LDS as bytes, four at a time: a
//      thread loads up to four bytes of a row of each of the three planes as the (up to two) naturally aligned words
//      that hold them -- the planes' rows have their own alignment --, takes the four deviations in packed 16-bit and
//      stores one word.  Positions outside the section hold 0; no byte outside the block is read.
//   2. row sums along x: 2 r + 1 bytes, at most 15 x 255 = 3825, in 16 bits.
//   3. column sums along y: 2 r + 1 row sums, Ws <= 225 x 255 = 57,375.
// c is geometry.  256 Ws <= 14,688,000 and thr c <= 65280 x 225 = 14,688,000: both below 2^24.  A thread counts the
// ones it wrote over its run, the wave sums meet in LDS, and ONE 64-bit global atomic add per workgroup adds them to
// `count`: adds to one address go one after the other (about 12 ns each, measured), so a workgroup per tile would
// spend 3 ms on a slab of 254,000 tiles that are all flagged; the run -- as long as leaves about ZDM_WANT_GRID
// workgroups -- makes that one add per run.  A section without a verdict stages nothing.
#include "zc_pieces.h"

namespace {

constexpr int ZD_K = 4;                          // pieces per thread
constexpr int ZD_ITEMS = ZC_THREADS * ZD_K;      // pieces per part, at most
constexpr int ZD_MAX_RUN = 16;                   // planes per run, at most
constexpr int ZD_MAX_LAG = 8;                    // z - lo and hi - z, at most
constexpr int ZD_MAX_RADIUS = 7;
constexpr int ZD_MAX_THR = 65280;                // 255 x 256
constexpr int64_t ZD_MAX_WGS = (int64_t)1 << 24; // workgroups of one launch: their 256 threads stay below 2^32
constexpr int ZDM_TY = 8, ZDM_TX = 32;           // outputs per workgroup, (y, x): one per thread
constexpr int ZDM_THREADS = ZDM_TY * ZDM_TX;
constexpr int ZDM_WANT_GRID = 8192;              // workgroups the run length aims at (32 on each of 256 CUs)
constexpr int ZDM_MAX_RUN = 64;                  // tiles per workgroup, at most

typedef unsigned short zd_u16x2 __attribute__((ext_vector_type(2)));

// The median of (a, v, b) in each of two 16-bit lanes.
__device__ __forceinline__ uint32_t zd_median(uint32_t a, uint32_t v, uint32_t b) {
  const zd_u16x2 A = __builtin_bit_cast(zd_u16x2, a), V = __builtin_bit_cast(zd_u16x2, v);
  const zd_u16x2 B = __builtin_bit_cast(zd_u16x2, b);
  const zd_u16x2 lo = __builtin_elementwise_min(A, B), hi = __builtin_elementwise_max(A, B);
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(V, lo), hi));
}

// sum |v - median(a, v, b)| over the four bytes of a word, added to acc.
__device__ __forceinline__ uint32_t zd_dev_sum(uint32_t a, uint32_t v, uint32_t b, uint32_t acc) {
  const uint32_t m = 0x00FF00FFu;
  const uint32_t ve = v & m, vo = (v >> 8) & m;
  acc = __builtin_amdgcn_sad_u8(ve, zd_median(a & m, ve, b & m), acc);
  return __builtin_amdgcn_sad_u8(vo, zd_median((a >> 8) & m, vo, (b >> 8) & m), acc);
}

// |v - median(a, v, b)| of the four bytes of a word, byte by byte.
__device__ __forceinline__ uint32_t zd_dev_word(uint32_t a, uint32_t v, uint32_t b) {
  const uint32_t m = 0x00FF00FFu;
  const uint32_t ve = v & m, vo = (v >> 8) & m;
  const uint32_t me = zd_median(a & m, ve, b & m), mo = zd_median((a >> 8) & m, vo, (b >> 8) & m);
  const zd_u16x2 Ve = __builtin_bit_cast(zd_u16x2, ve), Me = __builtin_bit_cast(zd_u16x2, me);
  const zd_u16x2 Vo = __builtin_bit_cast(zd_u16x2, vo), Mo = __builtin_bit_cast(zd_u16x2, mo);
  const zd_u16x2 ee = __builtin_elementwise_max(Ve, Me) - __builtin_elementwise_min(Ve, Me);
  const zd_u16x2 eo = __builtin_elementwise_max(Vo, Mo) - __builtin_elementwise_min(Vo, Mo);
  return __builtin_bit_cast(uint32_t, ee) | (__builtin_bit_cast(uint32_t, eo) << 8);
}

// The n (1...4) bytes at p as one word, the bytes past n zero: the one or two naturally aligned words that hold them.
__device__ __forceinline__ uint32_t zd_load4(const uint8_t *p, int n) {
  const uint32_t a = (uint32_t)((uintptr_t)p & 3);
  const uint32_t *q = reinterpret_cast<const uint32_t *>(p - a);
  const uint32_t w0 = q[0], w1 = (int)a + n > 4 ? q[1] : 0u;
  const uint32_t w = __builtin_amdgcn_alignbyte(w1, w0, a);
  return n < 4 ? w & ((1u << (8 * n)) - 1u) : w;
}

// The block's planes of row (lo, hi) of the device's table for a plane with a verdict, clamped into the block.
__device__ __forceinline__ int32_t zd_plane(int32_t z, int32_t sz0, int32_t D) { return min(max(z, sz0), sz0 + D - 1) - sz0; }

// Block b = ((run * nty + ti) * ntx + tj) * parts + part, as u8_zcorr_tiles_k.  rpp * S <= ZD_ITEMS.
__global__ __launch_bounds__(ZC_THREADS) void u8_zdev_tiles_k(const uint8_t *src, int32_t D, int64_t H, int64_t W,
                                                              int32_t sz0, int32_t c0, int32_t c1, int64_t y_org,
                                                              int64_t x_org, int64_t th, int64_t tw, int64_t gy,
                                                              int64_t gx, int64_t ti0, int64_t tj0, uint32_t nty,
                                                              uint32_t ntx, uint32_t parts, int64_t rpp, uint32_t S,
                                                              uint32_t magicS, int32_t zr, const int32_t *nbr,
                                                              uint64_t *sums) {
  __shared__ uint32_t red[2][ZC_THREADS / 64];
  uint32_t b = blockIdx.x;
  const uint32_t part = b % parts;
  b /= parts;
  const uint32_t tjl = b % ntx;
  b /= ntx;
  const uint32_t til = b % nty, run = b / nty;
  const int64_t ti = ti0 + til, tj = tj0 + tjl;
  const int64_t ya = max(ti * th - y_org, (int64_t)0) + (int64_t)part * rpp;
  const int64_t yb = min(min((ti + 1) * th - y_org, H), ya + rpp);
  const int64_t xa = max(tj * tw - x_org, (int64_t)0), xb = min((tj + 1) * tw - x_org, W);
  if (ya >= yb || xa >= xb) return;                                      // the whole workgroup: the tail part of a cut tile
  const int32_t width = (int32_t)(xb - xa);
  const uint32_t total = (uint32_t)(yb - ya) * S;                        // <= ZD_ITEMS
  const int32_t z0 = c0 + (int32_t)run * zr, z1 = min(z0 + zr, c1);
  const int64_t plane = H * W;
  const uint8_t *first = src + ya * W + xa;                              // in the block's plane 0

  int64_t off[ZD_K];                                                     // piece k of this thread: its offset in a plane
  int32_t cnt[ZD_K];                                                     // and its bytes, 0: none
#pragma unroll
  for (int k = 0; k < ZD_K; ++k) {
    const uint32_t i = threadIdx.x + ZC_THREADS * k;
    const uint32_t ri = S == 1 ? i : __umulhi(i, magicS), s = i - ri * S;
    const int32_t lo = 16 * (int32_t)s;
    cnt[k] = i < total && lo < width ? min(16, width - lo) : 0;
    off[k] = (int64_t)ri * W + lo;
  }
  uint32_t A[ZD_K][4] = {}, V[ZD_K][4] = {}, B[ZD_K][4] = {};            // the block's planes ha, hv, hb; -1: none yet
  int32_t ha = -1, hv = -1, hb = -1;
  auto load = [&](uint32_t(&w)[ZD_K][4], int32_t p) {
#pragma unroll
    for (int k = 0; k < ZD_K; ++k) {
      w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0;
      if (cnt[k]) zc_load(first + (int64_t)p * plane + off[k], cnt[k], w[k]);
    }
  };
  auto move = [&](uint32_t(&w)[ZD_K][4], const uint32_t(&u)[ZD_K][4]) {
#pragma unroll
    for (int k = 0; k < ZD_K; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[k][j] = u[k][j];
    }
  };
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t nvox = (uint64_t)(yb - ya) * (uint64_t)width;
  int par = 0;
  for (int32_t d = z0; d < z1; ++d) {
    const int32_t *t = nbr + 2 * ((int64_t)sz0 + d);
    const int32_t lo = __builtin_amdgcn_readfirstlane(t[0]), hi = __builtin_amdgcn_readfirstlane(t[1]);
    if (lo < 0 || hi < 0) continue;                                      // no verdict: the same in every thread
    const int32_t na = zd_plane(lo, sz0, D), nb = zd_plane(hi, sz0, D);
    // the labels always say what the registers hold, so any table gives the sums of the planes it names
    if (na != ha) {
      if (na == hv) move(A, V); else if (na == hb) move(A, B); else load(A, na);
      ha = na;
    }
    if (d != hv) {
      if (d == hb) move(V, B); else if (d == ha) move(V, A); else load(V, d);
      hv = d;
    }
    if (nb != hb) {
      if (nb == ha) move(B, A); else if (nb == hv) move(B, V); else load(B, nb);
      hb = nb;
    }
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < ZD_K; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s = zd_dev_sum(A[k][j], V[k][j], B[k][j], s);
    }
    s = zc_wave_sum(s);
    // two copies of the wave sums, taken in turn by the planes that are counted: one barrier per plane (whoever
    // writes a copy again has passed the barrier of the plane in between, behind which no thread still reads it)
    if (lane == 0) red[par][wave] = s;
    __syncthreads();
    if (threadIdx.x < 2) {
      uint64_t v = nvox;
      if (threadIdx.x == 0) {
        v = 0;
#pragma unroll
        for (int wv = 0; wv < ZC_THREADS / 64; ++wv) v += red[par][wv];
      }
      uint64_t *q = sums + ((((int64_t)(d - c0) * gy + ti) * gx + tj) * 2 + threadIdx.x);
      if (v) atomicAdd(reinterpret_cast<unsigned long long *>(q), (unsigned long long)v);
    }
    par ^= 1;
  }
}

struct zdm_args {
  const uint8_t *src;
  int32_t D;
  int64_t H, W;
  int32_t sz0, Y, y_org, c0, r0, r1, x0, x1, th, tw, gy, gx;
  int32_t tiles_x, tiles;                        // tiles of 8 x 32 outputs along x, and per plane
  int32_t run, runs;                             // tiles per workgroup, workgroups per plane
  const int32_t *nbr, *thr;
  const uint8_t *marks;                          // tiles_dev, or null
  uint8_t *dst;
  unsigned long long *count;                     // or null
};

// Block b = plane * runs + q: tiles [q run, min((q + 1) run, tiles)) of core plane c0 + plane, one after the other;
// tile t = ty * tiles_x + tx holds the outputs [r0 + 8 ty, +8) x [x0 + 32 tx, +32).
template <int R>
__global__ __launch_bounds__(ZDM_THREADS) void u8_zdev_mask_k(zdm_args g) {
  constexpr int WIN = 2 * R + 1, RH = ZDM_TY + 2 * R, RW = ZDM_TX + 2 * R, RWW = (RW + 3) / 4, RWP = 4 * RWW;
  __shared__ uint32_t se[RH * RWW];              // e of the patch: rows of RWP bytes
  __shared__ uint16_t rs[RH * ZDM_TX];
  __shared__ uint32_t ones[ZDM_THREADS / 64];

  const int tid = threadIdx.x, tx = tid % ZDM_TX, ty = tid / ZDM_TX;
  const int pl = blockIdx.x / g.runs, first = (blockIdx.x - pl * g.runs) * g.run, d = g.c0 + pl;
  const int32_t *t = g.nbr + 2 * ((int64_t)g.sz0 + d);
  const int32_t lo = __builtin_amdgcn_readfirstlane(t[0]), hi = __builtin_amdgcn_readfirstlane(t[1]);
  const bool verdict = lo >= 0 && hi >= 0;                               // the same in every thread
  const int64_t plane = g.H * g.W;
  const uint8_t *pa = g.src + (int64_t)zd_plane(lo, g.sz0, g.D) * plane, *pv = g.src + (int64_t)d * plane;
  const uint8_t *pb = g.src + (int64_t)zd_plane(hi, g.sz0, g.D) * plane;
  uint32_t mine = 0;                                                     // ones this thread wrote
  for (int tile = first; tile < min(first + g.run, g.tiles); ++tile) {
    const int tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
    const int oy = g.r0 + tyi * ZDM_TY, ox = g.x0 + txi * ZDM_TX;          // the tile's first output, in the block
    uint32_t Ws = 0;
    if (verdict) {
      // 1. stage e of the patch, a word of four columns per step (whoever still adds the previous tile's row sums has
      //    not passed this tile's first barrier, behind which they are written again)
      for (int i = tid; i < RH * RWW; i += ZDM_THREADS) {
        const int rr = i / RWW, k = i - rr * RWW;
        const int y = oy - R + rr, ca = ox - R + 4 * k;                    // the word: columns [ca, ca + 4) of row y
        const int xl = max(ca, 0), xh = (int)min((int64_t)ca + 4, g.W);
        uint32_t e = 0;
        if (y >= 0 && y < g.H && xl < xh) {
          const int64_t at = (int64_t)y * g.W + xl;
          const int n = xh - xl;
          e = zd_dev_word(zd_load4(pa + at, n), zd_load4(pv + at, n), zd_load4(pb + at, n)) << (8 * (xl - ca));
        }
        se[i] = e;
      }
      __syncthreads();
      // 2. row sums along x
      const uint8_t *sb = reinterpret_cast<const uint8_t *>(se);
      for (int i = tid; i < RH * ZDM_TX; i += ZDM_THREADS) {
        const int rr = i / ZDM_TX, cc = i - rr * ZDM_TX;
        const uint8_t *p = sb + rr * RWP + cc;
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < WIN; ++j) s += p[j];
        rs[i] = (uint16_t)s;
      }
      __syncthreads();
      // 3. column sums along y
#pragma unroll
      for (int j = 0; j < WIN; ++j) Ws += rs[(ty + j) * ZDM_TX + tx];
    }
    const int y = oy + ty, x = ox + tx;
    uint32_t one = 0;
    if (y < g.r1 && x < g.x1) {
      const int yv = g.y_org + y;                                          // the volume's row; x is the volume's column
      const int cy = min(yv + R, g.Y - 1) - max(yv - R, 0) + 1;
      const int cx = (int)min((int64_t)x + R, g.W - 1) - max(x - R, 0) + 1;
      const int64_t cell = (int64_t)(yv / g.th) * g.gx + x / g.tw;
      const uint32_t thr = (uint32_t)min(max(g.thr[cell], 1), ZD_MAX_THR);
      one = 256u * Ws > thr * (uint32_t)(cy * cx);
      if (g.marks && g.marks[(int64_t)pl * g.gy * g.gx + cell]) one = 1;
      g.dst[((int64_t)pl * (g.r1 - g.r0) + (y - g.r0)) * (g.x1 - g.x0) + (x - g.x0)] = (uint8_t)one;
    }
    mine += one;
  }
  if (g.count) {                                                         // the same in every thread
    mine = zc_wave_sum(mine);                                            // at most ZDM_MAX_RUN per thread
    if ((tid & 63) == 0) ones[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
      unsigned long long n = 0;
#pragma unroll
      for (int wv = 0; wv < ZDM_THREADS / 64; ++wv) n += ones[wv];
      if (n) atomicAdd(g.count, n);
    }
  }
}

// The rows of the host's table for the block's core planes [c0, c1): each (-1, -1), or lo < z < hi inside the stack,
// at most ZD_MAX_LAG away, and inside the block.
bool zd_rows_ok(const int32_t *nbr, int32_t sz0, int32_t Z, int32_t D, int32_t c0, int32_t c1) {
  for (int64_t z = (int64_t)sz0 + c0; z < (int64_t)sz0 + c1; ++z) {
    const int64_t lo = nbr[2 * z], hi = nbr[2 * z + 1];
    if (lo == -1 && hi == -1) continue;
    if (lo < 0 || hi >= Z || lo >= z || hi <= z || z - lo > ZD_MAX_LAG || hi - z > ZD_MAX_LAG) return false;
    if (lo < sz0 || hi >= (int64_t)sz0 + D) return false;
  }
  return true;
}

}  // namespace

extern "C" int tem_u8_zdev_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t Z,
                                 int32_t c0, int32_t c1, int32_t y_org, int32_t x_org, int32_t th, int32_t tw,
                                 int32_t gy, int32_t gx, const int32_t *nbr_host, const int32_t *nbr_dev,
                                 uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !sums || !nbr_host || !nbr_dev || ((uintptr_t)sums & 7) || ((uintptr_t)nbr_dev & 3) || D < 1 || H < 1 ||
      W < 1 || th < 1 || th > ZC_MAX_TILE || tw < 1 || tw > ZC_MAX_TILE || gy < 1 || gx < 1 || y_org < 0 || x_org < 0 ||
      (int64_t)y_org + H > (int64_t)gy * th || (int64_t)x_org + W > (int64_t)gx * tw || c0 < 0 || c0 > c1 || c1 > D ||
      Z < 1 || sz0 < 0 || (int64_t)sz0 + D > Z)
    return TEM_EINVAL;
  if (!zd_rows_ok(nbr_host, sz0, Z, D, c0, c1)) return TEM_EINVAL;
  if (c0 == c1) return TEM_OK;
  const int64_t ti0 = y_org / th, tj0 = x_org / tw;
  const int64_t nty = ((int64_t)y_org + H - 1) / th - ti0 + 1, ntx = ((int64_t)x_org + W - 1) / tw - tj0 + 1;
  const int64_t rows = th < H ? th : H, width = tw < W ? tw : W;        // of a tile's part in the block, at most
  const int64_t S = (width + 15) / 16;                                   // <= 128
  const int64_t rpp = ZD_ITEMS / S;                                      // >= 8
  const int64_t parts = (rows + rpp - 1) / rpp;
  const int64_t units = nty * ntx * parts, ncore = c1 - c0;              // < 2^31 * 2^31 * 2^8
  if (units >= ZD_MAX_WGS) return TEM_EUNSUPPORTED;
  // the run: as long as leaves about ZC_WANT_GRID workgroups, ZD_MAX_RUN planes at most
  int64_t zr = ncore * units / ZC_WANT_GRID;
  zr = zr < 1 ? 1 : (zr > ZD_MAX_RUN ? ZD_MAX_RUN : zr);
  const int64_t nruns = (ncore + zr - 1) / zr;
  if (units * nruns >= ZD_MAX_WGS) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_zdev_tiles_k, dim3((unsigned)(units * nruns)), dim3(ZC_THREADS), 0, (hipStream_t)stream, src, D,
                     (int64_t)H, (int64_t)W, sz0, c0, c1, (int64_t)y_org, (int64_t)x_org, (int64_t)th, (int64_t)tw,
                     (int64_t)gy, (int64_t)gx, ti0, tj0, (uint32_t)nty, (uint32_t)ntx, (uint32_t)parts, rpp,
                     (uint32_t)S, magic_for((int)S), (int32_t)zr, nbr_dev, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_zdev_mask(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t Z, int32_t Y,
                                int32_t y_org, int32_t c0, int32_t c1, int32_t r0, int32_t r1, int32_t x0, int32_t x1,
                                int32_t th, int32_t tw, int32_t gy, int32_t gx, int32_t radius, const int32_t *nbr_host,
                                const int32_t *nbr_dev, const int32_t *thr_host, const int32_t *thr_dev,
                                const uint8_t *tiles_dev, uint8_t *dst, uint64_t *count, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || !nbr_host || !nbr_dev || !thr_host || !thr_dev || ((uintptr_t)nbr_dev & 3) ||
      ((uintptr_t)thr_dev & 3) || ((uintptr_t)count & 7) || D < 1 || H < 1 || W < 1 || Y < 1 || Z < 1 || th < 1 ||
      th > ZC_MAX_TILE || tw < 1 || tw > ZC_MAX_TILE || gy < 1 || gx < 1 || radius < 1 || radius > ZD_MAX_RADIUS ||
      y_org < 0 || (int64_t)y_org + H > Y || Y > (int64_t)gy * th || W > (int64_t)gx * tw || sz0 < 0 ||
      (int64_t)sz0 + D > Z || c0 < 0 || c0 > c1 || c1 > D || r0 < 0 || r0 > r1 || r1 > H || x0 < 0 || x0 > x1 || x1 > W)
    return TEM_EINVAL;
  for (int64_t k = 0; k < (int64_t)gy * gx; ++k)
    if (thr_host[k] < 1 || thr_host[k] > ZD_MAX_THR) return TEM_EINVAL;
  if (!zd_rows_ok(nbr_host, sz0, Z, D, c0, c1)) return TEM_EINVAL;
  if (c0 == c1 || r0 == r1 || x0 == x1) return TEM_OK;
  // every row under a core window that the section has: [r0 - radius, r1 + radius) cut to [-y_org, Y - y_org)
  const int64_t need0 = (int64_t)r0 - radius > -(int64_t)y_org ? (int64_t)r0 - radius : -(int64_t)y_org;
  const int64_t need1 = (int64_t)r1 + radius < (int64_t)Y - y_org ? (int64_t)r1 + radius : (int64_t)Y - y_org;
  if (need0 < 0 || need1 > H) return TEM_EINVAL;
  zdm_args g;
  g.src = src, g.D = D, g.H = H, g.W = W;
  g.sz0 = sz0, g.Y = Y, g.y_org = y_org, g.c0 = c0, g.r0 = r0, g.r1 = r1, g.x0 = x0, g.x1 = x1;
  g.th = th, g.tw = tw, g.gy = gy, g.gx = gx;
  const int64_t tiles_x = ((int64_t)x1 - x0 + ZDM_TX - 1) / ZDM_TX, tiles_y = ((int64_t)r1 - r0 + ZDM_TY - 1) / ZDM_TY;
  const int64_t tiles = tiles_x * tiles_y, ncore = c1 - c0;              // tiles < 2^27 * 2^29
  if (tiles > 0x7fffffff) return TEM_EUNSUPPORTED;
  // the run: as long as leaves about ZDM_WANT_GRID workgroups, ZDM_MAX_RUN tiles at most -- `count` then takes one
  // add per run, not per tile: adds to one address go one after the other
  int64_t run = tiles * ncore / ZDM_WANT_GRID;
  run = run < 1 ? 1 : (run > ZDM_MAX_RUN ? ZDM_MAX_RUN : run);
  const int64_t runs = (tiles + run - 1) / run, wgs = runs * ncore;
  if (runs >= ZD_MAX_WGS || wgs >= ZD_MAX_WGS) return TEM_EUNSUPPORTED;
  g.tiles_x = (int32_t)tiles_x, g.tiles = (int32_t)tiles, g.run = (int32_t)run, g.runs = (int32_t)runs;
  g.nbr = nbr_dev, g.thr = thr_dev, g.marks = tiles_dev, g.dst = dst;
  g.count = reinterpret_cast<unsigned long long *>(count);
  const dim3 grid((unsigned)wgs), wg(ZDM_THREADS);
  hipStream_t s = (hipStream_t)stream;
  switch (radius) {
    case 1: hipLaunchKernelGGL(u8_zdev_mask_k<1>, grid, wg, 0, s, g); break;
    case 2: hipLaunchKernelGGL(u8_zdev_mask_k<2>, grid, wg, 0, s, g); break;
    case 3: hipLaunchKernelGGL(u8_zdev_mask_k<3>, grid, wg, 0, s, g); break;
    case 4: hipLaunchKernelGGL(u8_zdev_mask_k<4>, grid, wg, 0, s, g); break;
    case 5: hipLaunchKernelGGL(u8_zdev_mask_k<5>, grid, wg, 0, s, g); break;
    case 6: hipLaunchKernelGGL(u8_zdev_mask_k<6>, grid, wg, 0, s, g); break;
    default: hipLaunchKernelGGL(u8_zdev_mask_k<7>, grid, wg, 0, s, g); break;
  }
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
