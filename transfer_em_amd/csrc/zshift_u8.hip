// zshift_u8.hip -- the sums behind the correlation of every tile of a uint8 section with the next section displaced by
// every integer offset within a radius (utils.section_shift_sums -> shift_scores -> section_shifts):
//   tem_u8_zshift_tiles   sums[d - c0][i][j][dy + r][dx + r][0..4] += sum v, sum v v, sum w, sum w w, sum v w over the
//                         core voxels v = (d, y, x) of tile (i, j) whose partner w = (d + 1, y + dy, x + dx) lies in the
//                         section (no sums at all for the block's last plane)
//   tem_u8_zshift_tiles_at  the same with the offsets of every plane and tile centred on (cy, cx) of a device table:
//                         the partner is w = (d + 1, y + cy + dy, x + cx + dx) (utils.section_shift_sums_at, the
//                         device leg of section_shifts_coarse_to_fine); see zs_tiles_at
//   tem_u8_zshift_tiles_pairs  the centred sums of an explicit device list of section pairs (a, b), a < b, with a row
//                         of centres and of sums per pair: v = (a, y, x), w = (b, y + cy + dy, x + cx + dx)
//                         (utils.section_shift_sums_pairs, the device leg of section_shifts_bridged: bad sections are
//                         skipped and their good neighbours measured against each other); the same body, zs_tiles_at
// The tile grid is tem_u8_hist_tiles': anchored at (0, 0) of the caller's VOLUME; the block holds whole rows, its row 0
// at volume row y_org.  Everything is integers and the adds are atomic, so the sums do not depend on how the volume
// was cut into blocks or the block into workgroups.
//
// The offsets sit on the LANES.  A workgroup of 256 threads owns one core plane d and a PART of one tile: up to
// ZS_MAX_ROWS rows of up to ZS_MAX_COLS columns, ZS_MAX_WORDS 4-byte words (4096 voxels) at most.  It stages two
// images in LDS as bytes: the part of plane d (`v`, its rows padded with zeros to whole words) and the WINDOW of plane
// d + 1 (`w`): the part grown by r on every side, zero wherever the section -- not the tile -- ends, so a partner that
// does not exist adds nothing to sum w, sum w w and sum v w.  The window's row stride is padded to 5, 13, 19 or 27 words
// modulo 32: the lanes of one 32-lane half read a handful of consecutive window rows at up to five consecutive words,
// and these strides keep those on different banks.
//
// A lane owns one offset o = 64 pass + lane = (dy + r) R + (dx + r); a wave owns a quarter of the part's rows and walks
// them once per pass (1 pass up to r = 3, 2 at r = 4, 5 at r = 8).  Per step the lane reads ONE new word of its window
// row and funnel-shifts it against the previous one by (dx + r) & 3 (v_alignbyte_b32), which gives the four partners
// of one word of v; the word of v is the same for all lanes, a broadcast read.  sum w, sum w w and sum v w are three
// packed byte dot products (v_dot4_u32_u8) against 0x01010101, itself and v.  sum v and sum v v differ between offsets
// only where a partner can miss, and there the miss is whole rows (by dy) times whole columns (by dx): a wave first
// sums every row of its quarter once, one row per lane (the rows of v have an odd stride, so the lanes sit on
// different banks).  In a part within r of a face of the section a lane then adds up the rows whose partner row
// exists, each less the at most r voxels at the row's end whose partner column does not; in every other part the
// row sums are added once per wave, not per offset.  The walk itself is the same three dot products everywhere.  The
// lane's sums stay in registers for its rows, the four waves' meet in LDS (32-bit adds), and they leave as one 64-bit
// global atomic add per workgroup, offset and quantity.
//
// Loads.  A staged word starts at any address: it is put together from the one or two naturally aligned words that
// hold its bytes (v_alignbyte_b32), and a word is loaded only if it holds a byte that is wanted -- a byte of the
// block --; the bytes past a row's ends are masked to zero.
//
// No partial can overflow.  A part holds at most 4096 voxels, each term at most 255 x 255 = 65025: a lane's sums, a
// wave's and the LDS sums over the whole part all stay below 4096 x 65025 < 2^28 in 32 bits.  They are widened to 64
// bits for the global add; a whole 2048 x 2048 tile of 255s is 2^22 x 65025 < 2^38 per plane, offset and quantity.
#include "tem_common.h"

namespace {

constexpr int ZS_THREADS = 256;
constexpr int ZS_WAVES = ZS_THREADS / 64;
constexpr int ZS_MAX_TILE = 2048;
constexpr int ZS_MAX_R = 8;
constexpr int ZS_MAX_CENTER = 1024;              // tem_u8_zshift_tiles_at: |cy|, |cx| of a window's centre, at most
constexpr int ZS_MAX_COLS = 128;                 // columns of a part, at most
constexpr int ZS_MAX_ROWS = 64;                  // rows of a part, at most
constexpr int ZS_MAX_WORDS = 1024;               // words of a part, at most: rows x ceil(columns / 4)
constexpr int ZS_MAX_OFFS = (2 * ZS_MAX_R + 1) * (2 * ZS_MAX_R + 1);
// the window: (rows + 2 r) x stride, stride <= words + 2 r / 4 + 1 + 9 of padding:
// rows words + 14 rows + 16 words + 224 <= 1024 + 14 x 64 + 16 x 32 + 224
constexpr int ZS_WIN_WORDS = 2656;

// 0xff in the bytes b of a word with lo <= b < hi, for any lo, hi
__device__ __forceinline__ uint32_t zs_bytes(int lo, int hi) {
  lo = max(lo, 0), hi = min(hi, 4);
  if (lo >= hi) return 0u;
  const uint32_t up = hi >= 4 ? 0xffffffffu : (1u << (8 * hi)) - 1u;
  return up & (0xffffffffu << (8 * lo));
}

// rows x nw words of plane `d` of the block into dst (row stride `stride` words): the word (i, j) holds the bytes at
// block row row0 + i, columns col0 + 4 j ... + 3, zero outside rows [rl, rh) and columns [cl, ch) -- both inside the
// block.
__device__ __forceinline__ void zs_stage(uint32_t *dst, int rows, int nw, int stride, const uint8_t *src, int64_t d,
                                         int64_t H, int64_t W, int64_t row0, int64_t col0, int64_t rl, int64_t rh,
                                         int64_t cl, int64_t ch) {
  const uint32_t total = (uint32_t)(rows * nw);
  for (uint32_t idx = threadIdx.x; idx < total; idx += ZS_THREADS) {
    const uint32_t i = idx / (uint32_t)nw, j = idx - i * (uint32_t)nw;
    const int64_t row = row0 + i, col = col0 + 4 * (int64_t)j;
    uint32_t val = 0;
    if (row >= rl && row < rh) {
      const int lo = (int)max(cl - col, (int64_t)0), hi = (int)min(ch - col, (int64_t)4);
      if (lo < hi) {
        const uintptr_t p = (uintptr_t)src + (uintptr_t)((d * H + row) * W + col);
        const uint32_t a = (uint32_t)(p & 3);
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - a);           // q[0]: bytes -a ... 3 - a of the word
        const uint32_t w0 = lo < 4 - (int)a ? q[0] : 0u;
        const uint32_t w1 = hi > 4 - (int)a ? q[1] : 0u;
        val = __builtin_amdgcn_alignbyte(w1, w0, a) & zs_bytes(lo, hi);
      }
    }
    dst[i * (uint32_t)stride + j] = val;
  }
}

__device__ __forceinline__ uint32_t zs_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block b = (((plane * nty + ti) * ntx + tj) * nrc + rc) * ncc + cc: core plane c0 + plane, rows
// [rc * prows, (rc + 1) * prows) and columns [cc * ZS_MAX_COLS, (cc + 1) * ZS_MAX_COLS) of the part of tile
// (ti0 + ti, tj) that lies in the core rows [r0, r1).  prows * ceil(min(tile part's width, ZS_MAX_COLS) / 4) <= ZS_MAX_WORDS.
__global__ __launch_bounds__(ZS_THREADS) void u8_zshift_tiles_k(const uint8_t *src, int64_t H, int64_t W, int32_t c0,
                                                                int64_t r0, int64_t r1, int64_t y_org, int64_t Y,
                                                                int64_t th, int64_t tw, int64_t gy, int64_t gx,
                                                                int64_t ti0, uint32_t nty, uint32_t ntx, uint32_t nrc,
                                                                uint32_t ncc, int32_t prows, int32_t r,
                                                                uint64_t *sums) {
  __shared__ uint32_t vl[ZS_MAX_WORDS + ZS_MAX_ROWS];
  __shared__ uint32_t wl[ZS_WIN_WORDS];
  __shared__ uint32_t acc[ZS_MAX_OFFS * 5];
  __shared__ uint32_t once[2];                                           // sum v, sum v v of an interior part
  uint32_t b = blockIdx.x;
  const uint32_t cc = b % ncc;
  b /= ncc;
  const uint32_t rc = b % nrc;
  b /= nrc;
  const uint32_t tj = b % ntx;
  b /= ntx;
  const uint32_t til = b % nty, plane = b / nty;
  const int64_t ti = ti0 + til;
  const int64_t ya = max(ti * th - y_org, r0) + (int64_t)rc * prows;
  const int64_t yb = min(min((ti + 1) * th - y_org, r1), ya + prows);
  const int64_t xa = (int64_t)tj * tw + (int64_t)cc * ZS_MAX_COLS;
  const int64_t xb = min(min((int64_t)(tj + 1) * tw, W), xa + ZS_MAX_COLS);
  if (ya >= yb || xa >= xb) return;                                      // the whole workgroup: the tail part of a cut tile
  const int rows = (int)(yb - ya), width = (int)(xb - xa);
  const int R = 2 * r + 1, noffs = R * R;
  const int pw = (width + 3) >> 2, pv = pw | 1;                          // words per row of v, and its odd row stride
  const int nw = pw + (2 * r >> 2) + 1;                                  // words per row of the window that are read
  int stride = nw;                                                       // 5, 13, 19 or 27 modulo 32
  while ((stride & 31) != 5 && (stride & 31) != 13 && (stride & 31) != 19 && (stride & 31) != 27) ++stride;
  const int64_t d = (int64_t)c0 + plane;
  // a part whose every voxel has every partner: no face of the section within r
  const bool inner = y_org + ya - r >= 0 && y_org + yb + r <= Y && xa - r >= 0 && xb + r <= W;

  for (uint32_t i = threadIdx.x; i < (uint32_t)noffs * 5; i += ZS_THREADS) acc[i] = 0;
  if (threadIdx.x < 2) once[threadIdx.x] = 0;
  zs_stage(vl, rows, pw, pv, src, d, H, W, ya, xa, ya, yb, xa, xb);
  zs_stage(wl, rows + 2 * r, nw, stride, src, d + 1, H, W, ya - r, xa - r, max((int64_t)0, -y_org), min(H, Y - y_org),
           0, W);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ra = rows * wave / ZS_WAVES, rb = rows * (wave + 1) / ZS_WAVES;      // this wave's rows of the part: <= 16
  const uint32_t tail = zs_bytes(0, width - 4 * (pw - 1));               // the bytes of a row's last word that are voxels
  if (ra < rb) {
    // sum v and sum v v of row ra + lane, in lane `lane` (the odd row stride pv keeps the lanes on different banks)
    uint32_t row1 = 0, row2 = 0;
    if (lane < rb - ra) {
      const uint32_t *vrow = vl + (ra + lane) * pv;
      for (int k = 0; k < pw; ++k) {
        const uint32_t v = vrow[k];
        row1 = __builtin_amdgcn_udot4(v, 0x01010101u, row1, false);
        row2 = __builtin_amdgcn_udot4(v, v, row2, false);
      }
    }
    if (inner) {                                                         // every offset has every partner: once per wave
      const uint32_t s1 = zs_wave_sum(row1), s2 = zs_wave_sum(row2);
      if (lane == 0) atomicAdd(&once[0], s1), atomicAdd(&once[1], s2);
    }
    for (int o0 = 0; o0 < noffs; o0 += 64) {
      const int o = min(o0 + lane, noffs - 1);
      const int dyi = o / R, dxi = o - dyi * R;                          // dy + r, dx + r
      uint32_t sv = 0, svv = 0, sw = 0, sww = 0, svw = 0;
      if (!inner) {
        // sum v, sum v v over the voxels with a partner: the rows whose partner row is in the section, of each the
        // row's sums less those of the columns [e0, e1) of the part whose partner column is not -- at most r of them,
        // at the row's left end for dx < 0 or at its right end for dx > 0
        const int64_t dx = dxi - r;
        const int e0 = dx > 0 ? (int)max((int64_t)0, min((int64_t)width, W - dx - xa)) : 0;
        const int e1 = dx > 0 ? width : (int)max((int64_t)0, min((int64_t)width, -dx - xa));
        const int k0 = e0 >> 2, k1 = e0 < e1 ? (e1 + 3) >> 2 : k0;
        for (int y = ra; y < rb; ++y) {
          const uint32_t a1 = (uint32_t)__shfl((int)row1, y - ra, 64), a2 = (uint32_t)__shfl((int)row2, y - ra, 64);
          const int64_t py = y_org + ya + y + dyi - r;                   // the partner's row in the volume
          uint32_t m1 = 0, m2 = 0;
          for (int k = k0; k < k1; ++k) {
            const uint32_t v = vl[y * pv + k] & zs_bytes(e0 - 4 * k, e1 - 4 * k);
            m1 = __builtin_amdgcn_udot4(v, 0x01010101u, m1, false);
            m2 = __builtin_amdgcn_udot4(v, v, m2, false);
          }
          if (py >= 0 && py < Y) sv += a1 - m1, svv += a2 - m2;
        }
      }
      const uint32_t sh = (uint32_t)dxi & 3u;
      const uint32_t *wrow = wl + (ra + dyi) * stride + (dxi >> 2);
      const uint32_t *vrow = vl + ra * pv;
      for (int y = ra; y < rb; ++y, wrow += stride, vrow += pv) {
        uint32_t prev = wrow[0];
#pragma unroll 4
        for (int k = 0; k < pw - 1; ++k) {
          const uint32_t nxt = wrow[k + 1];
          const uint32_t w = __builtin_amdgcn_alignbyte(nxt, prev, sh), v = vrow[k];
          prev = nxt;
          sw = __builtin_amdgcn_udot4(w, 0x01010101u, sw, false);
          sww = __builtin_amdgcn_udot4(w, w, sww, false);
          svw = __builtin_amdgcn_udot4(v, w, svw, false);
        }
        const uint32_t w = __builtin_amdgcn_alignbyte(wrow[pw], prev, sh) & tail, v = vrow[pw - 1];
        sw = __builtin_amdgcn_udot4(w, 0x01010101u, sw, false);
        sww = __builtin_amdgcn_udot4(w, w, sww, false);
        svw = __builtin_amdgcn_udot4(v, w, svw, false);
      }
      if (o0 + lane < noffs) {
        uint32_t *a = acc + 5 * o;
        if (sv) atomicAdd(a + 0, sv);
        if (svv) atomicAdd(a + 1, svv);
        if (sw) atomicAdd(a + 2, sw);
        if (sww) atomicAdd(a + 3, sww);
        if (svw) atomicAdd(a + 4, svw);
      }
    }
  }
  __syncthreads();
  uint64_t *out = sums + ((((int64_t)plane * gy + ti) * gx + tj) * noffs) * 5;
  for (uint32_t i = threadIdx.x; i < (uint32_t)noffs * 5; i += ZS_THREADS) {
    const uint32_t q = i % 5;
    const uint32_t v = inner && q < 2 ? once[q] : acc[i];
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(out + i), (unsigned long long)v);
  }
}

// u8_zshift_tiles_k with the search window of every plane and tile CENTRED on (cy, cx) of `centers`
// ([plane][gy][gx][2], the rows of core plane c0): the offset of lane o is (cy + dy, cx + dx).  Blocks, parts, LDS
// images and the walk are the sibling's; what differs:
//   - the workgroup reads its tile's centre once, uniformly, and clamps it to the host's promise: cy to
//     [cy_lo, cy_hi], cx to [-cx_max, cx_max] (all within 1024, so every sum of offsets below stays far inside 32 bits);
//   - the window of plane d + 1 is staged from (ya - r + cy, xa - r + cx): zs_stage zeroes what lies outside the
//     section's rows in the block and outside [0, W), and loads no word without a byte of the block, wherever the
//     origin lies;
//   - a part whose whole window lies outside the section has no voxel with a partner at any offset: the workgroup
//     leaves before it stages, loads or adds anything;
//   - `inner` and the edge sums of sum v, sum v v use the total offset.  The missing columns [e0, e1) of a row are
//     still one run at the row's left end (dx_total < 0) or right end (dx_total > 0), but the run is now up to the
//     WHOLE width of the part -- |dx_total| reaches 1032, a part has 128 columns at most --, so its words k0 ... k1
//     run over up to all pw words of the row, not over the one to three that r <= 8 columns took.
// The body is written once for two kernels.  `plane`, the slowest part of the block index, is the row of `centers`
// and of `sums`; what it says about the two planes of the block differs:
//   PAIRS false (u8_zshift_tiles_at_k)     v is plane c0 + plane, w the plane above it
//   PAIRS true  (u8_zshift_tiles_pairs_k)  `plane` is the index k of a pair (a, b) of VOLUME sections in the device
//     table `pairs` ([npairs][2]); the block's plane 0 is section c0 (z_org), so v is plane a - c0 and w plane b - c0.
//     The workgroup reads the two numbers once, uniformly, and clamps both planes to [0, D - 1]: a table that names a
//     section outside the block gives the sums of the clamped planes, never a read outside the block.
template <bool PAIRS>
__device__ __forceinline__ void zs_tiles_at(const uint8_t *src, int64_t H, int64_t W, int32_t c0, const int32_t *pairs,
                                            int32_t D, int64_t r0, int64_t r1, int64_t y_org, int64_t Y, int64_t th,
                                            int64_t tw, int64_t gy, int64_t gx, int64_t ti0, uint32_t nty, uint32_t ntx,
                                            uint32_t nrc, uint32_t ncc, int32_t prows, int32_t r,
                                            const int32_t *centers, int32_t cy_lo, int32_t cy_hi, int32_t cx_max,
                                            uint64_t *sums) {
  __shared__ uint32_t vl[ZS_MAX_WORDS + ZS_MAX_ROWS];
  __shared__ uint32_t wl[ZS_WIN_WORDS];
  __shared__ uint32_t acc[ZS_MAX_OFFS * 5];
  __shared__ uint32_t once[2];                                           // sum v, sum v v of an interior part
  uint32_t b = blockIdx.x;
  const uint32_t cc = b % ncc;
  b /= ncc;
  const uint32_t rc = b % nrc;
  b /= nrc;
  const uint32_t tj = b % ntx;
  b /= ntx;
  const uint32_t til = b % nty, plane = b / nty;
  const int64_t ti = ti0 + til;
  const int64_t ya = max(ti * th - y_org, r0) + (int64_t)rc * prows;
  const int64_t yb = min(min((ti + 1) * th - y_org, r1), ya + prows);
  const int64_t xa = (int64_t)tj * tw + (int64_t)cc * ZS_MAX_COLS;
  const int64_t xb = min(min((int64_t)(tj + 1) * tw, W), xa + ZS_MAX_COLS);
  if (ya >= yb || xa >= xb) return;                                      // the whole workgroup: the tail part of a cut tile
  const int32_t *ctr = centers + (((int64_t)plane * gy + ti) * gx + tj) * 2;       // the same for the whole workgroup
  const int cy = min(max(__builtin_amdgcn_readfirstlane(ctr[0]), cy_lo), cy_hi);
  const int cx = min(max(__builtin_amdgcn_readfirstlane(ctr[1]), -cx_max), cx_max);
  // the window's rows and columns in the volume: [wy0, wy1) x [wx0, wx1); nothing of it in the section: no partner
  // exists at any offset, so there is nothing to add and nothing to load
  const int64_t wy0 = y_org + ya - r + cy, wy1 = y_org + yb + r + cy, wx0 = xa - r + cx, wx1 = xb + r + cx;
  if (wy0 >= Y || wy1 <= 0 || wx0 >= W || wx1 <= 0) return;             // the whole workgroup
  const int rows = (int)(yb - ya), width = (int)(xb - xa);
  const int R = 2 * r + 1, noffs = R * R;
  const int pw = (width + 3) >> 2, pv = pw | 1;                          // words per row of v, and its odd row stride
  const int nw = pw + (2 * r >> 2) + 1;                                  // words per row of the window that are read
  int stride = nw;                                                       // 5, 13, 19 or 27 modulo 32
  while ((stride & 31) != 5 && (stride & 31) != 13 && (stride & 31) != 19 && (stride & 31) != 27) ++stride;
  int64_t d = (int64_t)c0 + plane, dw = d + 1;                           // the planes of v and of w in the block
  if constexpr (PAIRS) {
    const int32_t *ab = pairs + 2 * (int64_t)plane;                      // the same for the whole workgroup
    d = min(max((int64_t)__builtin_amdgcn_readfirstlane(ab[0]) - c0, (int64_t)0), (int64_t)D - 1);
    dw = min(max((int64_t)__builtin_amdgcn_readfirstlane(ab[1]) - c0, (int64_t)0), (int64_t)D - 1);
  }
  // a part whose every voxel has every partner: the whole window lies in the section
  const bool inner = wy0 >= 0 && wy1 <= Y && wx0 >= 0 && wx1 <= W;

  for (uint32_t i = threadIdx.x; i < (uint32_t)noffs * 5; i += ZS_THREADS) acc[i] = 0;
  if (threadIdx.x < 2) once[threadIdx.x] = 0;
  zs_stage(vl, rows, pw, pv, src, d, H, W, ya, xa, ya, yb, xa, xb);
  zs_stage(wl, rows + 2 * r, nw, stride, src, dw, H, W, ya - r + cy, xa - r + cx, max((int64_t)0, -y_org),
           min(H, Y - y_org), 0, W);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ra = rows * wave / ZS_WAVES, rb = rows * (wave + 1) / ZS_WAVES;      // this wave's rows of the part: <= 16
  const uint32_t tail = zs_bytes(0, width - 4 * (pw - 1));               // the bytes of a row's last word that are voxels
  if (ra < rb) {
    // sum v and sum v v of row ra + lane, in lane `lane` (the odd row stride pv keeps the lanes on different banks)
    uint32_t row1 = 0, row2 = 0;
    if (lane < rb - ra) {
      const uint32_t *vrow = vl + (ra + lane) * pv;
      for (int k = 0; k < pw; ++k) {
        const uint32_t v = vrow[k];
        row1 = __builtin_amdgcn_udot4(v, 0x01010101u, row1, false);
        row2 = __builtin_amdgcn_udot4(v, v, row2, false);
      }
    }
    if (inner) {                                                         // every offset has every partner: once per wave
      const uint32_t s1 = zs_wave_sum(row1), s2 = zs_wave_sum(row2);
      if (lane == 0) atomicAdd(&once[0], s1), atomicAdd(&once[1], s2);
    }
    for (int o0 = 0; o0 < noffs; o0 += 64) {
      const int o = min(o0 + lane, noffs - 1);
      const int dyi = o / R, dxi = o - dyi * R;                          // dy + r, dx + r
      uint32_t sv = 0, svv = 0, sw = 0, sww = 0, svw = 0;
      if (!inner) {
        // sum v, sum v v over the voxels with a partner: the rows whose partner row is in the section, of each the
        // row's sums less those of the columns [e0, e1) of the part whose partner column is not: one run at the row's
        // left end for dx < 0 or at its right end for dx > 0, of up to the whole width (k0 ... k1: up to pw words)
        const int64_t dx = cx + dxi - r;
        const int e0 = dx > 0 ? (int)max((int64_t)0, min((int64_t)width, W - dx - xa)) : 0;
        const int e1 = dx > 0 ? width : (int)max((int64_t)0, min((int64_t)width, -dx - xa));
        const int k0 = e0 >> 2, k1 = e0 < e1 ? (e1 + 3) >> 2 : k0;
        for (int y = ra; y < rb; ++y) {
          const uint32_t a1 = (uint32_t)__shfl((int)row1, y - ra, 64), a2 = (uint32_t)__shfl((int)row2, y - ra, 64);
          const int64_t py = y_org + ya + y + cy + dyi - r;              // the partner's row in the volume
          uint32_t m1 = 0, m2 = 0;
          for (int k = k0; k < k1; ++k) {
            const uint32_t v = vl[y * pv + k] & zs_bytes(e0 - 4 * k, e1 - 4 * k);
            m1 = __builtin_amdgcn_udot4(v, 0x01010101u, m1, false);
            m2 = __builtin_amdgcn_udot4(v, v, m2, false);
          }
          if (py >= 0 && py < Y) sv += a1 - m1, svv += a2 - m2;
        }
      }
      const uint32_t sh = (uint32_t)dxi & 3u;
      const uint32_t *wrow = wl + (ra + dyi) * stride + (dxi >> 2);
      const uint32_t *vrow = vl + ra * pv;
      for (int y = ra; y < rb; ++y, wrow += stride, vrow += pv) {
        uint32_t prev = wrow[0];
#pragma unroll 4
        for (int k = 0; k < pw - 1; ++k) {
          const uint32_t nxt = wrow[k + 1];
          const uint32_t w = __builtin_amdgcn_alignbyte(nxt, prev, sh), v = vrow[k];
          prev = nxt;
          sw = __builtin_amdgcn_udot4(w, 0x01010101u, sw, false);
          sww = __builtin_amdgcn_udot4(w, w, sww, false);
          svw = __builtin_amdgcn_udot4(v, w, svw, false);
        }
        const uint32_t w = __builtin_amdgcn_alignbyte(wrow[pw], prev, sh) & tail, v = vrow[pw - 1];
        sw = __builtin_amdgcn_udot4(w, 0x01010101u, sw, false);
        sww = __builtin_amdgcn_udot4(w, w, sww, false);
        svw = __builtin_amdgcn_udot4(v, w, svw, false);
      }
      if (o0 + lane < noffs) {
        uint32_t *a = acc + 5 * o;
        if (sv) atomicAdd(a + 0, sv);
        if (svv) atomicAdd(a + 1, svv);
        if (sw) atomicAdd(a + 2, sw);
        if (sww) atomicAdd(a + 3, sww);
        if (svw) atomicAdd(a + 4, svw);
      }
    }
  }
  __syncthreads();
  uint64_t *out = sums + ((((int64_t)plane * gy + ti) * gx + tj) * noffs) * 5;
  for (uint32_t i = threadIdx.x; i < (uint32_t)noffs * 5; i += ZS_THREADS) {
    const uint32_t q = i % 5;
    const uint32_t v = inner && q < 2 ? once[q] : acc[i];
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(out + i), (unsigned long long)v);
  }
}

__global__ __launch_bounds__(ZS_THREADS) void u8_zshift_tiles_at_k(const uint8_t *src, int64_t H, int64_t W, int32_t c0,
                                                                   int64_t r0, int64_t r1, int64_t y_org, int64_t Y,
                                                                   int64_t th, int64_t tw, int64_t gy, int64_t gx,
                                                                   int64_t ti0, uint32_t nty, uint32_t ntx,
                                                                   uint32_t nrc, uint32_t ncc, int32_t prows, int32_t r,
                                                                   const int32_t *centers, int32_t cy_lo, int32_t cy_hi,
                                                                   int32_t cx_max, uint64_t *sums) {
  zs_tiles_at<false>(src, H, W, c0, nullptr, 0, r0, r1, y_org, Y, th, tw, gy, gx, ti0, nty, ntx, nrc, ncc, prows, r,
                     centers, cy_lo, cy_hi, cx_max, sums);
}

// Block b = (((pair * nty + ti) * ntx + tj) * nrc + rc) * ncc + cc: the sibling's index with the pair k of `pairs` in
// the place of the core plane; centers and sums are [npairs][gy][gx]... tables with a row per pair.
__global__ __launch_bounds__(ZS_THREADS) void u8_zshift_tiles_pairs_k(const uint8_t *src, int32_t D, int64_t H, int64_t W,
                                                                      int32_t z_org, const int32_t *pairs, int64_t r0,
                                                                      int64_t r1, int64_t y_org, int64_t Y, int64_t th,
                                                                      int64_t tw, int64_t gy, int64_t gx, int64_t ti0,
                                                                      uint32_t nty, uint32_t ntx, uint32_t nrc,
                                                                      uint32_t ncc, int32_t prows, int32_t r,
                                                                      const int32_t *centers, int32_t cy_lo,
                                                                      int32_t cy_hi, int32_t cx_max, uint64_t *sums) {
  zs_tiles_at<true>(src, H, W, z_org, pairs, D, r0, r1, y_org, Y, th, tw, gy, gx, ti0, nty, ntx, nrc, ncc, prows, r,
                    centers, cy_lo, cy_hi, cx_max, sums);
}

}  // namespace

extern "C" int tem_u8_zshift_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1,
                                   int32_t r0, int32_t r1, int32_t y_org, int32_t Y, int32_t th, int32_t tw, int32_t gy,
                                   int32_t gx, int32_t radius, uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !sums || ((uintptr_t)sums & 7) || D < 1 || H < 1 || W < 1 || Y < 1 || th < 1 || th > ZS_MAX_TILE ||
      tw < 1 || tw > ZS_MAX_TILE || gy < 1 || gx < 1 || radius < 1 || radius > ZS_MAX_R || y_org < 0 ||
      (int64_t)y_org + H > Y || Y > (int64_t)gy * th || W > (int64_t)gx * tw || c0 < 0 || c0 > c1 || c1 > D || r0 < 0 ||
      r0 > r1 || r1 > H)
    return TEM_EINVAL;
  if (r0 < r1) {                                                         // every partner row that the volume has
    const int64_t lo = (int64_t)r0 - radius > -(int64_t)y_org ? (int64_t)r0 - radius : -(int64_t)y_org;
    const int64_t hi = (int64_t)r1 + radius < (int64_t)Y - y_org ? (int64_t)r1 + radius : (int64_t)Y - y_org;
    if (lo < 0 || hi > H) return TEM_EINVAL;
  }
  int64_t ncore = c1 - c0;
  if (c1 == D) --ncore;                                                  // the block's last plane has no partner plane
  if (ncore <= 0 || r0 == r1) return TEM_OK;
  const int64_t ti0 = ((int64_t)y_org + r0) / th, nty = ((int64_t)y_org + r1 - 1) / th - ti0 + 1;
  const int64_t ntx = ((int64_t)W + tw - 1) / tw;
  const int64_t rows = th < r1 - r0 ? th : r1 - r0, width = tw < W ? tw : W;    // of a tile's part in the core, at most
  const int64_t cols = width < ZS_MAX_COLS ? width : ZS_MAX_COLS;
  const int64_t ncc = (width + ZS_MAX_COLS - 1) / ZS_MAX_COLS;
  int64_t prows = ZS_MAX_WORDS / ((cols + 3) / 4);                       // >= 32
  prows = prows > ZS_MAX_ROWS ? ZS_MAX_ROWS : prows;
  prows = prows > rows ? rows : prows;
  const int64_t nrc = (rows + prows - 1) / prows;
  const int64_t units = nty * ntx * nrc * ncc;                           // < 2^31 * 2^31 * 2^11 * 2^4
  if (units > 0x7fffffff || units * ncore > 0x7fffffff) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_zshift_tiles_k, dim3((unsigned)(units * ncore)), dim3(ZS_THREADS), 0, (hipStream_t)stream, src,
                     (int64_t)H, (int64_t)W, c0, (int64_t)r0, (int64_t)r1, (int64_t)y_org, (int64_t)Y, (int64_t)th,
                     (int64_t)tw, (int64_t)gy, (int64_t)gx, ti0, (uint32_t)nty, (uint32_t)ntx, (uint32_t)nrc,
                     (uint32_t)ncc, (int32_t)prows, radius, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}


namespace {

struct zs_grid {
  int64_t ti0, nty, ntx, nrc, ncc, prows, units;                         // units: workgroups per core plane or pair
};

// What tem_u8_zshift_tiles_at and tem_u8_zshift_tiles_pairs share: every check that does not speak of core planes or
// pairs, and the workgroups of one plane's core rows [r0, r1).
int zs_at_grid(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t r0, int32_t r1, int32_t y_org, int32_t Y,
               int32_t th, int32_t tw, int32_t gy, int32_t gx, int32_t radius, const int32_t *centers, int32_t cy_lo,
               int32_t cy_hi, int32_t cx_max, const uint64_t *sums, zs_grid *g) {
  if (!src || !sums || ((uintptr_t)sums & 7) || D < 1 || H < 1 || W < 1 || Y < 1 || th < 1 || th > ZS_MAX_TILE ||
      tw < 1 || tw > ZS_MAX_TILE || gy < 1 || gx < 1 || radius < 1 || radius > ZS_MAX_R || y_org < 0 ||
      (int64_t)y_org + H > Y || Y > (int64_t)gy * th || W > (int64_t)gx * tw || r0 < 0 || r0 > r1 || r1 > H)
    return TEM_EINVAL;
  if (!centers || ((uintptr_t)centers & 3) || cy_lo > 0 || cy_lo < -ZS_MAX_CENTER || cy_hi < 0 ||
      cy_hi > ZS_MAX_CENTER || cx_max < 0 || cx_max > ZS_MAX_CENTER)
    return TEM_EINVAL;
  if (r0 < r1) {                                                         // every partner row that the volume has
    const int64_t below = (int64_t)r0 - radius + cy_lo, above = (int64_t)r1 + radius + cy_hi;
    const int64_t lo = below > -(int64_t)y_org ? below : -(int64_t)y_org;
    const int64_t hi = above < (int64_t)Y - y_org ? above : (int64_t)Y - y_org;
    if (lo < 0 || hi > H) return TEM_EINVAL;
  }
  g->units = 0;
  if (r0 == r1) return TEM_OK;
  g->ti0 = ((int64_t)y_org + r0) / th, g->nty = ((int64_t)y_org + r1 - 1) / th - g->ti0 + 1;
  g->ntx = ((int64_t)W + tw - 1) / tw;
  const int64_t rows = th < r1 - r0 ? th : r1 - r0, width = tw < W ? tw : W;    // of a tile's part in the core, at most
  const int64_t cols = width < ZS_MAX_COLS ? width : ZS_MAX_COLS;
  g->ncc = (width + ZS_MAX_COLS - 1) / ZS_MAX_COLS;
  int64_t prows = ZS_MAX_WORDS / ((cols + 3) / 4);                       // >= 32
  prows = prows > ZS_MAX_ROWS ? ZS_MAX_ROWS : prows;
  g->prows = prows > rows ? rows : prows;
  g->nrc = (rows + g->prows - 1) / g->prows;
  g->units = g->nty * g->ntx * g->nrc * g->ncc;                          // < 2^31 * 2^31 * 2^11 * 2^4
  return TEM_OK;
}

}  // namespace

extern "C" int tem_u8_zshift_tiles_at(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1,
                                      int32_t r0, int32_t r1, int32_t y_org, int32_t Y, int32_t th, int32_t tw,
                                      int32_t gy, int32_t gx, int32_t radius, const int32_t *centers, int32_t cy_lo,
                                      int32_t cy_hi, int32_t cx_max, uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  zs_grid g;
  if (zs_at_grid(src, D, H, W, r0, r1, y_org, Y, th, tw, gy, gx, radius, centers, cy_lo, cy_hi, cx_max, sums, &g) !=
          TEM_OK || c0 < 0 || c0 > c1 || c1 > D)
    return TEM_EINVAL;
  int64_t ncore = c1 - c0;
  if (c1 == D) --ncore;                                                  // the block's last plane has no partner plane
  if (ncore <= 0 || g.units == 0) return TEM_OK;
  if (g.units > 0x7fffffff || g.units * ncore > 0x7fffffff) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_zshift_tiles_at_k, dim3((unsigned)(g.units * ncore)), dim3(ZS_THREADS), 0, (hipStream_t)stream,
                     src, (int64_t)H, (int64_t)W, c0, (int64_t)r0, (int64_t)r1, (int64_t)y_org, (int64_t)Y, (int64_t)th,
                     (int64_t)tw, (int64_t)gy, (int64_t)gx, g.ti0, (uint32_t)g.nty, (uint32_t)g.ntx, (uint32_t)g.nrc,
                     (uint32_t)g.ncc, (int32_t)g.prows, radius, centers, cy_lo, cy_hi, cx_max, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_zshift_tiles_pairs(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t z_org,
                                         int32_t npairs, const int32_t *pairs, int32_t r0, int32_t r1, int32_t y_org,
                                         int32_t Y, int32_t th, int32_t tw, int32_t gy, int32_t gx, int32_t radius,
                                         const int32_t *centers, int32_t cy_lo, int32_t cy_hi, int32_t cx_max,
                                         uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  zs_grid g;
  if (zs_at_grid(src, D, H, W, r0, r1, y_org, Y, th, tw, gy, gx, radius, centers, cy_lo, cy_hi, cx_max, sums, &g) !=
          TEM_OK || !pairs || ((uintptr_t)pairs & 3) || npairs < 0)
    return TEM_EINVAL;
  if (npairs == 0 || g.units == 0) return TEM_OK;
  if (g.units > 0x7fffffff || g.units * npairs > 0x7fffffff) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_zshift_tiles_pairs_k, dim3((unsigned)(g.units * npairs)), dim3(ZS_THREADS), 0,
                     (hipStream_t)stream, src, D, (int64_t)H, (int64_t)W, z_org, pairs, (int64_t)r0, (int64_t)r1,
                     (int64_t)y_org, (int64_t)Y, (int64_t)th, (int64_t)tw, (int64_t)gy, (int64_t)gx, g.ti0,
                     (uint32_t)g.nty, (uint32_t)g.ntx, (uint32_t)g.nrc, (uint32_t)g.ncc, (int32_t)g.prows, radius,
                     centers, cy_lo, cy_hi, cx_max, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
