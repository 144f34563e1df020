// zcorr_u8.hip -- the sums behind the correlation of every tile of a uint8 section with the same tile one section up
// (utils.section_sums -> section_scores -> find_defects):
//   tem_u8_zcorr_tiles   sums[d - c0][i][j][0..3] += sum v, sum v v, sum v v+, count over the voxels of tile (i, j) of
//                        core plane d, v+ the voxel one plane up (no pair term for the block's last plane)
// The tile grid is tem_u8_hist_tiles': anchored at (0, 0) of the caller's VOLUME, the block's voxel (d, y, x) at
// in-plane volume coordinates (y_org + y, x_org + x).  Everything is integers and the adds are atomic, so the sums do
// not depend on how the volume was cut into blocks or the block into workgroups.
//
// A workgroup of 256 threads owns a PART -- up to ZC_ITEMS 16-byte pieces: a run of rows of the part of one tile that
// lies in the block, each row cut into pieces [16 s, 16 s + 16) counted from the tile part's first column -- and a RUN
// of up to `zr` core planes.  A thread owns ZC_K pieces (piece i = thread + 256 k, the same in every plane).  It
// marches its run along z with the words of the current plane in registers: per plane it loads only the plane above,
// so a run of n planes loads n + 1 (the one above the run is the halo; the block's last plane has none and gets no
// pair term).  Per 4-byte word the three sums are three packed byte dot products (v_dot4_u32_u8): against the word
// above, against itself, against 0x01010101.  The count needs no sum: rows x width of the part.
//
// Loads.  A piece starts at any address.  One that starts on a 16-byte boundary travels as one dwordx4; any other as
// the (up to five) naturally aligned dwords that hold at least one of its bytes, funnel-shifted (v_alignbyte_b32) into
// the piece's four words.  Either way only aligned words that hold a byte of the block are touched, and the bytes past
// the piece's end (the tile's or the block's edge) are masked to zero: a zero voxel adds nothing to any of the three
// sums, below or above.
//
// No partial can overflow.  A thread sums at most ZC_K x 16 = 64 voxels per plane in 32 bits, each at most 255 x 255:
// 64 x 65025 < 2^23.  A wave sums 64 such partials in 32 bits: < 2^29.  The four wave sums are widened to 64 bits in
// LDS (a part holds at most ZC_ITEMS x 16 = 16384 voxels, so even they would fit: 16384 x 65025 < 2^31) and added to
// `sums` with ONE 64-bit global atomic add (an ordinary vector atomic) per workgroup, plane and quantity.  The
// 64-bit counters take the rest: a whole 2048 x 2048 tile of 255s is 2^22 x 65025 < 2^38 per plane, and a volume
// would need 2^25 such tiles on top of each other to pass 2^63.
#include "zc_pieces.h"

namespace {

constexpr int ZC_K = 4;                          // pieces per thread
constexpr int ZC_ITEMS = ZC_THREADS * ZC_K;      // pieces per part, at most
constexpr int ZC_MAX_RUN = 16;                   // planes per run, at most: 17 planes loaded for 16 counted

// Block b = ((run * nty + ti) * ntx + tj) * parts + part: rows [part * rpp, (part + 1) * rpp) of the part of tile
// (ti0 + ti, tj0 + tj) that lies in the block, core planes [c0 + run * zr, min(c0 + (run + 1) * zr, c1)).
// S: pieces per row, ceil(width / 16) of the widest tile part; magicS = magic_for(S).  rpp * S <= ZC_ITEMS.
__global__ __launch_bounds__(ZC_THREADS) void u8_zcorr_tiles_k(const uint8_t *src, int32_t D, int64_t H, int64_t W,
                                                               int32_t c0, int32_t c1, int64_t y_org, int64_t x_org,
                                                               int64_t th, int64_t tw, int64_t gy, int64_t gx,
                                                               int64_t ti0, int64_t tj0, uint32_t nty, uint32_t ntx,
                                                               uint32_t parts, int64_t rpp, uint32_t S, uint32_t magicS,
                                                               int32_t zr, uint64_t *sums) {
  __shared__ uint32_t red[2][ZC_THREADS / 64][3];
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
  const uint32_t total = (uint32_t)(yb - ya) * S;                        // <= ZC_ITEMS
  const int32_t z0 = c0 + (int32_t)run * zr, z1 = min(z0 + zr, c1);
  const int64_t plane = H * W;
  const uint8_t *first = src + ((int64_t)z0 * H + ya) * W + xa;

  int64_t off[ZC_K];                                                     // piece k of this thread: its offset in a plane
  int32_t cnt[ZC_K];                                                     // and its bytes, 0: none
  uint32_t cur[ZC_K][4];
#pragma unroll
  for (int k = 0; k < ZC_K; ++k) {
    const uint32_t i = threadIdx.x + ZC_THREADS * k;
    const uint32_t ri = S == 1 ? i : __umulhi(i, magicS), s = i - ri * S;
    const int32_t lo = 16 * (int32_t)s;
    cnt[k] = i < total && lo < width ? min(16, width - lo) : 0;
    off[k] = (int64_t)ri * W + lo;
    cur[k][0] = cur[k][1] = cur[k][2] = cur[k][3] = 0;
    if (cnt[k]) zc_load(first + off[k], cnt[k], cur[k]);
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t nvox = (uint64_t)(yb - ya) * (uint64_t)width;
  for (int32_t d = z0; d < z1; ++d) {
    const bool pair = d + 1 < D;
    const uint8_t *up = first + (int64_t)(d + 1 - z0) * plane;
    uint32_t nxt[ZC_K][4];
#pragma unroll
    for (int k = 0; k < ZC_K; ++k) {
      nxt[k][0] = nxt[k][1] = nxt[k][2] = nxt[k][3] = 0;
      if (pair && cnt[k]) zc_load(up + off[k], cnt[k], nxt[k]);
    }
    uint32_t s1 = 0, s2 = 0, s12 = 0;
#pragma unroll
    for (int k = 0; k < ZC_K; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s1 = __builtin_amdgcn_udot4(cur[k][j], 0x01010101u, s1, false);
        s2 = __builtin_amdgcn_udot4(cur[k][j], cur[k][j], s2, false);
        s12 = __builtin_amdgcn_udot4(cur[k][j], nxt[k][j], s12, false);
        cur[k][j] = nxt[k][j];
      }
    }
    s1 = zc_wave_sum(s1), s2 = zc_wave_sum(s2), s12 = zc_wave_sum(s12);
    // two copies of the wave sums, by the plane's parity: one barrier per plane (whoever writes copy p again has
    // passed the barrier of the plane in between, behind which no thread still reads the older copy p)
    const int par = (d - z0) & 1;
    if (lane == 0) red[par][wave][0] = s1, red[par][wave][1] = s2, red[par][wave][2] = s12;
    __syncthreads();
    if (threadIdx.x < 4) {
      uint64_t v = nvox;
      if (threadIdx.x < 3) {
        v = 0;
#pragma unroll
        for (int wv = 0; wv < ZC_THREADS / 64; ++wv) v += red[par][wv][threadIdx.x];
      }
      uint64_t *q = sums + ((((int64_t)(d - c0) * gy + ti) * gx + tj) * 4 + threadIdx.x);
      if (v) atomicAdd(reinterpret_cast<unsigned long long *>(q), (unsigned long long)v);
    }
  }
}

}  // namespace

extern "C" int tem_u8_zcorr_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1,
                                  int32_t y_org, int32_t x_org, int32_t th, int32_t tw, int32_t gy, int32_t gx,
                                  uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !sums || ((uintptr_t)sums & 7) || D < 1 || H < 1 || W < 1 || th < 1 || th > ZC_MAX_TILE || tw < 1 ||
      tw > ZC_MAX_TILE || gy < 1 || gx < 1 || y_org < 0 || x_org < 0 || (int64_t)y_org + H > (int64_t)gy * th ||
      (int64_t)x_org + W > (int64_t)gx * tw || c0 < 0 || c0 > c1 || c1 > D)
    return TEM_EINVAL;
  if (c0 == c1) return TEM_OK;
  const int64_t ti0 = y_org / th, tj0 = x_org / tw;
  const int64_t nty = ((int64_t)y_org + H - 1) / th - ti0 + 1, ntx = ((int64_t)x_org + W - 1) / tw - tj0 + 1;
  const int64_t rows = th < H ? th : H, width = tw < W ? tw : W;        // of a tile's part in the block, at most
  const int64_t S = (width + 15) / 16;                                   // <= 128
  const int64_t rpp = ZC_ITEMS / S;                                      // >= 8
  const int64_t parts = (rows + rpp - 1) / rpp;
  const int64_t units = nty * ntx * parts, ncore = c1 - c0;              // < 2^31 * 2^31 * 2^8
  if (units > 0x7fffffff) return TEM_EUNSUPPORTED;
  // the run: as long as leaves about ZC_WANT_GRID workgroups, ZC_MAX_RUN planes at most
  int64_t zr = ncore * units / ZC_WANT_GRID;
  zr = zr < 1 ? 1 : (zr > ZC_MAX_RUN ? ZC_MAX_RUN : zr);
  const int64_t nruns = (ncore + zr - 1) / zr;
  if (units * nruns > 0x7fffffff) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_zcorr_tiles_k, dim3((unsigned)(units * nruns)), dim3(ZC_THREADS), 0, (hipStream_t)stream, src,
                     D, (int64_t)H, (int64_t)W, c0, c1, (int64_t)y_org, (int64_t)x_org, (int64_t)th, (int64_t)tw,
                     (int64_t)gy, (int64_t)gx, ti0, tj0, (uint32_t)nty, (uint32_t)ntx, (uint32_t)parts, rpp,
                     (uint32_t)S, magic_for((int)S), (int32_t)zr, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
