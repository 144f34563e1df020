// zplane_u8.hip -- the sums behind the correlation of every tile of a uint8 section with ITSELF displaced by 1...nlag
// pixels along y and along x (utils.section_plane_sums -> plane_scores -> section_sharpness / find_blurred: sections
// that are out of focus; plane_curve -> z_pitch: how many pixels thick a section is):
//   tem_u8_zplane_lags   sums[d - c0][i][j][0 .. 2 + 2 nlag] += sum v, sum v v, count, sum (v - w)^2 for the partner w
//                        k rows down (k = 1...nlag), then for the partner k columns to the right, over the core voxels v
//                        of tile (i, j) of plane d whose partner lies in the section (include/tem_hip.h)
// tem_u8_zshift_tiles' block contract (zshift_u8.hip): whole rows at volume row y_org of a section of Y rows, core planes
// and core rows, the tile grid of tem_u8_hist_tiles; zc_pieces.h' loads; 64-bit atomic adds.
//
// The WAVE is the unit of work, and it is tem_u8_zcorr_lags' ring turned from z to y.  A lane owns a 16-byte PIECE of a
// row and marches a RUN of up to ZP_ROWS = 16 rows down with a ring of nlag + 1 rows in registers: ring[0] is the row
// counted, ring[k] the row k below it; per row it loads only row y + nlag into the ring's last slot and moves the ring
// up one slot.  A row is held as SIX words, 16 + 8 bytes: the two words behind the piece are where the x partners of
// its last bytes lie, so the x lags come from the row the lane already holds -- the partner words of lag k are
// v_alignbyte_b32(r[j + 1 + (k >> 2)], r[j + (k >> 2)], k & 3).  The kernel is a template on nlag: every ring index and
// every byte shift is a constant after unrolling and nothing is indexed at run time -- no scratch.  (nlag as a launch
// constant would keep a ring of nine rows whatever nlag is and move 48 registers per row.)
//
// A wave's 64 lanes are NR runs x SC pieces: SC = the pieces of a row of a tile's part (at most 64: 1024 columns, a
// wider tile is cut into column chunks), NR = 64 / SC runs below each other.  The run length R is ceil(rows / NR), at
// most 16: a whole 128 x 128 tile is ONE wave (8 pieces x 8 runs of 16 rows), and at nlag = 8 a row is loaded
// (16 + 8) / 16 = 1.5 times; tiles with fewer rows than NR x 2 nlag reload more, out of the cache.  The four waves of a
// workgroup are four consecutive core PLANES of the same part: a wave sums its lanes (zc_wave_sum) and adds ONE 64-bit
// global atomic (an ordinary vector atomic) per quantity -- one per workgroup, plane and quantity -- so no LDS and no
// barrier is needed.
//
// Sum (v - w)^2 in packed byte dot products (v_dot4_u32_u8).  Over the pairs that exist it is sum v v + sum w w -
// 2 sum v w.  Along y a pair exists for a whole row or not at all, and sum w w of the row k down is sum v v of that
// row: it is taken once per row when the row enters the ring, so a y lag costs ONE dot product per word.  Along x, w
// is the row shifted: two dot products per word and lag (w w, v w) where every partner exists and the piece is whole
// (sum v v is the row's); a piece that the tile cuts short or that lies within nlag of the section's right edge masks
// the bytes without a pair in v and in w and takes all three.  Every 32-bit partial is a sum of a^2 + b^2 - 2 a b >= 0.
//
// No partial can overflow at (v - w)^2 <= 65025: a lane sums at most 16 rows x 16 bytes = 256 terms in 32 bits
// (256 x 65025 < 2^24; the intermediate sum v v + sum w w of one row < 2^22), a wave 64 such partials (< 2^30), which
// is widened to 64 bits for the global add; a whole 2048 x 2048 tile of 255s next to 0s is 2^22 x 65025 < 2^38.
#include "zc_pieces.h"

namespace {

constexpr int ZP_MAX_LAG = 8;
constexpr int ZP_ROWS = 16;                       // rows of a lane's run, at most
constexpr int ZP_PLANES = ZC_THREADS / 64;        // a workgroup's waves: consecutive core planes of one part
constexpr int ZP_COLS = 64 * 16;                  // columns of a wave's part, at most
constexpr int64_t ZP_MAX_WGS = (int64_t)1 << 24;  // workgroups of one launch: their 256 threads stay below 2^32

// 0xff in the bytes b < n of a word, for any n
__device__ __forceinline__ uint32_t zp_low(int n) { return n >= 4 ? 0xffffffffu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u); }

// The n (0...8) bytes at p as two words, the bytes past n zero: zc_load's rule for the words behind a piece.
__device__ __forceinline__ void zp_load_tail(const uint8_t *p, int n, uint32_t (&w)[2]) {
  const uint32_t a = (uint32_t)((uintptr_t)p & 3);
  const uint32_t *q = reinterpret_cast<const uint32_t *>(p - a);
  uint32_t r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) r[j] = n > 0 && 4 * j < (int)a + n ? q[j] : 0u;  // word j: bytes [4 j - a, 4 j + 4 - a)
#pragma unroll
  for (int j = 0; j < 2; ++j) w[j] = __builtin_amdgcn_alignbyte(r[j + 1], r[j], a) & zp_low(n - 4 * j);
}

// Block b = (((pg * nty + ti) * ntx + tj) * nrc + rc) * ncc + cc: core planes c0 + 4 pg + wave, rows
// [rc * NR * R, (rc + 1) * NR * R) and columns [cc * ZP_COLS, (cc + 1) * ZP_COLS) of the part of tile (ti0 + ti, tj)
// that lies in the core rows [r0, r1).  NR * SC <= 64.
template <int NLAG>
__global__ __launch_bounds__(ZC_THREADS) void u8_zplane_lags_k(const uint8_t *src, int64_t H, int64_t W, int32_t c0,
                                                               int32_t c1, int64_t r0, int64_t r1, int64_t y_org,
                                                               int64_t Y, int64_t th, int64_t tw, int64_t gy, int64_t gx,
                                                               int64_t ti0, uint32_t nty, uint32_t ntx, uint32_t nrc,
                                                               uint32_t ncc, uint32_t SC, uint32_t NR, int32_t R,
                                                               uint64_t *sums) {
  constexpr int Q = 2 + 2 * NLAG;                                        // sums that are summed: the count is geometry
  uint32_t b = blockIdx.x;
  const uint32_t cc = b % ncc;
  b /= ncc;
  const uint32_t rc = b % nrc;
  b /= nrc;
  const uint32_t tj = b % ntx;
  b /= ntx;
  const uint32_t til = b % nty, pg = b / nty;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t lane = threadIdx.x & 63;
  const int32_t d = c0 + ZP_PLANES * (int32_t)pg + wave;
  if (d >= c1) return;                                                   // the whole wave
  const int64_t ti = ti0 + til, prw = (int64_t)NR * R;
  const int64_t ya = max(ti * th - y_org, r0) + (int64_t)rc * prw;
  const int64_t yb = min(min((ti + 1) * th - y_org, r1), ya + prw);
  const int64_t xa = (int64_t)tj * tw + (int64_t)cc * ZP_COLS;
  const int64_t xb = min(min((int64_t)(tj + 1) * tw, W), xa + ZP_COLS);
  if (ya >= yb || xa >= xb) return;                                      // the whole workgroup: the tail part of a cut tile
  const int32_t width = (int32_t)(xb - xa);
  const uint32_t rr = lane / SC, s = lane - rr * SC;
  const int32_t lo = 16 * (int32_t)s;
  const int32_t cnt = rr < NR && lo < width ? min(16, width - lo) : 0;  // the piece's bytes, 0: an idle lane
  const int64_t ys = ya + (int64_t)rr * R, ye = cnt ? min(ys + R, yb) : ys;        // the lane's run of rows
  const int32_t rem = (int32_t)min(W - xa - lo, (int64_t)64);            // bytes from the piece's first to the row's end
  const int32_t nload = min(min(cnt + NLAG, rem), 24);                   // the piece and the partners behind it
  const bool whole = cnt == 16 && rem >= 16 + NLAG;                      // no byte of the piece is without an x partner
  const int64_t Hs = Y - y_org;                                          // the section's rows end here, in block rows
  const uint8_t *first = src + ((int64_t)d * H + ys) * W + xa + lo;
  uint32_t cm[4];                                                        // the piece's bytes in its four words
#pragma unroll
  for (int j = 0; j < 4; ++j) cm[j] = zp_low(cnt - 4 * j);

  uint32_t ring[NLAG + 1][6], vv[NLAG + 1];                              // vv: sum v v over the piece's bytes of the row
  auto fetch = [&](int64_t row, uint32_t (&r)[6], uint32_t &sq) {        // a row that exists is in the block: the contract
    r[0] = r[1] = r[2] = r[3] = r[4] = r[5] = 0, sq = 0;
    if (row < Hs) {                                                      // row < min(r1 + NLAG, Hs) <= H
      uint32_t a[4], t[2];
      const uint8_t *p = first + (row - ys) * W;
      zc_load(p, min(nload, 16), a);
      zp_load_tail(p + 16, nload - 16, t);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = a[j];
        sq = __builtin_amdgcn_udot4(a[j] & cm[j], a[j] & cm[j], sq, false);
      }
      r[4] = t[0], r[5] = t[1];
    }
  };
  // the word behind word i of the row counted; lag 8 moves by whole words and never looks at the one behind the sixth
  auto next = [&](int i) { return i + 1 < 6 ? ring[0][i + 1 < 6 ? i + 1 : 5] : 0u; };
  uint32_t acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0;
  if (ys < ye) {
#pragma unroll
    for (int l = 0; l < NLAG; ++l) fetch(ys + l, ring[l], vv[l]);
  }
  for (int64_t y = ys; y < ye; ++y) {
    fetch(y + NLAG, ring[NLAG], vv[NLAG]);
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = ring[0][j] & cm[j];
      acc[0] = __builtin_amdgcn_udot4(v[j], 0x01010101u, acc[0], false);
    }
    acc[1] += vv[0];
#pragma unroll
    for (int k = 1; k <= NLAG; ++k) {                                    // the partner k rows down: the same columns
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_udot4(v[j], ring[k][j], c, false);
      acc[1 + k] += y + k < Hs ? vv[0] + vv[k] - 2 * c : 0u;
    }
    if (whole) {
#pragma unroll
      for (int k = 1; k <= NLAG; ++k) {                                  // the partner k columns to the right
        uint32_t t = vv[0], c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t hi = next(j + (k >> 2));
          const uint32_t w = __builtin_amdgcn_alignbyte(hi, ring[0][j + (k >> 2)], k & 3);
          t = __builtin_amdgcn_udot4(w, w, t, false);
          c = __builtin_amdgcn_udot4(v[j], w, c, false);
        }
        acc[1 + NLAG + k] += t - 2 * c;
      }
    } else {
#pragma unroll
      for (int k = 1; k <= NLAG; ++k) {                                  // a byte mask drops the pairs that do not exist
        const int32_t lim = min(cnt, rem - k);                           // the piece's bytes b with b + k in the section
        uint32_t t = 0, c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t hi = next(j + (k >> 2));
          const uint32_t pm = zp_low(lim - 4 * j);
          const uint32_t w = __builtin_amdgcn_alignbyte(hi, ring[0][j + (k >> 2)], k & 3) & pm, vm = v[j] & pm;
          t = __builtin_amdgcn_udot4(vm, vm, t, false);
          t = __builtin_amdgcn_udot4(w, w, t, false);
          c = __builtin_amdgcn_udot4(vm, w, c, false);
        }
        acc[1 + NLAG + k] += t - 2 * c;
      }
    }
#pragma unroll
    for (int l = 0; l < NLAG; ++l) {                                     // the ring moves up one row
      vv[l] = vv[l + 1];
#pragma unroll
      for (int j = 0; j < 6; ++j) ring[l][j] = ring[l + 1][j];
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = zc_wave_sum(acc[q]);
  // columns: sum v, sum v v, n, the nlag y sums, the nlag x sums -- lane t adds column t (a select chain, not acc[t])
  uint64_t val = lane == 2 ? (uint64_t)(yb - ya) * (uint64_t)width : 0;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (lane == (uint32_t)(q < 2 ? q : q + 1)) val = acc[q];
  if (lane < Q + 1 && val) {
    uint64_t *p = sums + ((((int64_t)(d - c0) * gy + ti) * gx + tj) * (Q + 1) + lane);
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)val);
  }
}

template <int NLAG>
int zplane_launch(const uint8_t *src, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t r0, int32_t r1,
                  int32_t y_org, int32_t Y, int32_t th, int32_t tw, int32_t gy, int32_t gx, uint64_t *sums,
                  hipStream_t stream) {
  const int64_t ti0 = ((int64_t)y_org + r0) / th, nty = ((int64_t)y_org + r1 - 1) / th - ti0 + 1;
  const int64_t ntx = ((int64_t)W + tw - 1) / tw;
  const int64_t rows = th < r1 - r0 ? th : r1 - r0, width = tw < W ? tw : W;    // of a tile's part in the core, at most
  const int64_t cols = width < ZP_COLS ? width : ZP_COLS, ncc = (width + ZP_COLS - 1) / ZP_COLS;
  const int64_t SC = (cols + 15) / 16, NR = 64 / SC;                     // 1...64 pieces, 64...1 runs
  int64_t R = (rows + NR - 1) / NR;
  R = R > ZP_ROWS ? ZP_ROWS : R;                                         // >= 1
  const int64_t nrc = (rows + NR * R - 1) / (NR * R);
  const int64_t units = nty * ntx * nrc * ncc;                           // < 2^31 * 2^31 * 2^11 * 2
  const int64_t npg = ((int64_t)c1 - c0 + ZP_PLANES - 1) / ZP_PLANES;
  if (units >= ZP_MAX_WGS || units * npg >= ZP_MAX_WGS) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL((u8_zplane_lags_k<NLAG>), dim3((unsigned)(units * npg)), dim3(ZC_THREADS), 0, stream, src,
                     (int64_t)H, (int64_t)W, c0, c1, (int64_t)r0, (int64_t)r1, (int64_t)y_org, (int64_t)Y, (int64_t)th,
                     (int64_t)tw, (int64_t)gy, (int64_t)gx, ti0, (uint32_t)nty, (uint32_t)ntx, (uint32_t)nrc,
                     (uint32_t)ncc, (uint32_t)SC, (uint32_t)NR, (int32_t)R, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

}  // namespace

extern "C" int tem_u8_zplane_lags(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1,
                                  int32_t r0, int32_t r1, int32_t y_org, int32_t Y, int32_t th, int32_t tw, int32_t gy,
                                  int32_t gx, int32_t nlag, uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !sums || ((uintptr_t)sums & 7) || D < 1 || H < 1 || W < 1 || Y < 1 || th < 1 || th > ZC_MAX_TILE ||
      tw < 1 || tw > ZC_MAX_TILE || gy < 1 || gx < 1 || nlag < 1 || nlag > ZP_MAX_LAG || y_org < 0 ||
      (int64_t)y_org + H > Y || Y > (int64_t)gy * th || W > (int64_t)gx * tw || c0 < 0 || c0 > c1 || c1 > D || r0 < 0 ||
      r0 > r1 || r1 > H)
    return TEM_EINVAL;
  if (r0 < r1) {                                                         // every partner row that the section has
    const int64_t hi = (int64_t)r1 + nlag < (int64_t)Y - y_org ? (int64_t)r1 + nlag : (int64_t)Y - y_org;
    if (hi > H) return TEM_EINVAL;
  }
  if (c0 == c1 || r0 == r1) return TEM_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (nlag) {
    case 1: return zplane_launch<1>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    case 2: return zplane_launch<2>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    case 3: return zplane_launch<3>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    case 4: return zplane_launch<4>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    case 5: return zplane_launch<5>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    case 6: return zplane_launch<6>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    case 7: return zplane_launch<7>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
    default: return zplane_launch<8>(src, H, W, c0, c1, r0, r1, y_org, Y, th, tw, gy, gx, sums, s);
  }
}
