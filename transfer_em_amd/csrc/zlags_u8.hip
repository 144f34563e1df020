// zlags_u8.hip -- the sums behind the correlation of every tile of a uint8 section with the same tile 1...nlag sections
// up (utils.section_lag_sums -> lag_scores -> section_spacing: how fast correlation decays with the lag is how far
// sections sit apart along z):
//   tem_u8_zcorr_lags    sums[d - c0][i][j][0 .. 2 + nlag] += sum v, sum v v, count, sum v v+1, ..., sum v v+nlag over the
//                        voxels of tile (i, j) of core plane d, v+k the voxel k planes up (no term k where d + k >= D)
// tem_u8_zcorr_tiles' contract (zcorr_u8.hip) with nlag partners instead of one: its tile grid, block, core, loads
// (zc_pieces.h) and adds.
//
// A workgroup of 256 threads owns a PART -- up to 256 K 16-byte pieces: a run of rows of the part of one tile that lies
// in the block, each row cut into pieces counted from the tile part's first column -- and a RUN of up to `zr` core
// planes.  A thread owns K pieces (piece i = thread + 256 k, the same in every plane) and marches its run along z with a
// RING of nlag + 1 planes' words in registers: ring[0] is the plane counted, ring[k] the plane k above it.  Per plane it
// loads only plane d + nlag into the ring's last slot, takes per 4-byte word nlag + 2 packed byte dot products
// (v_dot4_u32_u8: against 0x01010101, itself, and the nlag words above) and moves the ring down one slot.  The kernel is
// a template on nlag, every ring index is a constant after unrolling, and nothing is indexed at run time: no scratch.
// A plane at or past D is a ring slot of zeros, and a zero voxel adds nothing to any sum: that is the rule d + k < D.
//
// Registers.  The ring holds (nlag + 1) x K x 4 words.  K = 4 for nlag <= 4 (at most 80 words), K = 2 above (at most 72),
// so that the ring, one piece's five load words, the offsets and the sums stay far below the 512 registers of a lane.
//
// The run.  A run of n planes loads n + nlag.  As the sibling, the run is as long as leaves about ZC_WANT_GRID
// workgroups; where that is shorter than 2 nlag planes -- the halo a third of the loads or more -- it is lengthened up to
// 2 nlag as far as about half that many workgroups remain.  At most 24 + 8 nlag planes (32...88): the halo is then at
// most 1 / 12 of the loads.
//
// No partial can overflow, by the sibling's argument: a thread sums at most K x 16 <= 64 voxels per plane in 32 bits
// (64 x 65025 < 2^23), a wave 64 such partials (< 2^29), the four wave sums are widened to 64 bits in LDS and added
// with ONE 64-bit global atomic add (an ordinary vector atomic) per workgroup, plane and quantity.
#include "zc_pieces.h"

namespace {

constexpr int ZLAG_MAX = 8;
constexpr int64_t ZLAG_MAX_WGS = (int64_t)1 << 24;   // workgroups of one launch: their 256 threads stay below 2^32

// Block b = ((run * nty + ti) * ntx + tj) * parts + part, as u8_zcorr_tiles_k.  rpp * S <= ZC_THREADS * K.
template <int NLAG, int K>
__global__ __launch_bounds__(ZC_THREADS) void u8_zcorr_lags_k(const uint8_t *src, int32_t D, int64_t H, int64_t W,
                                                              int32_t c0, int32_t c1, int64_t y_org, int64_t x_org,
                                                              int64_t th, int64_t tw, int64_t gy, int64_t gx,
                                                              int64_t ti0, int64_t tj0, uint32_t nty, uint32_t ntx,
                                                              uint32_t parts, int64_t rpp, uint32_t S, uint32_t magicS,
                                                              int32_t zr, uint64_t *sums) {
  constexpr int Q = NLAG + 2;                                            // sums that are summed: the count is geometry
  __shared__ uint32_t red[2][ZC_THREADS / 64][Q];
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
  const uint32_t total = (uint32_t)(yb - ya) * S;                        // <= ZC_THREADS * K
  const int32_t z0 = c0 + (int32_t)run * zr, z1 = min(z0 + zr, c1);
  const int64_t plane = H * W;
  const uint8_t *first = src + ((int64_t)z0 * H + ya) * W + xa;

  int64_t off[K];                                                        // piece k of this thread: its offset in a plane
  int32_t cnt[K];                                                        // and its bytes, 0: none
  uint32_t ring[NLAG + 1][K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t i = threadIdx.x + ZC_THREADS * k;
    const uint32_t ri = S == 1 ? i : __umulhi(i, magicS), s = i - ri * S;
    const int32_t lo = 16 * (int32_t)s;
    cnt[k] = i < total && lo < width ? min(16, width - lo) : 0;
    off[k] = (int64_t)ri * W + lo;
  }
#pragma unroll
  for (int l = 0; l < NLAG; ++l) {                                       // planes z0 ... z0 + nlag - 1, those that exist
    const bool have = z0 + l < D;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ring[l][k][0] = ring[l][k][1] = ring[l][k][2] = ring[l][k][3] = 0;
      if (have && cnt[k]) zc_load(first + (int64_t)l * plane + off[k], cnt[k], ring[l][k]);
    }
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t nvox = (uint64_t)(yb - ya) * (uint64_t)width;
  for (int32_t d = z0; d < z1; ++d) {
    const bool have = d + NLAG < D;
    const uint8_t *up = first + (int64_t)(d + NLAG - z0) * plane;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ring[NLAG][k][0] = ring[NLAG][k][1] = ring[NLAG][k][2] = ring[NLAG][k][3] = 0;
      if (have && cnt[k]) zc_load(up + off[k], cnt[k], ring[NLAG][k]);
    }
    uint32_t acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t v = ring[0][k][j];
        acc[0] = __builtin_amdgcn_udot4(v, 0x01010101u, acc[0], false);
        acc[1] = __builtin_amdgcn_udot4(v, v, acc[1], false);
#pragma unroll
        for (int l = 1; l <= NLAG; ++l) acc[1 + l] = __builtin_amdgcn_udot4(v, ring[l][k][j], acc[1 + l], false);
#pragma unroll
        for (int l = 0; l < NLAG; ++l) ring[l][k][j] = ring[l + 1][k][j];          // the ring moves down one plane
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = zc_wave_sum(acc[q]);
    // two copies of the wave sums, by the plane's parity: one barrier per plane, as u8_zcorr_tiles_k
    const int par = (d - z0) & 1;
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q) red[par][wave][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < Q + 1) {                                           // columns: sum v, sum v v, n, the nlag pair sums
      const int q = threadIdx.x < 2 ? (int)threadIdx.x : (int)threadIdx.x - 1;
      uint64_t v = nvox;
      if (threadIdx.x != 2) {
        v = 0;
#pragma unroll
        for (int wv = 0; wv < ZC_THREADS / 64; ++wv) v += red[par][wv][q];
      }
      uint64_t *p = sums + ((((int64_t)(d - c0) * gy + ti) * gx + tj) * (Q + 1) + threadIdx.x);
      if (v) atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    }
  }
}

template <int NLAG>
int zlags_launch(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t y_org,
                 int32_t x_org, int32_t th, int32_t tw, int32_t gy, int32_t gx, uint64_t *sums, hipStream_t stream) {
  constexpr int K = NLAG <= 4 ? 4 : 2;
  constexpr int ITEMS = ZC_THREADS * K, MAX_RUN = 24 + 8 * NLAG;
  const int64_t ti0 = y_org / th, tj0 = x_org / tw;
  const int64_t nty = ((int64_t)y_org + H - 1) / th - ti0 + 1, ntx = ((int64_t)x_org + W - 1) / tw - tj0 + 1;
  const int64_t rows = th < H ? th : H, width = tw < W ? tw : W;        // of a tile's part in the block, at most
  const int64_t S = (width + 15) / 16;                                   // <= 128
  const int64_t rpp = ITEMS / S;                                         // >= 4
  const int64_t parts = (rows + rpp - 1) / rpp;
  const int64_t units = nty * ntx * parts, ncore = c1 - c0;              // < 2^31 * 2^31 * 2^9
  if (units >= ZLAG_MAX_WGS) return TEM_EUNSUPPORTED;
  int64_t zr = ncore * units / ZC_WANT_GRID;
  if (zr < 2 * NLAG) {                                                   // the halo: at most a third, at half the grid
    const int64_t longer = ncore * units / (ZC_WANT_GRID / 2);
    zr = longer < zr ? zr : (longer > 2 * NLAG ? 2 * NLAG : longer);
  }
  zr = zr < 1 ? 1 : (zr > MAX_RUN ? MAX_RUN : zr);
  const int64_t nruns = (ncore + zr - 1) / zr;
  if (units * nruns >= ZLAG_MAX_WGS) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL((u8_zcorr_lags_k<NLAG, K>), dim3((unsigned)(units * nruns)), dim3(ZC_THREADS), 0, stream, src, D,
                     (int64_t)H, (int64_t)W, c0, c1, (int64_t)y_org, (int64_t)x_org, (int64_t)th, (int64_t)tw,
                     (int64_t)gy, (int64_t)gx, ti0, tj0, (uint32_t)nty, (uint32_t)ntx, (uint32_t)parts, rpp,
                     (uint32_t)S, magic_for((int)S), (int32_t)zr, sums);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

}  // namespace

extern "C" int tem_u8_zcorr_lags(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1,
                                 int32_t y_org, int32_t x_org, int32_t th, int32_t tw, int32_t gy, int32_t gx,
                                 int32_t nlag, uint64_t *sums, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !sums || ((uintptr_t)sums & 7) || D < 1 || H < 1 || W < 1 || th < 1 || th > ZC_MAX_TILE || tw < 1 ||
      tw > ZC_MAX_TILE || gy < 1 || gx < 1 || y_org < 0 || x_org < 0 || (int64_t)y_org + H > (int64_t)gy * th ||
      (int64_t)x_org + W > (int64_t)gx * tw || c0 < 0 || c0 > c1 || c1 > D || nlag < 1 || nlag > ZLAG_MAX)
    return TEM_EINVAL;
  if (c0 == c1) return TEM_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (nlag) {
    case 1: return zlags_launch<1>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    case 2: return zlags_launch<2>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    case 3: return zlags_launch<3>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    case 4: return zlags_launch<4>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    case 5: return zlags_launch<5>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    case 6: return zlags_launch<6>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    case 7: return zlags_launch<7>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
    default: return zlags_launch<8>(src, D, H, W, c0, c1, y_org, x_org, th, tw, gy, gx, sums, s);
  }
}
