// ssim_u8.hip -- tem_u8_ssim: the windowed structural similarity (SSIM) of two boxes of the same extents, one in each of
// two dense uint8 blocks, in integers up to two double divisions per window (include/tem_hip.h has the definition).
// Windows are uniform boxes of wz x win x win voxels (wz = win, or 1 for flat windows) that lie wholly inside the box.
//
// Tile and march.  A workgroup of 256 threads owns SSIM_TY x SSIM_TX = 8 x 32 window origins over (y, x) -- one window
// per thread -- and a run of at most SSIM_ZRUN = 32 window-sections along z, which it marches plane by plane:
//   1. stage: the (8 + win - 1) x (32 + win - 1) bytes of a and of b that the tile's windows cover in this plane go to
//      LDS as bytes, byte by byte (the two sides' rows have their own alignment; positions outside the box hold 0 and
//      feed only windows that are not counted).  No byte outside the boxes is read.
//   2. row sums along x: for every staged row and window column the five sums over win bytes, one uint4 in LDS:
//      {Sa | Sb << 16, Saa, Sbb, Sab} (a row's Sa, Sb <= 11 * 255 fit 16 bits each).
//   3. column sums along y: each thread adds the win row sums under its window into the plane's 2-D window sums P,
//      still packed (Sa, Sb <= 121 * 255 = 30,855 < 2^16; Saa <= 121 * 65025 < 2^23).
// The 3-D sums are S += P_new - P_old over the last wz planes' P in registers (4 words x wz <= 44 VGPRs), oldest
// first and moved down one place per plane, so every index is static -- 40 moves beside the few hundred operations of
// a plane, and the march needs no unrolling by wz.  A run pays wz - 1 warm-up planes.  Flat windows keep no planes.
// Every S fits 32 bits: Saa <= 1331 * 65025 < 2^27.  From S the thread forms A1, B1, A2, B2 in int64 (below 2^53 for
// win <= 11: the conversions to double are exact), l = A1 / B1, cs = A2 / B2, s = l cs and the three q = rint(x 2^30).
//
// Sums.  The q of one window-section are reduced inside each wave (shuffles), the four waves add their totals into the
// run's [32][3] 64-bit LDS accumulators, and the run ends with ONE 64-bit global atomic add per window-section and
// quantity.  Integer adds commute: the result does not depend on the launch geometry.  The map byte of a window is
// (255 max(q_s, 0) + 2^29) >> 30.
#include "tem_common.h"

namespace {

constexpr int SSIM_TY = 8, SSIM_TX = 32;       // window origins per workgroup plane, (y, x): one per thread
constexpr int SSIM_THREADS = SSIM_TY * SSIM_TX;
constexpr int SSIM_ZRUN = 32;                  // window-sections per workgroup run
constexpr int64_t SSIM_MAX_WGS = (1 << 24) - 1;   // x 256 threads stays below 2^32, the launch's limit

struct ssim_args {
  const uint8_t *a0, *b0;                      // the boxes' first bytes
  int64_t Ha, Wa, Hb, Wb;
  int nz, ny, nx;                              // the voxel box
  int nzw, nyw, nxw;                           // the window box
  int tiles_x, tiles;                          // tiles along x, tiles per window-section
  unsigned long long *sums;
  uint8_t *map;
};

__device__ __forceinline__ long long ssim_q(double x) { return __double2ll_rn(x * 1073741824.0); }

template <int WIN, bool FLAT>
__global__ __launch_bounds__(SSIM_THREADS) void u8_ssim_k(ssim_args g) {
  constexpr int WZ = FLAT ? 1 : WIN;
  constexpr int RH = SSIM_TY + WIN - 1, RW = SSIM_TX + WIN - 1;
  constexpr long long N = (long long)WZ * WIN * WIN;
  constexpr long long C1 = 65025ll * N * N, C2 = 585225ll * N * (N - 1);
  __shared__ uint8_t sa[RH * RW], sb[RH * RW];
  __shared__ uint4 rs[RH * SSIM_TX];
  __shared__ unsigned long long red[SSIM_ZRUN * 3];

  const int tid = threadIdx.x, tx = tid % SSIM_TX, ty = tid / SSIM_TX;
  const int run = blockIdx.x / g.tiles, tile = blockIdx.x - run * g.tiles;
  const int tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
  const int oy = tyi * SSIM_TY, ox = txi * SSIM_TX;                      // the tile's first window origin
  const int zw0 = run * SSIM_ZRUN, nzr = min(SSIM_ZRUN, g.nzw - zw0);    // this run: window-sections [zw0, zw0 + nzr)
  const int nplanes = nzr + WZ - 1;
  const bool counted = oy + ty < g.nyw && ox + tx < g.nxw;
  if (tid < SSIM_ZRUN * 3) red[tid] = 0;                                 // ordered by the first plane's barriers

  uint4 ring[WZ];
#pragma unroll
  for (int r = 0; r < WZ; ++r) ring[r] = make_uint4(0, 0, 0, 0);
  int Sa = 0, Sb = 0, Saa = 0, Sbb = 0, Sab = 0;

  for (int p = 0; p < nplanes; ++p) {
    // 1. stage plane zw0 + p of the box
    const uint8_t *pa = g.a0 + (int64_t)(zw0 + p) * g.Ha * g.Wa;
    const uint8_t *pb = g.b0 + (int64_t)(zw0 + p) * g.Hb * g.Wb;
    for (int i = tid; i < RH * RW; i += SSIM_THREADS) {
      const int rr = i / RW, cc = i - rr * RW;
      const int y = oy + rr, x = ox + cc;
      const bool in = y < g.ny && x < g.nx;
      sa[i] = in ? pa[(int64_t)y * g.Wa + x] : (uint8_t)0;
      sb[i] = in ? pb[(int64_t)y * g.Wb + x] : (uint8_t)0;
    }
    __syncthreads();
    // 2. row sums along x
    for (int i = tid; i < RH * SSIM_TX; i += SSIM_THREADS) {
      const int rr = i / SSIM_TX, cc = i - rr * SSIM_TX;
      const uint8_t *ra = sa + rr * RW + cc, *rb = sb + rr * RW + cc;
      uint32_t ab = 0, aa = 0, bb = 0, xy = 0;
#pragma unroll
      for (int j = 0; j < WIN; ++j) {
        const uint32_t u = ra[j], v = rb[j];
        ab += u | (v << 16);
        aa += u * u;
        bb += v * v;
        xy += u * v;
      }
      rs[i] = make_uint4(ab, aa, bb, xy);
    }
    __syncthreads();
    // 3. column sums along y: the plane's 2-D window sums
    uint4 P = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < WIN; ++j) {
      const uint4 v = rs[(ty + j) * SSIM_TX + tx];
      P.x += v.x, P.y += v.y, P.z += v.z, P.w += v.w;
    }
    if (FLAT) {
      Sa = (int)(P.x & 0xffffu), Sb = (int)(P.x >> 16), Saa = (int)P.y, Sbb = (int)P.z, Sab = (int)P.w;
    } else {
      const uint4 old = ring[0];
      Sa += (int)(P.x & 0xffffu) - (int)(old.x & 0xffffu);
      Sb += (int)(P.x >> 16) - (int)(old.x >> 16);
      Saa += (int)P.y - (int)old.y;
      Sbb += (int)P.z - (int)old.z;
      Sab += (int)P.w - (int)old.w;
#pragma unroll
      for (int r = 0; r + 1 < WZ; ++r) ring[r] = ring[r + 1];
      ring[WZ - 1] = P;
    }
    if (p >= WZ - 1) {                                                 // uniform: window-section zw0 + p - (WZ - 1)
      const int zr = p - (WZ - 1);
      long long qs = 0, ql = 0, qc = 0;
      if (counted) {
        const long long a = Sa, b = Sb;
        const long long A1 = 20000ll * a * b + C1, B1 = 10000ll * (a * a + b * b) + C1;
        const long long A2 = 20000ll * (N * Sab - a * b) + C2;
        const long long B2 = 10000ll * ((N * Saa - a * a) + (N * Sbb - b * b)) + C2;
        const double l = (double)A1 / (double)B1, cs = (double)A2 / (double)B2;
        qs = ssim_q(l * cs), ql = ssim_q(l), qc = ssim_q(cs);
        if (g.map) {
          const long long m = (255ll * (qs > 0 ? qs : 0ll) + (1ll << 29)) >> 30;
          g.map[((int64_t)(zw0 + zr) * g.nyw + (oy + ty)) * g.nxw + (ox + tx)] = (uint8_t)m;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        qs += __shfl_down(qs, d, 64);
        ql += __shfl_down(ql, d, 64);
        qc += __shfl_down(qc, d, 64);
      }
      if ((tid & 63) == 0) {
        atomicAdd(&red[zr * 3 + 0], (unsigned long long)qs);
        atomicAdd(&red[zr * 3 + 1], (unsigned long long)ql);
        atomicAdd(&red[zr * 3 + 2], (unsigned long long)qc);
      }
    }
  }
  __syncthreads();
  if (tid < nzr * 3) atomicAdd(g.sums + (int64_t)zw0 * 3 + tid, red[tid]);
}

template <int WIN> void ssim_launch(bool flat, unsigned wgs, hipStream_t stream, const ssim_args &g) {
  if (flat)
    hipLaunchKernelGGL((u8_ssim_k<WIN, true>), dim3(wgs), dim3(SSIM_THREADS), 0, stream, g);
  else
    hipLaunchKernelGGL((u8_ssim_k<WIN, false>), dim3(wgs), dim3(SSIM_THREADS), 0, stream, g);
}

}  // namespace

extern "C" int tem_u8_ssim(const uint8_t *a, int32_t Da, int32_t Ha, int32_t Wa, int32_t az0, int32_t ay0, int32_t ax0,
                           const uint8_t *b, int32_t Db, int32_t Hb, int32_t Wb, int32_t bz0, int32_t by0, int32_t bx0,
                           int32_t nz, int32_t ny, int32_t nx, int32_t win, int32_t flat, int64_t *sums, uint8_t *map,
                           tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!a || !b || !sums || ((uintptr_t)sums & 7) || Da < 1 || Ha < 1 || Wa < 1 || Db < 1 || Hb < 1 || Wb < 1 ||
      az0 < 0 || ay0 < 0 || ax0 < 0 || bz0 < 0 || by0 < 0 || bx0 < 0 || nz < 0 || ny < 0 || nx < 0)
    return TEM_EINVAL;
  if (win < 3 || win > 11 || !(win & 1)) return TEM_EINVAL;
  if ((int64_t)az0 + nz > Da || (int64_t)ay0 + ny > Ha || (int64_t)ax0 + nx > Wa || (int64_t)bz0 + nz > Db ||
      (int64_t)by0 + ny > Hb || (int64_t)bx0 + nx > Wb)
    return TEM_EINVAL;
  const int wz = flat ? 1 : win;
  if (nz < wz || ny < win || nx < win) return TEM_OK;                    // no window fits
  ssim_args g;
  g.a0 = a + ((int64_t)az0 * Ha + ay0) * Wa + ax0;
  g.b0 = b + ((int64_t)bz0 * Hb + by0) * Wb + bx0;
  g.Ha = Ha, g.Wa = Wa, g.Hb = Hb, g.Wb = Wb;
  g.nz = nz, g.ny = ny, g.nx = nx;
  g.nzw = nz - wz + 1, g.nyw = ny - win + 1, g.nxw = nx - win + 1;
  const int64_t tiles_x = (g.nxw + SSIM_TX - 1) / SSIM_TX, tiles_y = (g.nyw + SSIM_TY - 1) / SSIM_TY;
  const int64_t runs = (g.nzw + SSIM_ZRUN - 1) / SSIM_ZRUN;
  if (tiles_x * tiles_y > SSIM_MAX_WGS || tiles_x * tiles_y * runs > SSIM_MAX_WGS) return TEM_EINVAL;
  g.tiles_x = (int)tiles_x, g.tiles = (int)(tiles_x * tiles_y);
  g.sums = reinterpret_cast<unsigned long long *>(sums);
  g.map = map;
  const unsigned wgs = (unsigned)(g.tiles * runs);
  switch (win) {
    case 3: ssim_launch<3>(flat != 0, wgs, (hipStream_t)stream, g); break;
    case 5: ssim_launch<5>(flat != 0, wgs, (hipStream_t)stream, g); break;
    case 7: ssim_launch<7>(flat != 0, wgs, (hipStream_t)stream, g); break;
    case 9: ssim_launch<9>(flat != 0, wgs, (hipStream_t)stream, g); break;
    default: ssim_launch<11>(flat != 0, wgs, (hipStream_t)stream, g); break;
  }
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
