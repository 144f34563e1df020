// rescale_u8.hip -- tem_u8_rescale: a dense uint8 block of a volume resampled onto a grid of another voxel size, one step
// p/q per axis, in integers with ONE rounding per voxel (include/tem_hip.h has the definition): the area average where
// an axis shrinks (p >= q), linear between voxel centres where it grows (p < q).  Taps and the clipping at the far faces
// are computed in volume coordinates, so a block's bytes do not depend on how the volume was cut.
//
// Tile and march.  A workgroup of 256 threads owns RESCALE_TY x RESCALE_TX = 8 x 32 outputs over (y, x) -- one per
// thread -- and a run of at most RESCALE_ZRUN = 32 output planes, and marches the source planes under that run once:
//   1. stage: the tile's source footprint in this plane -- the hull of its y taps by the hull of its x taps, at most
//      66 x 258 bytes at step 8 -- goes to LDS as bytes, a wave per row (rows and pointers have any alignment).  Every
//      position of the footprint is a tap of some output of the tile: no byte outside the taps' hull is read.
//   2. x pass: for every staged row and output column the weighted sum over the column's taps, 16 bits in LDS (at most
//      255 * 128).  A thread's column is its own in every row it takes (256 = 8 rows of 32), so its x weights stay in
//      registers; so do its y weights.
//   3. y pass: each thread adds its rows' sums under its y weights: P, the plane resampled in (y, x), one int32 per
//      thread (at most 255 * 128^2).
// Along z an area axis adds wz P into the at most two output planes a source plane overlaps (q <= p) and emits a plane
// when its last tap has passed; a linear axis keeps the previous and the current P and emits every output plane between
// them.  Both are uniform scalar bookkeeping by additions: the only integer divisions are the ones that find a
// workgroup's first taps, up front.  S <= 255 * 128^3, and 2 S + Den < 2^31.
//
// The planes a run reads are consecutive.  Where the footprint is at most RESCALE_PREFETCH = 8 bytes per thread (steps up
// to about 3) it travels through registers and plane s + 1 is loaded while plane s is resampled, which about halves the
// time at step 2 (131 -> 72 us for 64 x 1024^2 -> 32 x 512^2 on one MI355X); a larger footprint is staged directly.
//
// The tap loops are unrolled over NT in {2, 3, 5, 9} taps, the smallest that holds the y and x axes' widest output;
// weights past an output's taps are 0 and multiply bytes of LDS that no output needs (the arrays carry that slack).
//
// The voxel is (2 S + Den) / (2 Den) with Den = Wz Wy Wx.  W is the axis' full denominator (p, or 2 q) except at the
// last output of a shrinking axis whose extent the step does not divide: eight divisors d = 2 Den per launch.  For each
// the host passes m = ceil(2^64 / d); with n = 2 S + Den < 2^31 and d <= 2^22, floor(n m / 2^64) = floor(n / d) exactly
// (the error term n (m d - 2^64) / (d 2^64) stays below 1 / d since n (m d - 2^64) < 2^31 2^22).
#include <algorithm>

#include "tem_common.h"

namespace {

constexpr int RESCALE_TY = 8, RESCALE_TX = 32;         // outputs per workgroup plane, (y, x): one per thread
constexpr int RESCALE_THREADS = RESCALE_TY * RESCALE_TX;
constexpr int RESCALE_ZRUN = 32;                       // output planes per workgroup run
constexpr int RESCALE_MAX_STEP = 8, RESCALE_MAX_PQ = 64;
constexpr int RESCALE_FY = RESCALE_MAX_STEP * RESCALE_TY + 2, RESCALE_FX = RESCALE_MAX_STEP * RESCALE_TX + 2;   // footprint
constexpr int RESCALE_MAX_TAPS = RESCALE_MAX_STEP + 1;
constexpr int RESCALE_PREFETCH = 8;                    // bytes of the next plane a thread holds in registers
constexpr int64_t RESCALE_MAX_WGS = (1 << 24) - 1;     // x 256 threads stays below 2^32, the launch's limit

struct rescale_args {
  const uint8_t *src;
  int64_t H, W;                                        // the source block's plane
  int sz0, sy0, sx0, VZ, VY, VX;
  int pz, qz, py, qy, px, qx;
  uint8_t *dst;
  int OD, OH, OW, oz0, oy0, ox0;
  int tiles_x, tiles;                                  // tiles along x, tiles per run
  int wfz, wfy, wfx, wlz;                              // the full denominator per axis; z's at the far face
  unsigned long long magic[8];                         // ceil(2^64 / (2 Den)), [z last][y last][x last]
};

__host__ __device__ inline int64_t rs_min(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t rs_max(int64_t a, int64_t b) { return a > b ? a : b; }
// a / b for a >= 0, b >= 1: in 32 bits where a allows it
__host__ __device__ inline int64_t rs_div(int64_t a, int b) {
  return (a >> 31) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// Output j of an axis of n source voxels at step p / q: its first tap, the weights of the NT voxels from there (0 past
// its taps), the denominator and the last tap of positive weight.  A tap of weight 0 is no tap: it is never read.
template <int NT>
__host__ __device__ inline void rescale_taps(int j, int p, int q, int n, int &first, int (&w)[NT], int &den, int &last) {
  if (p >= q) {
    const int64_t lo = (int64_t)j * p, hi = rs_min(lo + p, (int64_t)n * q);
    first = (int)rs_div(lo, q), last = (int)rs_div(hi - 1, q), den = (int)(hi - lo);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int64_t i = (int64_t)first + t;
      w[t] = (int)rs_max(rs_min((i + 1) * q, hi) - rs_max(i * q, lo), 0);
    }
  } else {
    const int64_t C = (2 * (int64_t)j + 1) * p - q;                      // > -q
    const int64_t i0 = C < 0 ? -1 : rs_div(C, 2 * q);
    const int f = (int)(C - 2 * q * i0);
    const int a = (int)rs_min(rs_max(i0, 0), n - 1), b = (int)rs_min(rs_max(i0 + 1, 0), n - 1);
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t] = 0;
    first = a, den = 2 * q;
    w[0] = a == b ? 2 * q : 2 * q - f;
    if (NT > 1) w[1 % NT] = a == b ? 0 : f;
    last = a != b && f > 0 ? b : a;
  }
}

template <int NT>
__global__ __launch_bounds__(RESCALE_THREADS) void u8_rescale_k(rescale_args g) {
  __shared__ uint8_t sa[RESCALE_FY * RESCALE_FX + 16];                   // the staged footprint, rows of fxn bytes
  __shared__ uint16_t xs[(RESCALE_FY + RESCALE_MAX_TAPS) * RESCALE_TX];  // its rows after the x pass

  const int tid = threadIdx.x, tx = tid % RESCALE_TX, ty = tid / RESCALE_TX;
  const int run = blockIdx.x / g.tiles, tile = blockIdx.x - run * g.tiles;
  const int tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
  const int by0 = tyi * RESCALE_TY, bx0 = txi * RESCALE_TX;              // the tile's first output in the block
  const int nyv = min(RESCALE_TY, g.OH - by0), nxv = min(RESCALE_TX, g.OW - bx0);
  const int zb0 = run * RESCALE_ZRUN, nzr = min(RESCALE_ZRUN, g.OD - zb0);

  // the tile's footprint (uniform), then this thread's taps inside it
  int fy0, fx0, fyn, fxn;
  {
    int w[NT], den, first, last;
    rescale_taps<NT>(g.oy0 + by0, g.py, g.qy, g.VY, fy0, w, den, last);
    rescale_taps<NT>(g.oy0 + by0 + nyv - 1, g.py, g.qy, g.VY, first, w, den, last);
    fyn = last - fy0 + 1;
    rescale_taps<NT>(g.ox0 + bx0, g.px, g.qx, g.VX, fx0, w, den, last);
    rescale_taps<NT>(g.ox0 + bx0 + nxv - 1, g.px, g.qx, g.VX, first, w, den, last);
    fxn = last - fx0 + 1;
  }
  int wy[NT], wx[NT], yf = 0, xf = 0, Wy = g.wfy, Wx = g.wfx;
#pragma unroll
  for (int t = 0; t < NT; ++t) wy[t] = wx[t] = 0;
  const bool live = ty < nyv && tx < nxv;
  if (ty < nyv) {
    int first, last;
    rescale_taps<NT>(g.oy0 + by0 + ty, g.py, g.qy, g.VY, first, wy, Wy, last);
    yf = first - fy0;
  }
  if (tx < nxv) {
    int first, last;
    rescale_taps<NT>(g.ox0 + bx0 + tx, g.px, g.qx, g.VX, first, wx, Wx, last);
    xf = first - fx0;
  }
  const int mi = (Wy != g.wfy ? 2 : 0) + (Wx != g.wfx ? 1 : 0);
  const unsigned long long m0 = g.magic[mi], m1 = g.magic[4 + mi];
  const unsigned den0 = (unsigned)(g.wfz * Wy * Wx), den1 = (unsigned)(g.wlz * Wy * Wx);
  const uint8_t *foot = g.src + ((int64_t)(fy0 - g.sy0)) * g.W + (fx0 - g.sx0);   // the footprint in block plane 0
  uint8_t *out = g.dst + ((int64_t)zb0 * g.OH + (by0 + ty)) * g.OW + (bx0 + tx);
  const int64_t oplane = (int64_t)g.OH * g.OW;

  // The planes a run reads are consecutive, up to the last tap of its last output.  A footprint of at most
  // RESCALE_PREFETCH bytes per thread travels through registers, so that plane s + 1 is in flight while plane s is
  // resampled; a larger one (steps past about 3) is staged directly.
  const int j0 = g.oz0 + zb0;                                            // the run's first output plane in the grid
  int s_last;
  {
    int w[NT], den, first;
    rescale_taps<NT>(j0 + nzr - 1, g.pz, g.qz, g.VZ, first, w, den, s_last);
  }
  const int fn = fyn * fxn;
  const bool small = fn <= RESCALE_PREFETCH * RESCALE_THREADS;
  int64_t goff[RESCALE_PREFETCH];                                        // this thread's bytes of the footprint
  uint8_t held[RESCALE_PREFETCH];
  int held_s = -1;                                                       // the plane `held` holds (uniform)
  if (small) {
#pragma unroll
    for (int k = 0; k < RESCALE_PREFETCH; ++k) {
      const int i = min(tid + k * RESCALE_THREADS, fn - 1), r = i / fxn;
      goff[k] = (int64_t)r * g.W + (i - r * fxn);
    }
  }
  auto fetch = [&](int s) {
    const uint8_t *pl = foot + (int64_t)(s - g.sz0) * g.H * g.W;
#pragma unroll
    for (int k = 0; k < RESCALE_PREFETCH; ++k)
      if (tid + k * RESCALE_THREADS < fn) held[k] = pl[goff[k]];
    held_s = s;
  };

  // source plane s (volume coordinates) resampled in (y, x): this thread's P
  auto plane = [&](int s) -> int {
    if (small) {
      if (held_s != s) fetch(s);
#pragma unroll
      for (int k = 0; k < RESCALE_PREFETCH; ++k)
        if (tid + k * RESCALE_THREADS < fn) sa[tid + k * RESCALE_THREADS] = held[k];
      if (s < s_last) fetch(s + 1);
    } else {
      const uint8_t *pl = foot + (int64_t)(s - g.sz0) * g.H * g.W;
      for (int r = tid >> 6; r < fyn; r += RESCALE_THREADS / 64)
        for (int c = tid & 63; c < fxn; c += 64) sa[r * fxn + c] = pl[(int64_t)r * g.W + c];
    }
    __syncthreads();
    for (int r = ty; r < fyn; r += RESCALE_TY) {
      const uint8_t *row = sa + r * fxn + xf;
      int a = 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) a += wx[t] * (int)row[t];
      xs[r * RESCALE_TX + tx] = (uint16_t)a;
    }
    __syncthreads();
    int P = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) P += wy[t] * (int)xs[(yf + t) * RESCALE_TX + tx];
    return P;
  };
  auto emit = [&](int zr, int S, bool zlast) {                           // output plane zb0 + zr of the block
    if (!live) return;
    const unsigned den = zlast ? den1 : den0;
    const unsigned long long m = zlast ? m1 : m0;
    out[zr * oplane] = (uint8_t)__umul64hi((unsigned long long)(2u * (unsigned)S + den), m);
  };

  if (g.pz >= g.qz) {
    const int64_t vend = (int64_t)g.VZ * g.qz;
    int64_t c_lo = (int64_t)j0 * g.pz;                                   // the open output, in 1 / qz source voxels
    int s = (int)rs_div(c_lo, g.qz);
    int64_t s_lo = (int64_t)s * g.qz;
    int acc0 = 0, acc1 = 0;
    for (int zr = 0; zr < nzr; ++s, s_lo += g.qz) {
      const int P = plane(s);
      const int64_t s_hi = s_lo + g.qz, c_hi = c_lo + g.pz;
      acc0 += (int)(rs_min(s_hi, c_hi) - rs_max(s_lo, c_lo)) * P;
      if (s_hi > c_hi) acc1 += (int)(s_hi - c_hi) * P;
      if (s_hi >= c_hi || s == g.VZ - 1) {                               // the open output's last tap
        emit(zr, acc0, rs_min(c_hi, vend) - c_lo != g.wfz);
        acc0 = acc1, acc1 = 0, c_lo = c_hi, ++zr;
        if (s == g.VZ - 1 && zr < nzr) emit(zr++, acc0, true);          // the grid's last output lies wholly in this plane
      }
    }
  } else {
    const int q2 = 2 * g.qz;
    const int64_t C = (2 * (int64_t)j0 + 1) * g.pz - g.qz;
    int i0 = C < 0 ? -1 : (int)rs_div(C, q2);
    int f = (int)(C - (int64_t)q2 * i0);
    int ip = -1, ic = -1, prev = 0, cur = 0;                             // the planes held: prev is ip, cur is ic
    for (int zr = 0; zr < nzr; ++zr) {
      const int a = min(max(i0, 0), g.VZ - 1);
      int b = min(max(i0 + 1, 0), g.VZ - 1);
      const int wb = a == b ? 0 : f;
      if (wb == 0) b = a;
      if (a != ip && a != ic) {
        prev = plane(a), ip = a;
      } else if (a == ic && ip != ic) {
        prev = cur, ip = ic;
      }
      if (b != ip && b != ic) cur = plane(b), ic = b;
      emit(zr, (q2 - wb) * prev + wb * (b == ip ? prev : cur), false);
      f += 2 * g.pz;
      if (f >= q2) f -= q2, ++i0;
    }
  }
}

int64_t grid_extent(int64_t n, int p, int q) { return (n * q + p - 1) / p; }

int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

bool step_ok(int p, int q) {
  return p >= 1 && q >= 1 && p <= RESCALE_MAX_PQ && q <= RESCALE_MAX_PQ && p <= RESCALE_MAX_STEP * q &&
         q <= RESCALE_MAX_STEP * p && gcd(p, q) == 1;
}

// the hull of the taps of outputs [o0, o0 + on) lies inside the source block [s0, s0 + sn)
bool hull_inside(int o0, int on, int p, int q, int n, int s0, int sn) {
  int w[1], den, lo, hi, first, last;
  rescale_taps<1>(o0, p, q, n, lo, w, den, last);
  rescale_taps<1>(o0 + on - 1, p, q, n, first, w, den, hi);
  return lo >= s0 && (int64_t)hi < (int64_t)s0 + sn;
}

// the widest output of an axis away from the far face, in taps
int max_taps(int p, int q) {
  if (p < q) return 2;
  int most = 1;
  for (int j = 0; j < q; ++j) most = std::max(most, ((j + 1) * p - 1) / q - j * p / q + 1);
  return most;
}

// the denominator of the axis' last output
int last_den(int n, int p, int q) {
  if (p < q) return 2 * q;
  const int64_t j = grid_extent(n, p, q) - 1;
  return (int)(rs_min((j + 1) * p, (int64_t)n * q) - j * p);
}

}  // namespace

extern "C" int tem_u8_rescale(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t sy0, int32_t sx0,
                              int32_t VZ, int32_t VY, int32_t VX, int32_t pz, int32_t qz, int32_t py, int32_t qy,
                              int32_t px, int32_t qx, uint8_t *dst, int32_t OD, int32_t OH, int32_t OW, int32_t oz0,
                              int32_t oy0, int32_t ox0, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || D < 1 || H < 1 || W < 1 || VZ < 1 || VY < 1 || VX < 1 || OD < 1 || OH < 1 || OW < 1 || sz0 < 0 ||
      sy0 < 0 || sx0 < 0 || oz0 < 0 || oy0 < 0 || ox0 < 0)
    return TEM_EINVAL;
  if (!step_ok(pz, qz) || !step_ok(py, qy) || !step_ok(px, qx)) return TEM_EINVAL;
  if ((int64_t)sz0 + D > VZ || (int64_t)sy0 + H > VY || (int64_t)sx0 + W > VX) return TEM_EINVAL;
  if ((int64_t)oz0 + OD > grid_extent(VZ, pz, qz) || (int64_t)oy0 + OH > grid_extent(VY, py, qy) ||
      (int64_t)ox0 + OW > grid_extent(VX, px, qx))
    return TEM_EINVAL;
  if (!hull_inside(oz0, OD, pz, qz, VZ, sz0, D) || !hull_inside(oy0, OH, py, qy, VY, sy0, H) ||
      !hull_inside(ox0, OW, px, qx, VX, sx0, W))
    return TEM_EINVAL;
  const int64_t tiles_x = ((int64_t)OW + RESCALE_TX - 1) / RESCALE_TX, tiles_y = ((int64_t)OH + RESCALE_TY - 1) / RESCALE_TY;
  const int64_t runs = ((int64_t)OD + RESCALE_ZRUN - 1) / RESCALE_ZRUN;
  if (tiles_x * tiles_y > RESCALE_MAX_WGS || tiles_x * tiles_y * runs > RESCALE_MAX_WGS) return TEM_EINVAL;
  rescale_args g;
  g.src = src, g.H = H, g.W = W;
  g.sz0 = sz0, g.sy0 = sy0, g.sx0 = sx0, g.VZ = VZ, g.VY = VY, g.VX = VX;
  g.pz = pz, g.qz = qz, g.py = py, g.qy = qy, g.px = px, g.qx = qx;
  g.dst = dst, g.OD = OD, g.OH = OH, g.OW = OW, g.oz0 = oz0, g.oy0 = oy0, g.ox0 = ox0;
  g.tiles_x = (int)tiles_x, g.tiles = (int)(tiles_x * tiles_y);
  g.wfz = pz >= qz ? pz : 2 * qz, g.wfy = py >= qy ? py : 2 * qy, g.wfx = px >= qx ? px : 2 * qx;
  g.wlz = last_den(VZ, pz, qz);
  const int wly = last_den(VY, py, qy), wlx = last_den(VX, px, qx);
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = 2ull * (i & 4 ? g.wlz : g.wfz) * (i & 2 ? wly : g.wfy) * (i & 1 ? wlx : g.wfx);   // 2 <= d <= 2^22
    g.magic[i] = ~0ull / d + 1;
  }
  const unsigned wgs = (unsigned)(g.tiles * runs);
  const int nt = std::max(max_taps(py, qy), max_taps(px, qx));
  if (nt <= 2)
    hipLaunchKernelGGL(u8_rescale_k<2>, dim3(wgs), dim3(RESCALE_THREADS), 0, (hipStream_t)stream, g);
  else if (nt <= 3)
    hipLaunchKernelGGL(u8_rescale_k<3>, dim3(wgs), dim3(RESCALE_THREADS), 0, (hipStream_t)stream, g);
  else if (nt <= 5)
    hipLaunchKernelGGL(u8_rescale_k<5>, dim3(wgs), dim3(RESCALE_THREADS), 0, (hipStream_t)stream, g);
  else
    hipLaunchKernelGGL(u8_rescale_k<RESCALE_MAX_TAPS>, dim3(wgs), dim3(RESCALE_THREADS), 0, (hipStream_t)stream, g);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
