// tiles_sym.hip -- tiled inference under a symmetry of the cube (square): the gather hands the generator T(tile), the
// accumulate folds the generator's output back with the inverse of T into an fp32 mean -- and, in its `_spread` form, into
// the moments of the members' spread (tile_math.h) at the same voxel, in the same launch.
//   T(v) = flip(transpose(v, perm), axes a with flips[a])            (tem_augment_f32's convention)
//   T(v)[q] = v[j(q)],   j[perm[a]] = flips[a] ? n - 1 - q[a] : q[a]
// A tile has extents (D, E, E): D == E (3-D) or D == 1 (2-D: perm[0] == 0, flips[0] == 0, so j[0] == q[0] == 0).
//
// Two kernels per direction.  perm[2] == 2: a row of q is a row of j (possibly reversed), so one wave walks one row and
// both sides run along x.  perm[2] != 2: x of j is fed by q axis a* != 2; a plain loop would touch one side with a
// stride of E or E^2 elements.  These go through a 64 x 64 LDS tile over the plane (q[a*], q[2]): it is filled with
// the lanes along the reading side's x and drained with the lanes along the writing side's x.  Rows of the LDS tile
// are padded to 65 dwords: the drain reads a column, lane l at dword 65 l + c, i.e. bank (l + c) % 32 -- 32 distinct
// banks per 32-lane group, as the row-wise fill has.  Ragged remainders (E % 64) are predicated, never read or written.
#include "tem_common.h"
#include "tile_math.h"

namespace {

// j[c] = g[c] ? n_c - 1 - q[ip[c]] : q[ip[c]]: ip = the inverse of perm, g[c] = flips[ip[c]]
struct SymDev { int ip0, ip1, ip2, g0, g1, g2; };

// the staging block, its origin in the volume, the volume's extents (tem_u8_tiles_to_f32_std_bc)
struct TileSrc { const uint8_t *blk; int BZ, BY, BX, lz, ly, lx, Z, Y, X; };

// select chain, not an indexed array: a runtime-indexed register array would be placed in scratch memory
__device__ __forceinline__ int pick(int a, int q0, int q1, int q2) { return a == 0 ? q0 : (a == 1 ? q1 : q2); }

// coordinate along one axis of the block that volume coordinate v reads (mode 0: v itself; else folded)
template <int MODE>
__device__ __forceinline__ int src_coord(int v, int n, int l) {
  if constexpr (MODE == 0) return v - l;
  else return bc_fold<MODE>(v, n) - l;
}

__device__ __forceinline__ float accum_op(float acc, float y, int first, int divisor) {
  float v = first ? y : __fadd_rn(acc, y);
  if (divisor > 1) v = __fdiv_rn(v, (float)divisor);
  return v;
}

// What the accumulate kernels do with value y of a member at the folded-back element i: the mean alone, or the mean
// and the spread's moments about the first member (`first` writes ref = y, s1 = s2 = 0 without reading them).
struct MeanOp {
  float *acc; int first, divisor;
  __device__ __forceinline__ void operator()(int64_t i, float y) const {
    acc[i] = accum_op(first ? 0.f : acc[i], y, first, divisor);
  }
};

struct SpreadOp {
  MeanOp mean; float *ref, *s1, *s2;
  __device__ __forceinline__ void operator()(int64_t i, float y) const {
    float r = y, a = 0.f, b = 0.f;
    if (!mean.first) { r = ref[i]; a = s1[i]; b = s2[i]; }           // every load ahead of the first store
    mean(i, y);
    if (mean.first) ref[i] = y;
    else spread_update(y, r, a, b);
    s1[i] = a; s2[i] = b;
  }
};

// ---------------------------------------------------------------- perm keeps x innermost: one wave per row
template <int MODE>
__global__ __launch_bounds__(256) void u8_tiles_sym_row_k(TileSrc s, const int32_t *origins, int D, int E, SymDev m,
                                                          float *out, float mean, float std, int64_t rows) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int rpt = D * E;                                               // rows per tile
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const int t = (int)(r / rpt), rr = (int)(r - (int64_t)t * rpt);
    const int q0 = rr / E, q1 = rr - q0 * E;
    int j0 = pick(m.ip0, q0, q1, 0), j1 = pick(m.ip1, q0, q1, 0);
    j0 = m.g0 ? D - 1 - j0 : j0;
    j1 = m.g1 ? E - 1 - j1 : j1;
    const int vx = s.lx + origins[3 * t + 2];
    const int bz = src_coord<MODE>(s.lz + origins[3 * t] + j0, s.Z, s.lz);          // z and y: once per row
    const int by = src_coord<MODE>(s.ly + origins[3 * t + 1] + j1, s.Y, s.ly);
    const bool rin = (unsigned)bz < (unsigned)s.BZ && (unsigned)by < (unsigned)s.BY;
    const uint8_t *row = s.blk + (rin ? ((int64_t)bz * s.BY + by) * s.BX : 0);
    float *orow = out + r * E;
    for (int x = lane; x < E; x += 64) {
      const int bx = src_coord<MODE>(vx + (m.g2 ? E - 1 - x : x), s.X, s.lx);
      const bool in = rin && (unsigned)bx < (unsigned)s.BX;
      orow[x] = u8_std(in ? (float)row[bx] : 0.f, mean, std);
    }
  }
}

template <class Op>
__global__ __launch_bounds__(256) void f32_tiles_sym_accum_row_k(const float *y, int D, int E, SymDev m, Op op,
                                                                 int64_t rows) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int rpt = D * E;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const int64_t t = r / rpt; const int rr = (int)(r - t * rpt);
    const int q0 = rr / E, q1 = rr - q0 * E;
    int j0 = pick(m.ip0, q0, q1, 0), j1 = pick(m.ip1, q0, q1, 0);
    j0 = m.g0 ? D - 1 - j0 : j0;
    j1 = m.g1 ? E - 1 - j1 : j1;
    const float *src = y + r * E;
    const int64_t dst = (t * rpt + (int64_t)j0 * E + j1) * E;
    for (int x = lane; x < E; x += 64) op(dst + (m.g2 ? E - 1 - x : x), src[x]);
  }
}

// ---------------------------------------------------------------- perm moves x: 64 x 64 planes through LDS
// workgroup = (tile t, q[b] = w, 64 x 64 window (tu, tv) of the plane (u = q[a*], v = q[2])); a* = ip2, b = 1 - a*
struct TrBlock { int t, w, u0, v0, U; };

__device__ __forceinline__ TrBlock tr_block(int D, int E, const SymDev &m, int nu, int nv) {
  unsigned b = blockIdx.x;
  TrBlock k;
  k.v0 = (int)(b % (unsigned)nv) * 64; b /= (unsigned)nv;
  k.u0 = (int)(b % (unsigned)nu) * 64; b /= (unsigned)nu;
  const unsigned W = m.ip2 == 0 ? E : D;
  k.w = (int)(b % W); k.t = (int)(b / W);
  k.U = m.ip2 == 0 ? D : E;
  return k;
}

// j(q) for q[a*] = u, q[b] = w, q[2] = v
__device__ __forceinline__ void tr_j(const SymDev &m, int D, int E, int u, int w, int v, int &q0, int &q1, int &j0,
                                     int &j1, int &j2) {
  q0 = m.ip2 == 0 ? u : w; q1 = m.ip2 == 0 ? w : u;
  j0 = pick(m.ip0, q0, q1, v); j1 = pick(m.ip1, q0, q1, v); j2 = u;
  j0 = m.g0 ? D - 1 - j0 : j0;
  j1 = m.g1 ? E - 1 - j1 : j1;
  j2 = m.g2 ? E - 1 - j2 : j2;
}

template <int MODE>
__global__ __launch_bounds__(256) void u8_tiles_sym_tr_k(TileSrc s, const int32_t *origins, int D, int E, SymDev m,
                                                         float *out, float mean, float std, int nu, int nv) {
  __shared__ float lds[64][65];
  const TrBlock k = tr_block(D, E, m, nu, nv);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int vz = s.lz + origins[3 * k.t], vy = s.ly + origins[3 * k.t + 1], vx = s.lx + origins[3 * k.t + 2];
  {                                                                    // fill: lanes along u = x of the volume
    const int u = k.u0 + lane;
    for (int i = wave; i < 64; i += 4) {
      const int v = k.v0 + i;
      float val = 0.f;
      if (u < k.U && v < E) {
        int q0, q1, j0, j1, j2;
        tr_j(m, D, E, u, k.w, v, q0, q1, j0, j1, j2);
        const int bz = src_coord<MODE>(vz + j0, s.Z, s.lz), by = src_coord<MODE>(vy + j1, s.Y, s.ly),
                  bx = src_coord<MODE>(vx + j2, s.X, s.lx);
        const bool in = (unsigned)bz < (unsigned)s.BZ && (unsigned)by < (unsigned)s.BY && (unsigned)bx < (unsigned)s.BX;
        val = u8_std(in ? (float)s.blk[((int64_t)bz * s.BY + by) * s.BX + bx] : 0.f, mean, std);
      }
      lds[i][lane] = val;
    }
  }
  __syncthreads();
  {                                                                    // drain: lanes along v = x of the tile
    const int v = k.v0 + lane;
    float *o = out + (int64_t)k.t * D * E * E;
    for (int i = wave; i < 64; i += 4) {
      const int u = k.u0 + i;
      if (u < k.U && v < E) {
        const int q0 = m.ip2 == 0 ? u : k.w, q1 = m.ip2 == 0 ? k.w : u;
        o[((int64_t)q0 * E + q1) * E + v] = lds[lane][i];
      }
    }
  }
}

template <class Op>
__global__ __launch_bounds__(256) void f32_tiles_sym_accum_tr_k(const float *y, int D, int E, SymDev m, Op op, int nu,
                                                                int nv) {
  __shared__ float lds[64][65];
  const TrBlock k = tr_block(D, E, m, nu, nv);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t base = (int64_t)k.t * D * E * E;
  {                                                                    // fill: lanes along v = x of y
    const int v = k.v0 + lane;
    for (int i = wave; i < 64; i += 4) {
      const int u = k.u0 + i;
      float val = 0.f;
      if (u < k.U && v < E) {
        const int q0 = m.ip2 == 0 ? u : k.w, q1 = m.ip2 == 0 ? k.w : u;
        val = y[base + ((int64_t)q0 * E + q1) * E + v];
      }
      lds[i][lane] = val;
    }
  }
  __syncthreads();
  {                                                                    // drain: lanes along u = x of the destinations
    const int u = k.u0 + lane;
    for (int i = wave; i < 64; i += 4) {
      const int v = k.v0 + i;
      if (u < k.U && v < E) {
        int q0, q1, j0, j1, j2;
        tr_j(m, D, E, u, k.w, v, q0, q1, j0, j1, j2);
        op(base + ((int64_t)j0 * E + j1) * E + j2, lds[lane][i]);
      }
    }
  }
}

// ---------------------------------------------------------------- host side
// perm is a permutation of (0, 1, 2), the flags are 0 or 1, a 2-D symmetry leaves z alone
bool sym_ok(int32_t p0, int32_t p1, int32_t p2, int32_t f0, int32_t f1, int32_t f2, bool is3d, SymDev &m) {
  const int32_t p[3] = {p0, p1, p2}, f[3] = {f0, f1, f2};
  int ip[3] = {-1, -1, -1};
  for (int a = 0; a < 3; ++a) {
    if (p[a] < 0 || p[a] > 2 || ip[p[a]] >= 0 || (f[a] != 0 && f[a] != 1)) return false;
    ip[p[a]] = a;
  }
  if (!is3d && (p0 != 0 || f0 != 0)) return false;
  m = SymDev{ip[0], ip[1], ip[2], f[ip[0]], f[ip[1]], f[ip[2]]};
  return true;
}

// the block lies inside a non-empty volume; mode 0 (zeros), reflect or edge
bool src_ok(const TileSrc &s, int32_t mode) {
  if (mode != 0 && mode != TEM_BOUNDARY_REFLECT && mode != TEM_BOUNDARY_EDGE) return false;
  if (!s.blk || s.Z < 1 || s.Y < 1 || s.X < 1 || s.BZ < 1 || s.BY < 1 || s.BX < 1 || s.lz < 0 || s.ly < 0 || s.lx < 0)
    return false;
  return s.BZ <= s.Z - s.lz && s.BY <= s.Y - s.ly && s.BX <= s.X - s.lx;
}

unsigned row_grid(int64_t rows) {
  const int64_t b = (rows + 3) / 4;
  return (unsigned)(b > 65536 ? 65536 : b);
}

// workgroups of the transposing kernels, 0 when they exceed a grid
int64_t tr_grid(int32_t ntile, int D, int E, const SymDev &m, int &nu, int &nv) {
  const int U = m.ip2 == 0 ? D : E, W = m.ip2 == 0 ? E : D;
  nu = (U + 63) / 64; nv = (E + 63) / 64;
  const int64_t n = (int64_t)ntile * W * nu * nv;
  return n > 0x7fffffff ? 0 : n;
}

int gather_sym(const TileSrc &s, int32_t mode, const int32_t *origins, int32_t ntile, int32_t edge, bool is3d, int32_t p0,
               int32_t p1, int32_t p2, int32_t f0, int32_t f1, int32_t f2, float *out, float mean, float std,
               hipStream_t st) {
  SymDev m;
  if (!origins || !out || !src_ok(s, mode) || ntile < 0 || edge < 1 || edge > 46340 ||
      !sym_ok(p0, p1, p2, f0, f1, f2, is3d, m))
    return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  const int D = is3d ? edge : 1;
  if (m.ip2 == 2) {
    const int64_t rows = (int64_t)ntile * D * edge;
    const dim3 g(row_grid(rows));
    if (mode == 0)
      hipLaunchKernelGGL(u8_tiles_sym_row_k<0>, g, dim3(256), 0, st, s, origins, D, edge, m, out, mean, std, rows);
    else if (mode == TEM_BOUNDARY_REFLECT)
      hipLaunchKernelGGL(u8_tiles_sym_row_k<TEM_BOUNDARY_REFLECT>, g, dim3(256), 0, st, s, origins, D, edge, m, out, mean,
                         std, rows);
    else
      hipLaunchKernelGGL(u8_tiles_sym_row_k<TEM_BOUNDARY_EDGE>, g, dim3(256), 0, st, s, origins, D, edge, m, out, mean,
                         std, rows);
  } else {
    int nu, nv;
    const int64_t nblk = tr_grid(ntile, D, edge, m, nu, nv);
    if (!nblk) return TEM_EUNSUPPORTED;
    const dim3 g((unsigned)nblk);
    if (mode == 0)
      hipLaunchKernelGGL(u8_tiles_sym_tr_k<0>, g, dim3(256), 0, st, s, origins, D, edge, m, out, mean, std, nu, nv);
    else if (mode == TEM_BOUNDARY_REFLECT)
      hipLaunchKernelGGL(u8_tiles_sym_tr_k<TEM_BOUNDARY_REFLECT>, g, dim3(256), 0, st, s, origins, D, edge, m, out, mean,
                         std, nu, nv);
    else
      hipLaunchKernelGGL(u8_tiles_sym_tr_k<TEM_BOUNDARY_EDGE>, g, dim3(256), 0, st, s, origins, D, edge, m, out, mean, std,
                         nu, nv);
  }
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

// the launch of either accumulate; `spread` null: the mean alone
int accum_sym(const float *y, int32_t ntile, int32_t yedge, bool is3d, int32_t p0, int32_t p1, int32_t p2, int32_t f0,
              int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor, float *const *spread, hipStream_t st) {
  SymDev m;
  if (!y || !acc || y == acc || ntile < 0 || yedge < 1 || yedge > 46340 || (first != 0 && first != 1) || divisor < 1 ||
      !sym_ok(p0, p1, p2, f0, f1, f2, is3d, m))
    return TEM_EINVAL;
  const int D = is3d ? yedge : 1;
  const int64_t count = (int64_t)ntile * D * yedge * yedge;           // elements of y and of every destination
  if (spread) {                                                        // five arrays of `count` floats, pairwise disjoint
    const uintptr_t a[5] = {(uintptr_t)y, (uintptr_t)acc, (uintptr_t)spread[0], (uintptr_t)spread[1],
                            (uintptr_t)spread[2]};
    const uintptr_t bytes = (uintptr_t)count * sizeof(float);
    for (int i = 0; i < 5; ++i) {
      if (!a[i]) return TEM_EINVAL;
      for (int j = 0; j < i; ++j)
        if (a[i] == a[j] || (a[i] < a[j] + bytes && a[j] < a[i] + bytes)) return TEM_EINVAL;
    }
  }
  if (ntile == 0) return TEM_OK;
  const MeanOp mean{acc, first, divisor};
  if (m.ip2 == 2) {
    const int64_t rows = (int64_t)ntile * D * yedge;
    const dim3 g(row_grid(rows));
    if (spread)
      hipLaunchKernelGGL(f32_tiles_sym_accum_row_k<SpreadOp>, g, dim3(256), 0, st, y, D, yedge, m,
                         SpreadOp{mean, spread[0], spread[1], spread[2]}, rows);
    else
      hipLaunchKernelGGL(f32_tiles_sym_accum_row_k<MeanOp>, g, dim3(256), 0, st, y, D, yedge, m, mean, rows);
  } else {
    int nu, nv;
    const int64_t nblk = tr_grid(ntile, D, yedge, m, nu, nv);
    if (!nblk) return TEM_EUNSUPPORTED;
    const dim3 g((unsigned)nblk);
    if (spread)
      hipLaunchKernelGGL(f32_tiles_sym_accum_tr_k<SpreadOp>, g, dim3(256), 0, st, y, D, yedge, m,
                         SpreadOp{mean, spread[0], spread[1], spread[2]}, nu, nv);
    else
      hipLaunchKernelGGL(f32_tiles_sym_accum_tr_k<MeanOp>, g, dim3(256), 0, st, y, D, yedge, m, mean, nu, nv);
  }
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

}  // namespace

extern "C" int tem_u8_tiles_to_f32_std_sym(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly,
                                           int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode,
                                           const int32_t *origins_dev, int32_t ntile, int32_t edge, int32_t p0,
                                           int32_t p1, int32_t p2, int32_t f0, int32_t f1, int32_t f2, float *out,
                                           float mean, float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return gather_sym(TileSrc{blk, BZ, BY, BX, lz, ly, lx, Z, Y, X}, mode, origins_dev, ntile, edge, true, p0, p1, p2, f0,
                    f1, f2, out, mean, std, (hipStream_t)stream);
}

extern "C" int tem_u8_tiles2d_to_f32_std_sym(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz,
                                             int32_t ly, int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode,
                                             const int32_t *origins_dev, int32_t ntile, int32_t edge, int32_t p0,
                                             int32_t p1, int32_t p2, int32_t f0, int32_t f1, int32_t f2, float *out,
                                             float mean, float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return gather_sym(TileSrc{blk, BZ, BY, BX, lz, ly, lx, Z, Y, X}, mode, origins_dev, ntile, edge, false, p0, p1, p2, f0,
                    f1, f2, out, mean, std, (hipStream_t)stream);
}

extern "C" int tem_f32_tiles_sym_accum(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1, int32_t p2,
                                       int32_t f0, int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor,
                                       tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return accum_sym(y, ntile, yedge, true, p0, p1, p2, f0, f1, f2, acc, first, divisor, nullptr, (hipStream_t)stream);
}

extern "C" int tem_f32_tiles2d_sym_accum(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1, int32_t p2,
                                         int32_t f0, int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor,
                                         tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return accum_sym(y, ntile, yedge, false, p0, p1, p2, f0, f1, f2, acc, first, divisor, nullptr, (hipStream_t)stream);
}

extern "C" int tem_f32_tiles_sym_accum_spread(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1,
                                              int32_t p2, int32_t f0, int32_t f1, int32_t f2, float *acc, int32_t first,
                                              int32_t divisor, float *ref, float *s1, float *s2, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  float *const spread[3] = {ref, s1, s2};
  return accum_sym(y, ntile, yedge, true, p0, p1, p2, f0, f1, f2, acc, first, divisor, spread, (hipStream_t)stream);
}

extern "C" int tem_f32_tiles2d_sym_accum_spread(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1,
                                                int32_t p2, int32_t f0, int32_t f1, int32_t f2, float *acc,
                                                int32_t first, int32_t divisor, float *ref, float *s1, float *s2,
                                                tem_stream_t stream) {
  TEM_CLEAR_ERR();
  float *const spread[3] = {ref, s1, s2};
  return accum_sym(y, ntile, yedge, false, p0, p1, p2, f0, f1, f2, acc, first, divisor, spread, (hipStream_t)stream);
}
