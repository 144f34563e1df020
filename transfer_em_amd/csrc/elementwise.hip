// elementwise.hip -- losses, optimizer and data-format kernels of the CycleGAN step.
// All are HBM-streaming kernels (or tiny); float32 storage, float/double accumulation as noted.
#include "tem_common.h"
#include "tile_math.h"
#include <cmath>

namespace {

struct V5 {  // device copy of a tem_view
  float *ptr; int32_t N, D, H, W, C; int64_t sN, sD, sH, sW;
};
inline V5 dv(const tem_view &v) { return V5{v.ptr, v.N, v.D, v.H, v.W, v.C, v.sN, v.sD, v.sH, v.sW}; }

__device__ __forceinline__ int64_t voff(const V5 &v, int64_t i, int &c) {
  // i = dense index over (N,D,H,W,C)
  c = (int)(i % v.C); int64_t r = i / v.C;
  int x = (int)(r % v.W); r /= v.W;
  int y = (int)(r % v.H); r /= v.H;
  int z = (int)(r % v.D); int n = (int)(r / v.D);
  return n * v.sN + z * v.sD + y * v.sH + x * v.sW + c;
}

// the same for tensors of fewer than 2^31 elements: 32-bit divisions (a 64-bit division is ~5x the instructions; the loss
// kernels sit on the step's critical chain between the forward and the backward sweeps)
__device__ __forceinline__ int64_t voff32(const V5 &v, uint32_t i, int &c) {
  uint32_t r = i;
  if (v.C == 1) c = 0; else { c = (int)(r % (uint32_t)v.C); r /= (uint32_t)v.C; }
  const uint32_t x = r % (uint32_t)v.W; r /= (uint32_t)v.W;
  const uint32_t y = r % (uint32_t)v.H; r /= (uint32_t)v.H;
  const uint32_t z = r % (uint32_t)v.D, n = r / (uint32_t)v.D;
  return (int64_t)n * v.sN + (int64_t)z * v.sD + (int64_t)y * v.sH + (int64_t)x * v.sW + c;
}

__device__ __forceinline__ void block_accumulate(double s, double *losses, uint32_t mask, double scale) {
  __shared__ double part[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0 && losses) {
    double t = (part[0] + part[1] + part[2] + part[3]) * scale;
    for (int k = 0; k < 8; ++k)
      if (mask & (1u << k)) atomicAdd(&losses[k], t);
  }
}

__device__ __forceinline__ float pow_gamma(float base, float gamma, float &dpow) {
  // (base^gamma, d/dbase) with tf.pow's gradient gamma*base^(gamma-1)
  if (gamma == 2.f) { dpow = 2.f * base; return base * base; }
  float v = powf(base, gamma);
  float d = gamma * powf(base, gamma - 1.f);
  dpow = isfinite(d) ? d : 0.f;
  return v;
}

// tfa sigmoid_focal_crossentropy(from_logits=True), alpha = 0.5 (cgan.py:78-79)
__global__ __launch_bounds__(256) void focal_logits_k(V5 z, int target, float gamma, double *losses, uint32_t mask,
                                                      double loss_scale, V5 dz, float grad_scale, int64_t total) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int c;
    int64_t o = voff(z, i, c);
    float zz = z.ptr[o];
    float ce = fmaxf(zz, 0.f) - zz * (float)target + log1pf(expf(-fabsf(zz)));
    float pr = 1.f / (1.f + expf(-zz));
    float dce = pr - (float)target;
    float base = target ? 1.f - pr : pr;
    float dbase = target ? -pr * (1.f - pr) : pr * (1.f - pr);
    float dmod, mod = pow_gamma(base, gamma, dmod);
    s += (double)(0.5f * mod * ce);
    if (dz.ptr) {
      int c2;
      dz.ptr[voff(dz, i, c2)] = grad_scale * 0.5f * (dmod * dbase * ce + mod * dce);
    }
  }
  block_accumulate(s, losses, mask, loss_scale);
}

// cgan.py:129-130 / 140-141 with loss_obj_nl (from_logits=False): t = 1 - |a-b|/2
__global__ __launch_bounds__(256) void focal_match_k(V5 a, V5 b, float gamma, double *losses, uint32_t mask,
                                                     double loss_scale, V5 db, float grad_scale, int64_t total) {
  const float eps = 1e-7f, hi = 1.0f - 1e-7f;
  double s = 0.0;
  const bool small = total < ((int64_t)1 << 31);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int c;
    const int64_t oa = small ? voff32(a, (uint32_t)i, c) : voff(a, i, c), ob = small ? voff32(b, (uint32_t)i, c) : voff(b, i, c);
    float av = a.ptr[oa], bv = b.ptr[ob];
    float diff = av - bv;
    float t = 1.f - fabsf(diff) * 0.5f;
    float tc = fminf(fmaxf(t, eps), hi);
    float ce = -logf(tc + eps);
    bool inside = t >= eps && t <= hi;
    float dce = inside ? -1.f / (tc + eps) : 0.f;
    float dmod, mod = pow_gamma(1.f - t, gamma, dmod);
    s += (double)(0.5f * mod * ce);
    if (db.ptr) {
      float dper = 0.5f * (-dmod * ce + mod * dce);
      float sg = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
      db.ptr[small ? voff32(db, (uint32_t)i, c) : voff(db, i, c)] = grad_scale * dper * 0.5f * sg;
    }
  }
  block_accumulate(s, losses, mask, loss_scale);
}

__global__ __launch_bounds__(256) void adam_keras_k(float *theta, const float *grad, float *m, float *v, int64_t n,
                                                    float lr, float b1, float b2, float eps, float gscale,
                                                    const uint32_t *step_dev) {
  // TF's ApplyAdam functor, op for op in float32 (tensorflow/core/kernels/training_ops.cc):
  //   alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t);  m += (g - m)*(1 - beta1);
  //   v += (g*g - v)*(1 - beta2);  var -= (m*alpha) / (sqrt(v) + epsilon)
  float t = (float)(*step_dev) + 1.f;
  float alpha = lr * sqrtf(1.f - powf(b2, t)) / (1.f - powf(b1, t));
  float omb1 = 1.f - b1, omb2 = 1.f - b2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float g = gscale * grad[i];
    float mm = m[i] + (g - m[i]) * omb1;
    float vv = v[i] + (g * g - v[i]) * omb2;
    m[i] = mm; v[i] = vv;
    theta[i] = theta[i] - (mm * alpha) / (sqrtf(vv) + eps);
  }
}

__global__ void step_tick_k(uint32_t *s) { *s += 1u; }

// u8_std / unstd_u8, the per-voxel arithmetic of every uint8 <-> float boundary, and bc_fold: tile_math.h

__global__ __launch_bounds__(256) void u8_to_f32_std_k(const uint8_t *in, float *out, int64_t n, float mean, float std) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = u8_std((float)in[i], mean, std);
}

__global__ __launch_bounds__(256) void f32_unstd_to_u8_k(V5 y, uint8_t *out, int64_t oD, int64_t oH, int64_t oW,
                                                         float mean, float std, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int x = (int)(i % y.W); int64_t r = i / y.W;
    int yy = (int)(r % y.H); int z = (int)(r / y.H);
    out[z * oD + yy * oH + x * oW] = unstd_u8(y.ptr[z * y.sD + yy * y.sH + x * y.sW], mean, std);
  }
}

__global__ __launch_bounds__(256) void fill_k(float *dst, int64_t n, float value) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = value;
}

template <bool ADD>
__global__ __launch_bounds__(256) void copy_view_k(V5 s, V5 d, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int c;
    int64_t so = voff(s, i, c), dof = voff(d, i, c);
    d.ptr[dof] = ADD ? d.ptr[dof] + s.ptr[so] : s.ptr[so];
  }
}

// g(view) = saved > 0 ? g : slope * g  (LeakyReLU gradient gated on the saved OUTPUT, in place)
__global__ __launch_bounds__(256) void leaky_gate_view_k(V5 g, V5 sv, float slope, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int c;
    int64_t go = voff(g, i, c), so = voff(sv, i, c);
    float v = g.ptr[go];
    g.ptr[go] = sv.ptr[so] > 0.f ? v : slope * v;
  }
}

// ---------------------------------------------------------------- InstanceNormalization (models/utils.py:10-38)
// One workgroup per (n, c): two passes over the channel's voxels (mean, then the mean squared deviation, as
// tf.nn.moments does), double accumulation, fixed summation order.  Channels-last makes a channel a stride-C
// gather, but all C workgroups of a sample walk the same cache lines at the same time, so HBM sees one pass.
__device__ __forceinline__ double block_sum_1024(double s, double *part) {
  s = wave_sum(s);
  __syncthreads();                                        // part[] may still be read from a previous call
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += part[w];
  return t;
}

__device__ __forceinline__ int64_t vox_off(const V5 &v, int64_t i) {   // i over (D,H,W)
  int x = (int)(i % v.W); int64_t r = i / v.W;
  int y = (int)(r % v.H); int z = (int)(r / v.H);
  return z * v.sD + y * v.sH + x * v.sW;
}

__global__ __launch_bounds__(1024) void inorm_stats_k(V5 x, float eps, float *mean_out, float *rstd_out) {
  __shared__ double part[16];
  const int n = blockIdx.x / x.C, c = blockIdx.x % x.C;
  const int64_t vox = (int64_t)x.D * x.H * x.W;
  const float *xp = x.ptr + n * x.sN + c;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < vox; i += blockDim.x) s += (double)xp[vox_off(x, i)];
  const float mean = (float)(block_sum_1024(s, part) / (double)vox);
  s = 0.0;
  for (int64_t i = threadIdx.x; i < vox; i += blockDim.x) {
    const float d = xp[vox_off(x, i)] - mean;
    s += (double)(d * d);
  }
  const float var = (float)(block_sum_1024(s, part) / (double)vox);
  if (threadIdx.x == 0) { mean_out[blockIdx.x] = mean; rstd_out[blockIdx.x] = rsqrtf(var + eps); }
}

// y = scale[c] * ((x - mean[n,c]) * rstd[n,c]) + offset[c]
__global__ __launch_bounds__(256) void inorm_apply_k(V5 x, V5 y, const float *scale, const float *offset, const float *mean,
                                                     const float *rstd, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int c, c2;
    const int64_t xo = voff(x, i, c), yo = voff(y, i, c2);
    const int n = (int)(i / ((int64_t)x.D * x.H * x.W * x.C));
    const float nrm = (x.ptr[xo] - mean[n * x.C + c]) * rstd[n * x.C + c];
    y.ptr[yo] = scale[c] * nrm + offset[c];
  }
}

// per (n, c): s1 = sum dy, s2 = sum dy * xhat  (double), written to sums[(n*C + c)*2 + {0,1}]
__global__ __launch_bounds__(1024) void inorm_bwd_sums_k(V5 x, V5 dy, const float *mean, const float *rstd, double *sums) {
  __shared__ double part[16];
  const int n = blockIdx.x / x.C, c = blockIdx.x % x.C;
  const int64_t vox = (int64_t)x.D * x.H * x.W;
  const float *xp = x.ptr + n * x.sN + c, *gp = dy.ptr + n * dy.sN + c;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = threadIdx.x; i < vox; i += blockDim.x) {
    const float g = gp[vox_off(dy, i)], xh = (xp[vox_off(x, i)] - mu) * rs;
    s1 += (double)g; s2 += (double)(g * xh);
  }
  s1 = block_sum_1024(s1, part);
  s2 = block_sum_1024(s2, part);
  if (threadIdx.x == 0) { sums[blockIdx.x * 2] = s1; sums[blockIdx.x * 2 + 1] = s2; }
}

// dx = scale*rstd * (dy - mean(dy) - xhat * mean(dy*xhat));  block 0 also folds the sums over n into dscale / doffset
__global__ __launch_bounds__(256) void inorm_bwd_apply_k(V5 x, V5 dy, V5 dx, const float *scale, const float *mean,
                                                         const float *rstd, const double *sums, float *dscale,
                                                         float *doffset, int64_t total) {
  const double inv = 1.0 / (double)((int64_t)x.D * x.H * x.W);
  if (blockIdx.x == 0 && (int)threadIdx.x < x.C) {
    double a = 0.0, b = 0.0;
    for (int n = 0; n < x.N; ++n) { a += sums[(n * x.C + threadIdx.x) * 2]; b += sums[(n * x.C + threadIdx.x) * 2 + 1]; }
    if (doffset) doffset[threadIdx.x] = (float)a;
    if (dscale) dscale[threadIdx.x] = (float)b;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int c, c2, c3;
    const int64_t xo = voff(x, i, c), go = voff(dy, i, c2), doo = voff(dx, i, c3);
    const int nc = (int)(i / ((int64_t)x.D * x.H * x.W * x.C)) * x.C + c;
    const float xh = (x.ptr[xo] - mean[nc]) * rstd[nc];
    const float m1 = (float)(sums[nc * 2] * inv), m2 = (float)(sums[nc * 2 + 1] * inv);
    dx.ptr[doo] = scale[c] * rstd[nc] * (dy.ptr[go] - m1 - xh * m2);
  }
}

// ---------------------------------------------------------------- tiled inference boundaries (utils.py:77-126)
// gather: tile t = the edge^3 window of the uint8 volume at origins[t] (zeros outside), scaled + standardized
__global__ __launch_bounds__(256) void u8_tiles_to_f32_std_k(const uint8_t *vol, int Z, int Y, int X, const int32_t *origins,
                                                             int edge, float *out, float mean, float std, int64_t per_tile) {
  const int t = blockIdx.y;
  const int oz = origins[3 * t], oy = origins[3 * t + 1], ox = origins[3 * t + 2];
  float *o = out + (int64_t)t * per_tile;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_tile; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % edge); const int64_t r = i / edge;
    const int y = (int)(r % edge), z = (int)(r / edge);
    const int gz = oz + z, gy = oy + y, gx = ox + x;
    const bool in = (unsigned)gz < (unsigned)Z && (unsigned)gy < (unsigned)Y && (unsigned)gx < (unsigned)X;
    o[i] = u8_std(in ? (float)vol[((int64_t)gz * Y + gy) * X + gx] : 0.f, mean, std);
  }
}

// gather with a boundary mode: as u8_tiles_to_f32_std_k on the staging block blk[BZ][BY][BX] that holds the volume's
// box at (lz, ly, lx); a voxel outside the volume [0,Z)x[0,Y)x[0,X) reads the volume voxel bc_fold names.  A folded
// coordinate outside the block reads 0 (the planner's footprint hull holds them all; the predicate keeps a wrong plan
// from reading outside blk).  A tile inside the volume (uniform per workgroup) runs the plain loop; a face tile goes
// row by row, one wave per row, so that z and y are folded once per row (in scalar registers) and only x per voxel.
template <int MODE>
__global__ __launch_bounds__(256) void u8_tiles_to_f32_std_bc_k(const uint8_t *blk, int BZ, int BY, int BX, int lz, int ly,
                                                                int lx, int Z, int Y, int X, const int32_t *origins,
                                                                int edge, float *out, float mean, float std,
                                                                int64_t per_tile) {
  const int t = blockIdx.y;
  const int oz = origins[3 * t], oy = origins[3 * t + 1], ox = origins[3 * t + 2];
  const int vz = lz + oz, vy = ly + oy, vx = lx + ox;                  // the tile's origin in volume coordinates
  float *o = out + (int64_t)t * per_tile;
  if (vz >= 0 && vz + edge <= Z && vy >= 0 && vy + edge <= Y && vx >= 0 && vx + edge <= X) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_tile; i += (int64_t)gridDim.x * 256) {
      const int x = (int)(i % edge); const int64_t r = i / edge;
      const int y = (int)(r % edge), z = (int)(r / edge);
      const int gz = oz + z, gy = oy + y, gx = ox + x;
      const bool in = (unsigned)gz < (unsigned)BZ && (unsigned)gy < (unsigned)BY && (unsigned)gx < (unsigned)BX;
      o[i] = u8_std(in ? (float)blk[((int64_t)gz * BY + gy) * BX + gx] : 0.f, mean, std);
    }
    return;
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int rows = edge * edge;                                        // edge <= 46340 (entry point)
  for (int r = (int)blockIdx.x * 4 + wave; r < rows; r += (int)gridDim.x * 4) {
    const int z = r / edge, y = r - z * edge;
    const int bz = bc_fold<MODE>(vz + z, Z) - lz, by = bc_fold<MODE>(vy + y, Y) - ly;
    const bool rin = (unsigned)bz < (unsigned)BZ && (unsigned)by < (unsigned)BY;
    const uint8_t *row = blk + (rin ? ((int64_t)bz * BY + by) * BX : 0);
    float *orow = o + (int64_t)r * edge;
    for (int x = lane; x < edge; x += 64) {
      const int bx = bc_fold<MODE>(vx + x, X) - lx;
      const bool in = rin && (unsigned)bx < (unsigned)BX;
      orow[x] = u8_std(in ? (float)row[bx] : 0.f, mean, std);
    }
  }
}

// The byte a scatter writes for element i of the dense tile batch: the un-standardised prediction, or the spread of the
// self-ensemble finished from its moments (count members; tile_math.h).
struct UnstdVal {
  const float *y; float mean, std;
  __device__ __forceinline__ uint8_t operator()(int64_t i) const { return unstd_u8(y[i], mean, std); }
};

struct SpreadVal {
  const float *s1, *s2; float count, absstd, gain;
  __device__ __forceinline__ uint8_t operator()(int64_t i) const { return spread_u8(s1[i], s2[i], count, absstd, gain); }
};

// scatter: the interior (tpad stripped, utils.py:113-116) of tile t of y -> uint8 block of the output volume at index[t]
template <class Val>
__global__ __launch_bounds__(256) void f32_tiles_to_u8_k(Val val, int yedge, int tpad, const int32_t *index,
                                                         uint8_t *out, int OY, int OX) {
  const int t = blockIdx.y, od = yedge - 2 * tpad;
  const int iz = index[3 * t], iy = index[3 * t + 1], ix = index[3 * t + 2];
  const int64_t src = (int64_t)t * yedge * yedge * yedge;
  const int64_t per_tile = (int64_t)od * od * od;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_tile; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % od); const int64_t r = i / od;
    const int yy = (int)(r % od), z = (int)(r / od);
    out[((int64_t)(iz + z) * OY + (iy + yy)) * OX + (ix + x)] =
        val(src + ((int64_t)(z + tpad) * yedge + (yy + tpad)) * yedge + (x + tpad));
  }
}

// 2-D tiles (one section each).  Thousands of small tiles per batch: the grid is flat over all tiles' element groups
// (no blockIdx.y tile, so no 65,535-tile limit), and xcd_contiguous_block keeps neighbouring groups -- one tile's rows,
// then the next tile's -- in one XCD's L2.
// gather: thread g fills V consecutive floats of the flat ntile x edge x edge output (one dwordx4 store when V == 4:
// edge even => every tile starts on 16 bytes); the V pixels may wrap onto the next row of the tile
template <int V>
__global__ __launch_bounds__(256) void u8_tiles2d_to_f32_std_k(const uint8_t *vol, int Z, int Y, int X,
                                                               const int32_t *origins, int edge, float *out, float mean,
                                                               float std, int64_t ngroup) {
  const int64_t g = (int64_t)xcd_contiguous_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= ngroup) return;
  const int per_tile = edge * edge / V;                        // groups per tile (edge * edge % V == 0)
  const int t = (int)(g / per_tile), e = (int)(g - (int64_t)t * per_tile) * V;
  const int oz = origins[3 * t], oy = origins[3 * t + 1], ox = origins[3 * t + 2];
  int yy = e / edge, xx = e - yy * edge;
  const bool zin = (unsigned)oz < (unsigned)Z;
  const uint8_t *plane = vol + (int64_t)(zin ? oz : 0) * Y * X;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (xx == edge) { xx = 0; ++yy; }
    const int gy = oy + yy, gx = ox + xx;
    const bool in = zin && (unsigned)gy < (unsigned)Y && (unsigned)gx < (unsigned)X;
    v[j] = u8_std(in ? (float)plane[(int64_t)gy * X + gx] : 0.f, mean, std);
    ++xx;
  }
  float *o = out + g * V;
  if constexpr (V == 4)
    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
  else
    o[0] = v[0];
}

// gather with a boundary mode (see u8_tiles_to_f32_std_bc_k): the same flat grid and stores over the staging block
// blk[BZ][BY][BX] at (lz, ly, lx).  A thread of a tile inside the volume runs the plain loop; a thread of a face tile
// folds its section once, its row once (again where its V pixels wrap onto the next row) and x per pixel.
template <int V, int MODE>
__global__ __launch_bounds__(256) void u8_tiles2d_to_f32_std_bc_k(const uint8_t *blk, int BZ, int BY, int BX, int lz,
                                                                  int ly, int lx, int Z, int Y, int X,
                                                                  const int32_t *origins, int edge, float *out,
                                                                  float mean, float std, int64_t ngroup) {
  const int64_t g = (int64_t)xcd_contiguous_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= ngroup) return;
  const int per_tile = edge * edge / V;                        // groups per tile (edge * edge % V == 0)
  const int t = (int)(g / per_tile), e = (int)(g - (int64_t)t * per_tile) * V;
  const int oz = origins[3 * t], oy = origins[3 * t + 1], ox = origins[3 * t + 2];
  const int vz = lz + oz, vy = ly + oy, vx = lx + ox;          // the tile's origin in volume coordinates
  int yy = e / edge, xx = e - yy * edge;
  float v[V];
  if ((unsigned)vz < (unsigned)Z && vy >= 0 && vy + edge <= Y && vx >= 0 && vx + edge <= X) {
    const bool zin = (unsigned)oz < (unsigned)BZ;
    const uint8_t *plane = blk + (int64_t)(zin ? oz : 0) * BY * BX;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (xx == edge) { xx = 0; ++yy; }
      const int gy = oy + yy, gx = ox + xx;
      const bool in = zin && (unsigned)gy < (unsigned)BY && (unsigned)gx < (unsigned)BX;
      v[j] = u8_std(in ? (float)plane[(int64_t)gy * BX + gx] : 0.f, mean, std);
      ++xx;
    }
  } else {
    const int bz = bc_fold<MODE>(vz, Z) - lz;
    const bool zin = (unsigned)bz < (unsigned)BZ;
    const uint8_t *plane = blk + (int64_t)(zin ? bz : 0) * BY * BX;
    int by = bc_fold<MODE>(vy + yy, Y) - ly;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (xx == edge) { xx = 0; ++yy; by = bc_fold<MODE>(vy + yy, Y) - ly; }
      const int bx = bc_fold<MODE>(vx + xx, X) - lx;
      const bool in = zin && (unsigned)by < (unsigned)BY && (unsigned)bx < (unsigned)BX;
      v[j] = u8_std(in ? (float)plane[(int64_t)by * BX + bx] : 0.f, mean, std);
      ++xx;
    }
  }
  float *o = out + g * V;
  if constexpr (V == 4)
    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
  else
    o[0] = v[0];
}

// scatter: thread g converts 4 consecutive interior pixels of one row of one tile (tpad stripped per side) and writes
// them to out[iz][iy + row][ix + col ...]: one packed dword when the 4 land in the row on a 4-byte boundary, bytes
// otherwise (the tail of a row whose interior is not a multiple of 4, unaligned offsets).  Pixels outside `out` are
// dropped.
template <class Val>
__global__ __launch_bounds__(256) void f32_tiles2d_to_u8_k(Val val, int yedge, int tpad, const int32_t *index,
                                                           uint8_t *out, int OZ, int OY, int OX, int64_t ngroup) {
  const int64_t g = (int64_t)xcd_contiguous_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= ngroup) return;
  const int od = yedge - 2 * tpad, gpr = (od + 3) >> 2, per_tile = od * gpr;
  const int t = (int)(g / per_tile), r = (int)(g - (int64_t)t * per_tile);
  const int row = r / gpr, col = (r - row * gpr) * 4;
  const int iz = index[3 * t], oy = index[3 * t + 1] + row, ox = index[3 * t + 2] + col;
  if ((unsigned)iz >= (unsigned)OZ || (unsigned)oy >= (unsigned)OY) return;
  const int64_t src = (int64_t)t * yedge * yedge + (int64_t)(row + tpad) * yedge + (col + tpad);
  const int n = min(4, od - col);
  uint8_t q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = j < n ? val(src + j) : 0;
  uint8_t *dst = out + ((int64_t)iz * OY + oy) * OX;
  if (n == 4 && ox >= 0 && ox + 4 <= OX && (((uintptr_t)(dst + ox)) & 3) == 0) {
    *reinterpret_cast<uint32_t *>(dst + ox) = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) |
                                              ((uint32_t)q[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n && (unsigned)(ox + j) < (unsigned)OX) dst[ox + j] = q[j];
  }
}

inline unsigned grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
inline int64_t vtotal(const tem_view &v) { return (int64_t)v.N * v.D * v.H * v.W * v.C; }
inline bool same_extents(const tem_view &a, const tem_view &b) {
  return a.N == b.N && a.D == b.D && a.H == b.H && a.W == b.W && a.C == b.C;
}

}  // namespace

extern "C" int tem_focal_logits(const tem_view *z, int32_t target, float gamma, double *losses, uint32_t slot_mask,
                                float loss_scale, const tem_view *dz, float grad_scale, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!z || !tem_view_ok(*z) || (target != 0 && target != 1)) return TEM_EINVAL;
  V5 d{};
  if (dz && dz->ptr) { if (!same_extents(*z, *dz)) return TEM_ESHAPE; d = dv(*dz); }
  int64_t total = vtotal(*z);
  unsigned g = grid_for(total); if (g > 256) g = 256;
  hipLaunchKernelGGL(focal_logits_k, dim3(g), dim3(256), 0, (hipStream_t)stream, dv(*z), target, gamma, losses,
                     slot_mask, (double)loss_scale / (double)total, d, grad_scale / (float)total, total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_focal_match(const tem_view *a, const tem_view *b, float gamma, double *losses, uint32_t slot_mask,
                               float loss_scale, const tem_view *db, float grad_scale, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!a || !b || !tem_view_ok(*a) || !tem_view_ok(*b)) return TEM_EINVAL;
  if (!same_extents(*a, *b)) return TEM_ESHAPE;
  V5 d{};
  if (db && db->ptr) { if (!same_extents(*b, *db)) return TEM_ESHAPE; d = dv(*db); }
  int64_t total = vtotal(*a);
  // Every workgroup ends in one fp64 atomic per loss slot on the same few addresses (~12 ns each, back to back), every
  // loop iteration of a thread costs a load latency (~1.3 us): the grid that balances the two (was 1024 workgroups:
  // loss.cyc_x 38 us, loss.id_x 22 us)
  unsigned g = grid_for(total);
  {
    const int slots = __builtin_popcount(slot_mask) > 0 ? __builtin_popcount(slot_mask) : 1;
    const double best = sqrt((double)total / 256.0 * 1300.0 / (12.0 * slots));
    const unsigned cap = best < 64 ? 64u : (best > 1024 ? 1024u : (unsigned)best);
    if (g > cap) g = cap;
  }
  hipLaunchKernelGGL(focal_match_k, dim3(g), dim3(256), 0, (hipStream_t)stream, dv(*a), dv(*b), gamma, losses,
                     slot_mask, (double)loss_scale / (double)total, d, grad_scale / (float)total, total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_instance_norm(const tem_view *x, const float *scale, const float *offset, float eps,
                                 const tem_view *y, float *mean, float *rstd, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!x || !y || !tem_view_ok(*x) || !tem_view_ok(*y) || !scale || !offset || !mean || !rstd) return TEM_EINVAL;
  if (!same_extents(*x, *y)) return TEM_ESHAPE;
  if (x->C > 256) return TEM_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(inorm_stats_k, dim3(x->N * x->C), dim3(1024), 0, st, dv(*x), eps, mean, rstd);
  TEM_CHECK_LAUNCH();
  const int64_t total = vtotal(*x);
  hipLaunchKernelGGL(inorm_apply_k, dim3(grid_for(total)), dim3(256), 0, st, dv(*x), dv(*y), scale, offset, mean, rstd, total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_instance_norm_bwd(const tem_view *x, const tem_view *dy, const float *scale, const float *mean,
                                     const float *rstd, const tem_view *dx, float *dscale, float *doffset,
                                     double *workspace, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!x || !dy || !dx || !tem_view_ok(*x) || !tem_view_ok(*dy) || !tem_view_ok(*dx) || !scale || !mean || !rstd ||
      !workspace)
    return TEM_EINVAL;
  if (!same_extents(*x, *dy) || !same_extents(*x, *dx)) return TEM_ESHAPE;
  if (x->C > 256) return TEM_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(inorm_bwd_sums_k, dim3(x->N * x->C), dim3(1024), 0, st, dv(*x), dv(*dy), mean, rstd, workspace);
  TEM_CHECK_LAUNCH();
  const int64_t total = vtotal(*x);
  hipLaunchKernelGGL(inorm_bwd_apply_k, dim3(grid_for(total)), dim3(256), 0, st, dv(*x), dv(*dy), dv(*dx), scale, mean,
                     rstd, workspace, dscale, doffset, total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_tiles_to_f32_std(const uint8_t *vol, int32_t Z, int32_t Y, int32_t X, const int32_t *origins_dev,
                                       int32_t ntile, int32_t edge, float *out, float mean, float std,
                                       tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!vol || !origins_dev || !out || Z < 1 || Y < 1 || X < 1 || ntile < 0 || edge < 1) return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  if (ntile > 65535) return TEM_EUNSUPPORTED;
  const int64_t per_tile = (int64_t)edge * edge * edge;
  unsigned gx = grid_for(per_tile); if (gx > 512) gx = 512;
  hipLaunchKernelGGL(u8_tiles_to_f32_std_k, dim3(gx, (unsigned)ntile), dim3(256), 0, (hipStream_t)stream, vol, Z, Y, X,
                     origins_dev, edge, out, mean, std, per_tile);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

namespace {
// the launch of the 3-D scatters; `ok`: the source pointers and the value's own arguments
template <class Val>
int scatter_tiles(Val val, bool ok, int32_t ntile, int32_t yedge, int32_t tpad, const int32_t *index_dev, uint8_t *out,
                  int32_t OZ, int32_t OY, int32_t OX, hipStream_t st) {
  if (!ok || !index_dev || !out || ntile < 0 || yedge < 1 || tpad < 0 || 2 * tpad >= yedge || OZ < 1 || OY < 1 || OX < 1)
    return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  if (ntile > 65535) return TEM_EUNSUPPORTED;
  const int od = yedge - 2 * tpad;
  unsigned gx = grid_for((int64_t)od * od * od); if (gx > 512) gx = 512;
  hipLaunchKernelGGL(f32_tiles_to_u8_k<Val>, dim3(gx, (unsigned)ntile), dim3(256), 0, st, val, yedge, tpad, index_dev, out,
                     OY, OX);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

// ... and of the 2-D ones
template <class Val>
int scatter_tiles2d(Val val, bool ok, int32_t ntile, int32_t yedge, int32_t tpad, const int32_t *index_dev, uint8_t *out,
                    int32_t OZ, int32_t OY, int32_t OX, hipStream_t st) {
  if (!ok || !index_dev || !out || ntile < 0 || yedge < 1 || yedge > 46340 || tpad < 0 || 2 * tpad >= yedge || OZ < 1 ||
      OY < 1 || OX < 1)
    return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  const int od = yedge - 2 * tpad;
  const int64_t ngroup = (int64_t)ntile * od * ((od + 3) / 4);
  const int64_t nblk = (ngroup + 255) / 256;
  if (nblk > 0x7fffffff) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(f32_tiles2d_to_u8_k<Val>, dim3((unsigned)nblk), dim3(256), 0, st, val, yedge, tpad, index_dev, out,
                     OZ, OY, OX, ngroup);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

// the moments, a member count >= 1 and a finite gain > 0
inline bool spread_args_ok(const float *s1, const float *s2, int32_t count, float gain) {
  return s1 && s2 && count >= 1 && gain > 0.f && std::isfinite(gain);
}
}  // namespace

extern "C" int tem_f32_tiles_unstd_to_u8(const float *y, int32_t ntile, int32_t yedge, int32_t tpad,
                                         const int32_t *index_dev, uint8_t *out, int32_t OZ, int32_t OY, int32_t OX,
                                         float mean, float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return scatter_tiles(UnstdVal{y, mean, std}, y != nullptr, ntile, yedge, tpad, index_dev, out, OZ, OY, OX,
                       (hipStream_t)stream);
}

extern "C" int tem_f32_tiles_spread_to_u8(const float *s1, const float *s2, int32_t ntile, int32_t yedge, int32_t tpad,
                                          const int32_t *index_dev, uint8_t *out, int32_t OZ, int32_t OY, int32_t OX,
                                          int32_t count, float std_y, float gain, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return scatter_tiles(SpreadVal{s1, s2, (float)count, fabsf(std_y), gain}, spread_args_ok(s1, s2, count, gain), ntile,
                       yedge, tpad, index_dev, out, OZ, OY, OX, (hipStream_t)stream);
}

extern "C" int tem_u8_tiles2d_to_f32_std(const uint8_t *vol, int32_t Z, int32_t Y, int32_t X, const int32_t *origins_dev,
                                         int32_t ntile, int32_t edge, float *out, float mean, float std,
                                         tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!vol || !origins_dev || !out || Z < 1 || Y < 1 || X < 1 || ntile < 0 || edge < 1 || edge > 46340)
    return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  const int V = (edge % 2 == 0 && ((uintptr_t)out & 15) == 0) ? 4 : 1;
  const int64_t ngroup = (int64_t)ntile * edge * edge / V;
  const int64_t nblk = (ngroup + 255) / 256;
  if (nblk > 0x7fffffff) return TEM_EUNSUPPORTED;
  if (V == 4)
    hipLaunchKernelGGL(u8_tiles2d_to_f32_std_k<4>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, vol, Z, Y,
                       X, origins_dev, edge, out, mean, std, ngroup);
  else
    hipLaunchKernelGGL(u8_tiles2d_to_f32_std_k<1>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, vol, Z, Y,
                       X, origins_dev, edge, out, mean, std, ngroup);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

namespace {
// the block lies inside a non-empty volume, the mode is one the kernels fold by
inline bool bc_args_ok(int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly, int32_t lx, int32_t Z, int32_t Y,
                       int32_t X, int32_t mode) {
  if (mode != TEM_BOUNDARY_REFLECT && mode != TEM_BOUNDARY_EDGE) return false;
  if (Z < 1 || Y < 1 || X < 1 || BZ < 1 || BY < 1 || BX < 1 || lz < 0 || ly < 0 || lx < 0) return false;
  return BZ <= Z - lz && BY <= Y - ly && BX <= X - lx;
}
}  // namespace

extern "C" int tem_u8_tiles_to_f32_std_bc(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly,
                                          int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode,
                                          const int32_t *origins_dev, int32_t ntile, int32_t edge, float *out,
                                          float mean, float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!blk || !origins_dev || !out || !bc_args_ok(BZ, BY, BX, lz, ly, lx, Z, Y, X, mode) || ntile < 0 || edge < 1 ||
      edge > 46340)
    return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  if (ntile > 65535) return TEM_EUNSUPPORTED;
  const int64_t per_tile = (int64_t)edge * edge * edge;
  unsigned gx = grid_for(per_tile); if (gx > 512) gx = 512;
  const dim3 grid(gx, (unsigned)ntile);
  if (mode == TEM_BOUNDARY_REFLECT)
    hipLaunchKernelGGL(u8_tiles_to_f32_std_bc_k<TEM_BOUNDARY_REFLECT>, grid, dim3(256), 0, (hipStream_t)stream, blk, BZ,
                       BY, BX, lz, ly, lx, Z, Y, X, origins_dev, edge, out, mean, std, per_tile);
  else
    hipLaunchKernelGGL(u8_tiles_to_f32_std_bc_k<TEM_BOUNDARY_EDGE>, grid, dim3(256), 0, (hipStream_t)stream, blk, BZ, BY,
                       BX, lz, ly, lx, Z, Y, X, origins_dev, edge, out, mean, std, per_tile);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

namespace {
template <int V>
void launch_tiles2d_bc(int32_t mode, unsigned nblk, hipStream_t st, const uint8_t *blk, int BZ, int BY, int BX, int lz,
                       int ly, int lx, int Z, int Y, int X, const int32_t *origins, int edge, float *out, float mean,
                       float std, int64_t ngroup) {
  if (mode == TEM_BOUNDARY_REFLECT)
    hipLaunchKernelGGL((u8_tiles2d_to_f32_std_bc_k<V, TEM_BOUNDARY_REFLECT>), dim3(nblk), dim3(256), 0, st, blk, BZ, BY,
                       BX, lz, ly, lx, Z, Y, X, origins, edge, out, mean, std, ngroup);
  else
    hipLaunchKernelGGL((u8_tiles2d_to_f32_std_bc_k<V, TEM_BOUNDARY_EDGE>), dim3(nblk), dim3(256), 0, st, blk, BZ, BY, BX,
                       lz, ly, lx, Z, Y, X, origins, edge, out, mean, std, ngroup);
}
}  // namespace

extern "C" int tem_u8_tiles2d_to_f32_std_bc(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz,
                                            int32_t ly, int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode,
                                            const int32_t *origins_dev, int32_t ntile, int32_t edge, float *out,
                                            float mean, float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!blk || !origins_dev || !out || !bc_args_ok(BZ, BY, BX, lz, ly, lx, Z, Y, X, mode) || ntile < 0 || edge < 1 ||
      edge > 46340)
    return TEM_EINVAL;
  if (ntile == 0) return TEM_OK;
  const int V = (edge % 2 == 0 && ((uintptr_t)out & 15) == 0) ? 4 : 1;
  const int64_t ngroup = (int64_t)ntile * edge * edge / V;
  const int64_t nblk = (ngroup + 255) / 256;
  if (nblk > 0x7fffffff) return TEM_EUNSUPPORTED;
  if (V == 4)
    launch_tiles2d_bc<4>(mode, (unsigned)nblk, (hipStream_t)stream, blk, BZ, BY, BX, lz, ly, lx, Z, Y, X, origins_dev,
                         edge, out, mean, std, ngroup);
  else
    launch_tiles2d_bc<1>(mode, (unsigned)nblk, (hipStream_t)stream, blk, BZ, BY, BX, lz, ly, lx, Z, Y, X, origins_dev,
                         edge, out, mean, std, ngroup);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_f32_tiles2d_unstd_to_u8(const float *y, int32_t ntile, int32_t yedge, int32_t tpad,
                                           const int32_t *index_dev, uint8_t *out, int32_t OZ, int32_t OY, int32_t OX,
                                           float mean, float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return scatter_tiles2d(UnstdVal{y, mean, std}, y != nullptr, ntile, yedge, tpad, index_dev, out, OZ, OY, OX,
                         (hipStream_t)stream);
}

extern "C" int tem_f32_tiles2d_spread_to_u8(const float *s1, const float *s2, int32_t ntile, int32_t yedge, int32_t tpad,
                                            const int32_t *index_dev, uint8_t *out, int32_t OZ, int32_t OY, int32_t OX,
                                            int32_t count, float std_y, float gain, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  return scatter_tiles2d(SpreadVal{s1, s2, (float)count, fabsf(std_y), gain}, spread_args_ok(s1, s2, count, gain), ntile,
                         yedge, tpad, index_dev, out, OZ, OY, OX, (hipStream_t)stream);
}

extern "C" int tem_adam_keras(float *theta, const float *grad, float *m, float *v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float grad_scale, const uint32_t *step_dev,
                              tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!theta || !grad || !m || !v || !step_dev || n < 0) return TEM_EINVAL;
  if (n == 0) return TEM_OK;
  hipLaunchKernelGGL(adam_keras_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, theta, grad, m, v, n, lr,
                     beta1, beta2, eps, grad_scale, step_dev);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

// Keep bits of up to two Dropout layers for one step: mask bit e = DropoutStream::bit of dense element e, i.e. the 16
// bytes of 128-element block b ARE the four Philox words of that block (little-endian) -- one 16-byte store per thread.
__global__ __launch_bounds__(256) void dropout_masks_k(uint4 *m0, int64_t nblk0, uint32_t site0, uint4 *m1, int64_t nblk1,
                                                       uint32_t site1, uint32_t k0, uint32_t k1, const uint32_t *step_dev,
                                                       uint32_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk0 + nblk1) return;
  const bool second = i >= nblk0;
  const int64_t b = second ? i - nblk0 : i;
  DropoutStream ds{k0, k1, second ? site1 : site0, step_dev ? *step_dev : step};
  const Philox128 ph = ds.block((uint64_t)b);
  (second ? m1 : m0)[b] = make_uint4(ph.r[0], ph.r[1], ph.r[2], ph.r[3]);
}

extern "C" int tem_dropout_masks(uint8_t *mask0, int64_t nbytes0, uint32_t site0, uint8_t *mask1, int64_t nbytes1,
                                 uint32_t site1, uint64_t seed, const uint32_t *step_dev, uint32_t step,
                                 tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!mask0 || nbytes0 <= 0 || nbytes0 % 16 || ((uintptr_t)mask0 & 15)) return TEM_EINVAL;
  if (mask1 && (nbytes1 <= 0 || nbytes1 % 16 || ((uintptr_t)mask1 & 15))) return TEM_EINVAL;
  const int64_t n0 = nbytes0 / 16, n1 = mask1 ? nbytes1 / 16 : 0;
  hipLaunchKernelGGL(dropout_masks_k, dim3((unsigned)((n0 + n1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint4 *)mask0, n0, site0, (uint4 *)mask1, n1, site1, (uint32_t)seed, (uint32_t)(seed >> 32), step_dev, step);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_step_tick(uint32_t *step_dev, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!step_dev) return TEM_EINVAL;
  hipLaunchKernelGGL(step_tick_k, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_to_f32_std(const uint8_t *in, float *out, int64_t n, float mean, float std,
                                 tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!in || !out || n < 0) return TEM_EINVAL;
  if (n == 0) return TEM_OK;
  hipLaunchKernelGGL(u8_to_f32_std_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n, mean, std);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_f32_unstd_to_u8(const tem_view *y, uint8_t *out, int64_t oD, int64_t oH, int64_t oW, float mean,
                                   float std, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!y || !tem_view_ok(*y) || !out) return TEM_EINVAL;
  int64_t total = (int64_t)y->D * y->H * y->W;
  hipLaunchKernelGGL(f32_unstd_to_u8_k, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dv(*y), out, oD, oH,
                     oW, mean, std, total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_fill_f32(float *dst, int64_t n, float value, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!dst || n < 0) return TEM_EINVAL;
  if (n == 0) return TEM_OK;
  hipLaunchKernelGGL(fill_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dst, n, value);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_copy_view(const tem_view *src, const tem_view *dst, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || !tem_view_ok(*src) || !tem_view_ok(*dst)) return TEM_EINVAL;
  if (!same_extents(*src, *dst)) return TEM_ESHAPE;
  int64_t total = vtotal(*src);
  hipLaunchKernelGGL(copy_view_k<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dv(*src), dv(*dst),
                     total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_add_view(const tem_view *src, const tem_view *dst, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || !tem_view_ok(*src) || !tem_view_ok(*dst)) return TEM_EINVAL;
  if (!same_extents(*src, *dst)) return TEM_ESHAPE;
  int64_t total = vtotal(*src);
  hipLaunchKernelGGL(copy_view_k<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dv(*src), dv(*dst),
                     total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

// theta_t = every conv kernel of a flat parameter vector with its taps reversed and (ci, co) transposed:
//   theta_t[off + ((ntap-1-t)*co + b)*ci + a] = theta[off + (t*ci + a)*co + b];  elements outside the table are copied.
__global__ __launch_bounds__(256) void flip_transpose_k(const float *__restrict__ theta, float *__restrict__ theta_t,
                                                        const tem_wlayer *__restrict__ layers, int nlayers, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t dst = i;
    for (int l = 0; l < nlayers; ++l) {
      const tem_wlayer L = layers[l];
      const int64_t rel = i - L.offset, n = (int64_t)L.ntap * L.ci * L.co;
      if (rel >= 0 && rel < n) {
        const int b = (int)(rel % L.co);
        const int64_t ta = rel / L.co;
        const int a = (int)(ta % L.ci), t = (int)(ta / L.ci);
        dst = L.offset + ((int64_t)(L.ntap - 1 - t) * L.co + b) * L.ci + a;
        break;
      }
    }
    theta_t[dst] = theta[i];
  }
}

extern "C" int tem_flip_transpose(const float *theta, float *theta_t, const tem_wlayer *layers_dev, int32_t nlayers,
                                  int64_t total, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!theta || !theta_t || theta == theta_t || nlayers < 0 || (nlayers > 0 && !layers_dev) || total < 0) return TEM_EINVAL;
  if (total == 0) return TEM_OK;
  hipLaunchKernelGGL(flip_transpose_k, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, theta, theta_t, layers_dev,
                     nlayers, total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_leaky_gate_view(const tem_view *g, const tem_view *saved, float slope, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!g || !saved || !tem_view_ok(*g) || !tem_view_ok(*saved)) return TEM_EINVAL;
  if (!same_extents(*g, *saved)) return TEM_ESHAPE;
  int64_t total = vtotal(*g);
  hipLaunchKernelGGL(leaky_gate_view_k, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dv(*g), dv(*saved), slope,
                     total);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_abi_version(const char **arch) {
  TEM_CLEAR_ERR();
  if (arch) *arch = "gfx950";
  return TEM_ABI_VERSION;
}
