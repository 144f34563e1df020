// batchcrop.hip -- the generator dataset's input side in one pass (datasets.py:69-155 over generators.py:59-118): B
// random crops cut straight out of a uint8 volume (or a float32 block, after the warp) into the standardized,
// augmented float32 batch, plus the per-sample sums of the statistics pass.  HBM-streaming kernels.
#include "tem_common.h"

namespace {

constexpr int kTile = 64;                 // a workgroup writes one 64 x 64 plane tile of one sample's output
constexpr int kLds = kTile + 1;           // row pitch of the LDS tile: column writes are conflict-free

// np.pad(..., mode="reflect") as an index map: i in [-pad_before, n + pad_after) -> [0, n).  Reflection without edge
// repetition is periodic with period 2 (n - 1), so any pad width is covered.
__device__ __forceinline__ int reflect(int i, int n) {
  if (n == 1) return 0;
  const int per = 2 * (n - 1);
  int j = i % per;
  if (j < 0) j += per;
  return j >= n ? per - j : j;
}

// The host pipeline's per-voxel arithmetic, in its order, each step correctly rounded and kept apart (no fma
// contraction): scale_tensor, standardize_population, augment's `* var_adj` and `+ mean_adj`.
__device__ __forceinline__ float crop_value(float v, bool scale, int standardize, float mean, float std, int augment,
                                            float var_adj, float mean_adj) {
  if (scale) {
    v = __fdiv_rn(v, 127.5f);
    asm volatile("" : "+v"(v));
    v = __fsub_rn(v, 1.f);                                       // datasets.py:200
    asm volatile("" : "+v"(v));
  }
  if (standardize) {
    v = __fsub_rn(v, mean);
    asm volatile("" : "+v"(v));
    v = __fdiv_rn(v, std);                                       // datasets.py:161-162
    asm volatile("" : "+v"(v));
  }
  if (augment) {
    v = __fmul_rn(v, var_adj);                                   // datasets.py:152
    asm volatile("" : "+v"(v));
    v = __fadd_rn(v, mean_adj);                                  // datasets.py:153
  }
  return v;
}

// Output axis k of a sample reads source axis perm[k]: its stride, crop origin, padding, crop extent and flip.  Picked
// with select chains, so that nothing is a runtime-indexed array (those would live in scratch memory).
struct CropAxis {
  int64_t stride;
  int org, pad, n, E, flip;
};

__device__ __forceinline__ CropAxis crop_axis(const tem_crop_args &g, const int32_t *prm, int k) {
  const int ax = prm[3 + k];
  auto pick = [ax](int64_t v0, int64_t v1, int64_t v2) { return ax == 0 ? v0 : (ax == 1 ? v1 : v2); };
  CropAxis c;
  c.stride = pick(g.sZ, g.sY, g.sX);
  c.org = (int)pick(prm[0], prm[1], prm[2]);
  c.pad = (int)pick(g.pad_lo[0], g.pad_lo[1], g.pad_lo[2]);
  c.n = (int)pick(g.n[0], g.n[1], g.n[2]);
  c.E = c.n + c.pad + (int)pick(g.pad_hi[0], g.pad_hi[1], g.pad_hi[2]);
  c.flip = prm[6 + k];
  return c;
}

__device__ __forceinline__ int64_t crop_offset(const CropAxis &c, int o) {
  const int s = c.flip ? c.E - 1 - o : o;                        // index into the padded crop
  return (int64_t)(c.org + reflect(s - c.pad, c.n)) * c.stride;
}

// One workgroup = one 64 x 64 tile of the plane (a, 2) of sample b's output at a fixed index of the third output axis
// m.  The output axis `a` is the one that reads the source's fastest axis (x): perm[a] == 2.  When perm[2] == 2 the
// plane is (1, 2) and both the reads and the writes run along x.  Otherwise the tile is loaded with lanes along source
// x (coalesced bytes), transposed through LDS, and written with lanes along output x (dwordx4 stores).
template <typename T>
__global__ __launch_bounds__(256) void crop_batch_k(tem_crop_args g) {
  __shared__ float tile[kTile * kLds];
  const int b = blockIdx.y;
  const int32_t *prm = g.params + 12 * b;
  if (((1 << (prm[3] & 3)) | (1 << (prm[4] & 3)) | (1 << (prm[5] & 3))) != 7 || prm[3] > 2 || prm[4] > 2 || prm[5] > 2)
    return;                                                       // not a permutation: the host never sends one
  const CropAxis A0 = crop_axis(g, prm, 0), A1 = crop_axis(g, prm, 1), A2 = crop_axis(g, prm, 2);
  const float var_adj = __int_as_float(prm[9]), mean_adj = __int_as_float(prm[10]);
  const bool a0axis = prm[3] == 2;                                // a == 0 (m == 1); else a == 1 (m == 0)
  const int Ea = a0axis ? A0.E : A1.E, Em = a0axis ? A1.E : A0.E;
  const int ta = (Ea + kTile - 1) / kTile, tc = (A2.E + kTile - 1) / kTile;
  const int blk = blockIdx.x;
  if (blk >= Em * ta * tc) return;
  const int om = blk / (ta * tc), a0 = (blk / tc) % ta * kTile, c0 = blk % tc * kTile;
  const int64_t total = (int64_t)A0.E * A1.E * A2.E;
  float *dst = g.dst + (int64_t)b * total;
  const bool inside = prm[0] >= 0 && prm[1] >= 0 && prm[2] >= 0 && (int64_t)prm[0] + g.n[0] <= g.vol[0] &&
                      (int64_t)prm[1] + g.n[1] <= g.vol[1] && (int64_t)prm[2] + g.n[2] <= g.vol[2];
  const T *src = reinterpret_cast<const T *>(g.src) + (int64_t)b * g.sB;
  const bool along_x = prm[5] == 2;                               // source x is the output's fastest axis

  // load: element (la, lc) of the tile is output voxel (o_m = om, o_a = a0 + la, o_2 = c0 + lc)
  for (int i = 0; i < kTile / 4; ++i) {
    const int fast = threadIdx.x & 63, slow = (threadIdx.x >> 6) + 4 * i;
    const int la = along_x ? slow : fast, lc = along_x ? fast : slow;
    const int oa = a0 + la, o2 = c0 + lc;
    if (oa >= Ea || o2 >= A2.E) continue;
    const int o0 = a0axis ? oa : om, o1 = a0axis ? om : oa;
    float v = __int_as_float(0x7fc00000);                         // a crop outside the volume reads NaN, never memory
    if (inside) {
      const int64_t off = crop_offset(A0, o0) + crop_offset(A1, o1) + crop_offset(A2, o2);
      v = crop_value((float)src[off], sizeof(T) == 1, g.standardize, g.mean, g.std, g.augment, var_adj, mean_adj);
    }
    tile[la * kLds + lc] = v;
  }
  __syncthreads();

  // store: 16 lanes x 4 floats per output row of the tile
  const int cq = threadIdx.x & 15;
  const int64_t sa = a0axis ? (int64_t)A1.E * A2.E : A2.E, sm = a0axis ? A2.E : (int64_t)A1.E * A2.E;
  const bool vec = (A2.E & 3) == 0;
  for (int r = threadIdx.x >> 4; r < kTile; r += 16) {
    const int oa = a0 + r, oc = c0 + 4 * cq;
    if (oa >= Ea || oc >= A2.E) continue;
    const float *t = tile + r * kLds + 4 * cq;
    float *d = dst + om * sm + oa * sa + oc;
    if (vec) {
      *reinterpret_cast<float4 *>(d) = make_float4(t[0], t[1], t[2], t[3]);
    } else {
      for (int j = 0; j < 4 && oc + j < A2.E; ++j) d[j] = t[j];
    }
  }
}

// per-sample partial sums in float64: block (k, b) strides over sample b -> partials[b][k] = {sum, sum of squares}
__global__ __launch_bounds__(256) void sample_sums_k(const float *src, int64_t n, double *partials) {
  __shared__ double part[8];
  const int b = blockIdx.y;
  const float *s = src + (int64_t)b * n;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = (double)s[i];
    s1 += v;
    s2 += v * v;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = s1; part[4 + (threadIdx.x >> 6)] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double *p = partials + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
    p[0] = part[0] + part[1] + part[2] + part[3];
    p[1] = part[4] + part[5] + part[6] + part[7];
  }
}

}  // namespace

extern "C" int tem_crop_batch(const tem_crop_args *args, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!args) return TEM_EINVAL;
  const tem_crop_args &g = *args;
  if (!g.src || !g.params || !g.dst || g.B < 1 || g.B > 65535 || (g.src_f32 != 0 && g.src_f32 != 1)) return TEM_EINVAL;
  if (((uintptr_t)g.dst & 15) != 0) return TEM_EINVAL;
  int ext[3];
  for (int k = 0; k < 3; ++k) {
    if (g.n[k] < 1 || g.pad_lo[k] < 0 || g.pad_hi[k] < 0 || g.vol[k] < g.n[k]) return TEM_EINVAL;
    if (g.n[k] == 1 && (g.pad_lo[k] || g.pad_hi[k])) return TEM_EINVAL;     // np.pad cannot reflect a single voxel
    ext[k] = g.n[k] + g.pad_lo[k] + g.pad_hi[k];
  }
  if (g.standardize && !(g.std != 0.f)) return TEM_EINVAL;
  // grid: the most tiles any permutation of the extents needs (plane (a, 2) x the third axis)
  int64_t nblk = 0;
  const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (const auto &p : P) {
    const int64_t E0 = ext[p[0]], E1 = ext[p[1]], E2 = ext[p[2]];
    const int a = p[0] == 2 ? 0 : 1, mm = a == 0 ? 1 : 0;
    const int64_t Ea = a == 0 ? E0 : E1, Em = mm == 0 ? E0 : E1;
    const int64_t t = Em * ((Ea + kTile - 1) / kTile) * ((E2 + kTile - 1) / kTile);
    nblk = t > nblk ? t : nblk;
  }
  if (nblk > 0x7fffffff) return TEM_EINVAL;
  if (g.src_f32)
    hipLaunchKernelGGL(crop_batch_k<float>, dim3((unsigned)nblk, (unsigned)g.B), dim3(256), 0, (hipStream_t)stream, g);
  else
    hipLaunchKernelGGL(crop_batch_k<uint8_t>, dim3((unsigned)nblk, (unsigned)g.B), dim3(256), 0, (hipStream_t)stream, g);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_sample_sums_f32(const float *src, int32_t B, int64_t n, int32_t nblk, double *partials,
                                   tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !partials || B < 1 || B > 65535 || n < 1 || nblk < 1) return TEM_EINVAL;
  hipLaunchKernelGGL(sample_sums_k, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, src, n, partials);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
