// bww2d_bf16.hip -- 2-D kernel gradient for the bf16 mixed-precision mode: the 2-D twin of bww_bf16.hip (bf16
// activations and gradients in, fp32 accumulation on the matrix cores, one fp32 partial slab per workgroup out,
// finished by tem_reduce_slabs_multi).  Views are (N, 1, H, W, C).
//
//   dW[(tap,ci)][co] = sum over output pixels o of  X[o*S + tap - P][ci] * G[o][co]
//
// GEMM with M = (tap,ci) rows (9 C_in or 16 C_in), N = co and K = pixels.  Both operands are read K-major from the
// channels-last LDS image with ds_read_b64_tr_b16 (per 16-lane group a [4 pixels][16 channels] block) into
// v_mfma_f32_16x16x16_bf16.  The work is a list of (image, band of TY output rows) units; a workgroup owns a contiguous
// run of them (across image boundaries) and ALL accumulator tiles of the layer, which stay in registers for the whole
// run.  Per unit it loads the band's input rows and gradient rows into LDS; the next unit's loads fly in registers under
// the current unit's matrix work.  C_in == 1 (first layers, and the swapped form of the C_out == 1 layer) takes its A
// fragments with plain 2-byte reads: 4 consecutive pixels of one tap are contiguous.
#include "bf16_common.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace bww2d_bf16 {

using namespace tem_bf16;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

struct Dev {
  const u16 *in0, *in1;
  int32_t i0N, i0H, i0W, i1N, i1H, i1W, C0;
  int32_t H, W;
  const u16 *g;
  int32_t gN, gH, gW, OH, OW, P;
  float *slabs;
  int64_t slab_stride;
  int32_t TY, nband, units, per;             // rows per band, bands per image, (image, band) units, units per workgroup
  int32_t rows, colsR, colsA, OWp;           // X patch rows, loaded / allocated columns; G row length padded to 16
  uint32_t magicColsR, magicOW;
};

template <int CI, int CO, int K, int S, int PFX, int PFG>
__global__ __launch_bounds__(256) void bww2d_bf16_k(Dev p) {
  constexpr int NTAP = K * K, ROWS = NTAP * CI, MT = (ROWS + 15) / 16, NT = (CO + 15) / 16;
  constexpr int NB = NT;                                   // n-tiles per wave (C_out 32: each A fragment meets both)
  constexpr int WPN = 4;                                   // the four waves split the m-tiles
  constexpr int TPW = (MT + WPN - 1) / WPN;                // m-tiles per wave (x NB accumulator tiles)
  constexpr int PITCH = CI >= 8 ? (CI <= 16 ? CI : CI + 4) : 1;     // voxel pitches as in bww_bf16.hip
  constexpr int GP = CO <= 16 ? CO : CO + 4;
  constexpr int CPX = CI >= 8 ? CI / 8 : 1, CPG = CO / 8;  // 16-byte chunks per voxel
  static_assert(CO % 8 == 0 && (CI == 1 || CI % 8 == 0) && NT <= 2, "channel counts");
  static_assert(CI > 1 || S == 1, "C_in 1: stride 1");
  extern __shared__ __attribute__((aligned(16))) u16 lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g4 = lane >> 4, q = m >> 2, pq = m & 3;
  u16 *Xs = lds;
  const int x_elems = (p.rows * p.colsA * PITCH + 7) & ~7;
  u16 *Gs = lds + x_elems;
  const int g_elems = p.TY * p.OWp * GP + 16;

  const int u0 = blockIdx.x * p.per, u1 = min(p.units, u0 + p.per);

  // zero the whole image once: padded columns are never written again and must stay zero (G) / finite (X)
  for (int i = tid; i < (x_elems + g_elems + 7) / 8; i += 256) reinterpret_cast<uint4 *>(lds)[i] = make_uint4(0u, 0u, 0u, 0u);

  // ---- this wave's accumulator tiles: m-tiles wave + j*WPN, all n-tiles
  int aconst[TPW];                                         // fragment offset of the lane inside the X image
  f32x4 acc[TPW][NB];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int mt = min(wave + j * WPN, MT - 1);            // surplus tiles recompute the last one, never stored
    if constexpr (CI >= 8) {
      const int m0 = min(16 * mt + 4 * pq, ROWS - 4);     // this lane addresses rows m0..m0+3 (4 channels of one tap)
      const int tap = m0 / CI, ci0 = m0 - tap * CI;
      const int dy = tap / K, dx = tap - dy * K;
      aconst[j] = (dy * p.colsA + dx) * PITCH + ci0 + (4 * g4 + q) * S * PITCH;
    } else {
      const int tap = min(16 * mt + m, NTAP - 1);          // row m of the tile = one tap
      const int dy = tap / K, dx = tap - dy * K;
      aconst[j] = dy * p.colsA + dx + 4 * g4;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[j][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int bconst[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bconst[nb] = (4 * g4 + q) * GP + min(nb * 16 + 4 * pq, CO + 4 - 4);

  const int nk = p.OWp >> 4;
  typedef typename std::conditional<(CI >= 8), uint4, u16>::type xchunk;
  auto issue_x = [&](int u, xchunk (&pf)[PFX]) {           // global loads of the input rows of unit u
    const int n = u / p.nband, band = u - n * p.nband;
    const int iy0 = band * p.TY * S - p.P;
#pragma unroll
    for (int i = 0; i < PFX; ++i) {
      const int id = tid + i * 256;
      if constexpr (CI >= 8) {
        const int totalX = p.rows * p.colsR * CPX;
        const int vox = id / CPX, c8 = (id - vox * CPX) * 8;
        const int r = fdiv(vox, p.colsR, p.magicColsR), cx = vox - r * p.colsR;
        const int iy = iy0 + r, ix = cx - p.P;
        const bool ok = id < totalX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const u16 *src = c8 < p.C0 ? p.in0 + (n * p.i0N + iy * p.i0H + ix * p.i0W + c8)
                                   : p.in1 + (n * p.i1N + iy * p.i1H + ix * p.i1W + (c8 - p.C0));
        pf[i] = ok ? *reinterpret_cast<const uint4 *>(src) : make_uint4(0u, 0u, 0u, 0u);
      } else {
        const int totalX = p.rows * p.colsR;
        const int r = fdiv(id, p.colsR, p.magicColsR), cx = id - r * p.colsR;
        const int iy = iy0 + r, ix = cx - p.P;
        const bool ok = id < totalX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        pf[i] = ok ? p.in0[n * p.i0N + iy * p.i0H + ix * p.i0W] : (u16)0;
      }
    }
  };
  auto commit_x = [&](const xchunk (&pf)[PFX]) {
#pragma unroll
    for (int i = 0; i < PFX; ++i) {
      const int id = tid + i * 256;
      if constexpr (CI >= 8) {
        if (id < p.rows * p.colsR * CPX) {
          const int vox = id / CPX, c8 = (id - vox * CPX) * 8;
          const int r = fdiv(vox, p.colsR, p.magicColsR), cx = vox - r * p.colsR;
          u16 *d = Xs + (r * p.colsA + cx) * PITCH + c8;      // 8-byte aligned
          *reinterpret_cast<uint2 *>(d) = make_uint2(pf[i].x, pf[i].y);
          *reinterpret_cast<uint2 *>(d + 4) = make_uint2(pf[i].z, pf[i].w);
        }
      } else {
        if (id < p.rows * p.colsR) {
          const int r = fdiv(id, p.colsR, p.magicColsR), cx = id - r * p.colsR;
          Xs[r * p.colsA + cx] = pf[i];
        }
      }
    }
  };
  auto rows_of = [&](int u) { const int band = u % p.nband; return min(p.TY, p.OH - band * p.TY); };
  auto issue_g = [&](int u, uint4 (&pg)[PFG]) {
    const int n = u / p.nband, band = u - n * p.nband;
    const int oy0 = band * p.TY;
    const int totalG = min(p.TY, p.OH - oy0) * p.OW * CPG;
#pragma unroll
    for (int i = 0; i < PFG; ++i) {
      const int id = tid + i * 256;
      const int vox = id / CPG, c = (id - vox * CPG) * 8;
      const int r = fdiv(vox, p.OW, p.magicOW), x = vox - r * p.OW;
      pg[i] = id < totalG ? *reinterpret_cast<const uint4 *>(p.g + (n * p.gN + (oy0 + r) * p.gH + x * p.gW + c))
                          : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto commit_g = [&](int u, const uint4 (&pg)[PFG]) {
    const int totalG = rows_of(u) * p.OW * CPG;
#pragma unroll
    for (int i = 0; i < PFG; ++i) {
      const int id = tid + i * 256;
      if (id < totalG) {
        const int vox = id / CPG, c = (id - vox * CPG) * 8;
        const int r = fdiv(vox, p.OW, p.magicOW), x = vox - r * p.OW;
        u16 *d = Gs + (r * p.OWp + x) * GP + c;
        *reinterpret_cast<uint2 *>(d) = make_uint2(pg[i].x, pg[i].y);
        *reinterpret_cast<uint2 *>(d + 4) = make_uint2(pg[i].z, pg[i].w);
      }
    }
  };
  // prologue: the first unit's rows
  if (u0 < u1) {
    xchunk pf[PFX];
    uint4 pg[PFG];
    __syncthreads();                                         // zero fill done
    issue_x(u0, pf);
    issue_g(u0, pg);
    commit_x(pf);
    commit_g(u0, pg);
  }
  for (int u = u0; u < u1; ++u) {
    __syncthreads();                                         // this unit's image is complete
    // the next unit's rows fly into registers under this unit's matrix work
    const bool more = u + 1 < u1;
    xchunk nf[PFX];
    uint4 ng[PFG];
    if (more) {
      issue_x(u + 1, nf);
      issue_g(u + 1, ng);
    }
    const int TYr = rows_of(u);
    for (int r = 0; r < TYr; ++r) {
      const u16 *xr = Xs + r * S * p.colsA * PITCH;
      const u16 *gr = Gs + r * p.OWp * GP;
      for (int kb = 0; kb < nk; ++kb) {
        s16x4 bfrag[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bfrag[nb] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(gr + bconst[nb] + kb * 16 * GP));
        s16x4 afrag[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if constexpr (CI >= 8) {
            afrag[j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(xr + aconst[j] + kb * 16 * S * PITCH));
          } else {
            const u16 *s = xr + aconst[j] + kb * 16;
            afrag[j] = s16x4{(short)s[0], (short)s[1], (short)s[2], (short)s[3]};
          }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[j][nb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(afrag[j], bfrag[nb], acc[j][nb], 0, 0, 0);
      }
    }
    if (more) {
      __syncthreads();                                       // every wave is done with this unit's rows
      commit_x(nf);
      commit_g(u + 1, ng);
    }
  }

  // ---- one partial slab per workgroup
  float *slab = p.slabs + (int64_t)blockIdx.x * p.slab_stride;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int mt = wave + j * WPN;
    if (mt < MT) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int co = nb * 16 + m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mt * 16 + g4 * 4 + r;            // C/D map: row = 4*(lane>>4)+reg, col = lane&15
          if (row < ROWS && co < CO) slab[(int64_t)row * CO + co] = acc[j][nb][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host
// Rows per band for output rows of OW pixels: the largest band (<= 16 rows) whose rows fit the loaders' prefetch registers
// and the LDS; 0 when not even a band of one row fits.
template <int CI, int CO, int K, int S, int PFX, int PFG>
int band_rows(int OW, int OH, size_t *lds_bytes) {
  constexpr int PITCH = CI >= 8 ? (CI <= 16 ? CI : CI + 4) : 1, GP = CO <= 16 ? CO : CO + 4, CPX = CI >= 8 ? CI / 8 : 1, CPG = CO / 8;
  const int OWp = (OW + 15) & ~15, colsR = (OW - 1) * S + K, colsA = (OWp - 1) * S + K + 4;
  int TY = 0;
  for (int ty = 1; ty <= 16 && ty <= OH; ++ty) {
    const int rows = (ty - 1) * S + K;
    const size_t xel = (((size_t)rows * colsA * PITCH) + 7) & ~(size_t)7, gel = (size_t)ty * OWp * GP + 16;
    const size_t bytes = ((xel + gel) * 2 + 15) & ~(size_t)15;
    // two workgroups per CU (<= 72 KB each) where the rows allow; a single row may take up to 120 KB
    if ((size_t)rows * colsR * CPX > (size_t)PFX * 256 || (size_t)ty * OW * CPG > (size_t)PFG * 256 ||
        bytes > (ty == 1 ? 120 : 72) * 1024) break;
    TY = ty; *lds_bytes = bytes;
  }
  return TY;
}

// One launch over output rows of p.OW pixels.  nseg: the number of column segments the row was cut into (run(), below);
// the segments share the workgroup budget.
template <int CI, int CO, int K, int S, int PFX, int PFG>
int run_seg(Dev p, int N, int max_slabs, int nseg, hipStream_t st, bool dry, int *nslab_out, char *name, int name_len) {
  constexpr int NTAP = K * K;
  p.OWp = (p.OW + 15) & ~15;
  p.colsR = (p.OW - 1) * S + K;
  p.colsA = (p.OWp - 1) * S + K + 4;                      // the last k-block reads up to OWp pixels (+ C_in == 1: 4-pixel reads)
  size_t lds_bytes = 0;
  const int TY = band_rows<CI, CO, K, S, PFX, PFG>(p.OW, p.OH, &lds_bytes);
  if (TY < 1) return TEM_EUNSUPPORTED;
  p.TY = TY; p.rows = (TY - 1) * S + K;
  p.nband = (p.OH + TY - 1) / TY;
  p.units = N * p.nband;
  // workgroup budget as in bww_bf16.hip: every workgroup costs a slab that tem_reduce_slabs_multi reads again
  const bool small_slab = NTAP * CI * CO * 4 <= 32 * 1024;
  int want = (small_slab ? 256 : 128) / nseg;
  if (want < 1) want = 1;
  if (want > max_slabs) want = max_slabs;
  p.per = (p.units + want - 1) / want;
  const int nblocks = (p.units + p.per - 1) / p.per;
  if (nblocks > max_slabs) return TEM_EUNSUPPORTED;
  if (nslab_out) *nslab_out = nblocks;
  p.magicColsR = magic_for(p.colsR);
  p.magicOW = magic_for(p.OW);
  if (dry) {
    if (name) snprintf(name, name_len, "bww2d_bf16_k<%d, %d, %d, %d, %d, %d>", CI, CO, K, S, PFX, PFG);
    return TEM_OK;
  }
  if (tem_debug_flags() & 8)
    fprintf(stderr, "bww2d_bf16<%d,%d,%d,%d> O=%dx%d P=%d: TY=%d units=%d per=%d blocks=%d lds=%zu\n", CI, CO, K, S, p.OH,
            p.OW, p.P, p.TY, p.units, p.per, nblocks, lds_bytes);
  auto kern = bww2d_bf16_k<CI, CO, K, S, PFX, PFG>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(256), lds_bytes, st, p);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

// A row that fits one band is one launch.  A wider row (pad 0 only: the 260 model's layers) is cut into column segments of a
// multiple of 16 output pixels, as in bww_bf16.hip: one launch per segment on the offset views, each into its own slab range.
template <int CI, int CO, int K, int S, int PFX, int PFG>
int run(Dev p, int N, int max_slabs, hipStream_t st, bool dry, int *nslab_out, char *name, int name_len) {
  size_t unused = 0;
  if (p.OW < 1 || band_rows<CI, CO, K, S, PFX, PFG>(p.OW, 1, &unused) >= 1)
    return run_seg<CI, CO, K, S, PFX, PFG>(p, N, max_slabs, 1, st, dry, nslab_out, name, name_len);
  if (p.P != 0) return TEM_EUNSUPPORTED;                   // the zero frame of a padded row belongs to its first and last segment only
  int seg = p.OW & ~15;
  while (seg >= 16 && band_rows<CI, CO, K, S, PFX, PFG>(seg, 1, &unused) < 1) seg -= 16;
  if (seg < 16) return TEM_EUNSUPPORTED;
  const int nseg = (p.OW + seg - 1) / seg;
  seg = ((p.OW + nseg - 1) / nseg + 15) & ~15;             // equal segments, not one sliver at the end
  int total = 0;
  for (int x0 = 0; x0 < p.OW; x0 += seg) {
    Dev q = p;
    q.in0 += (int64_t)x0 * S * p.i0W; q.in1 += (int64_t)x0 * S * p.i1W; q.g += (int64_t)x0 * p.gW;
    q.W = p.W - x0 * S;
    q.OW = p.OW - x0 < seg ? p.OW - x0 : seg;
    if (p.slabs) q.slabs = p.slabs + (int64_t)total * p.slab_stride;
    if (max_slabs - total < 1) return TEM_EUNSUPPORTED;
    int n = 0;
    const int rc = run_seg<CI, CO, K, S, PFX, PFG>(q, N, max_slabs - total, nseg, st, dry, &n, name, name_len);
    if (rc != TEM_OK) return rc;
    total += n;
  }
  if (nslab_out) *nslab_out = total;
  return TEM_OK;
}

}  // namespace bww2d_bf16

// 2-D geometry (kd = sd = 1, pd = 0, kh = kw in {3, 4}, sh = sw, ph = pw, depth-1 views): bww2d_bf16_k.
// TEM_EUNSUPPORTED for every other geometry (the caller goes on to the 3-D kernels).
int tem_bww2d_bf16_try(const tem_bww_args *a, hipStream_t st, bool dry, int *nslab_out, char *name, int name_len) {
  using namespace bww2d_bf16;
  const tem_view &i0 = a->in0, &g = a->dout;
  if (!(a->kd == 1 && a->sd == 1 && a->pd == 0 && a->kh > 1 && a->kh == a->kw && a->sh == a->sw && a->ph == a->pw))
    return TEM_EUNSUPPORTED;
  if (i0.D != 1 || g.D != 1) return TEM_EUNSUPPORTED;
  if (g.N != i0.N) return TEM_ESHAPE;
  auto U = as_u16;
  auto al16 = [](const tem_view &v) { return v.C % 8 != 0 || aligned(v, 8, false); };     // 16-byte channel chunks: 8 bf16
  if (!fits32(i0) || !fits32(g) || !al16(i0) || !al16(g) || g.C % 8) return TEM_EUNSUPPORTED;
  Dev p{};
  p.in0 = U(i0.ptr); p.i0N = (int)i0.sN; p.i0H = (int)i0.sH; p.i0W = (int)i0.sW; p.C0 = i0.C;
  p.in1 = p.in0; p.i1N = p.i0N; p.i1H = p.i0H; p.i1W = p.i0W;
  int CI = i0.C;
  if (a->in1.ptr) {
    const tem_view &i1 = a->in1;
    if (i1.N != i0.N || i1.D != i0.D || i1.H != i0.H || i1.W != i0.W) return TEM_ESHAPE;
    if (!fits32(i1) || !al16(i1) || i0.C % 8 || i1.C % 8) return TEM_EUNSUPPORTED;
    p.in1 = U(i1.ptr); p.i1N = (int)i1.sN; p.i1H = (int)i1.sH; p.i1W = (int)i1.sW;
    CI += i1.C;
  }
  p.H = i0.H; p.W = i0.W;
  p.g = U(g.ptr); p.gN = (int)g.sN; p.gH = (int)g.sH; p.gW = (int)g.sW;
  p.OH = g.H; p.OW = g.W; p.P = a->ph;
  p.slabs = a->slabs;
  const int CO = g.C, K = a->kh, S = a->sh, N = i0.N;
  p.slab_stride = a->slab_stride ? a->slab_stride : (int64_t)K * K * CI * CO;
  const int max_slabs = a->nslab;
#define BW2(ci, co, k, s, pfx, pfg) \
  if (CI == ci && CO == co && K == k && S == s) return run<ci, co, k, s, pfx, pfg>(p, N, max_slabs, st, dry, nslab_out, name, name_len);
  //   CI  CO  K  S  X-chunks  G-chunks (per thread)
  BW2(1, 8, 3, 1, 8, 8)   BW2(1, 16, 3, 1, 8, 8)
  BW2(8, 8, 3, 1, 8, 8)   BW2(8, 16, 3, 1, 8, 8)   BW2(16, 8, 3, 1, 8, 8)  BW2(16, 16, 3, 1, 8, 8)
  BW2(16, 32, 3, 1, 8, 8) BW2(32, 16, 3, 1, 8, 8)  BW2(32, 32, 3, 1, 8, 8)
  BW2(8, 8, 4, 2, 8, 8)   BW2(16, 16, 4, 2, 8, 8)  BW2(8, 16, 4, 2, 8, 8)  BW2(16, 32, 4, 2, 8, 8)
  BW2(32, 32, 4, 2, 8, 8)
#undef BW2
  return TEM_EUNSUPPORTED;
}
