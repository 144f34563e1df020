// convT2d_bf16.hip -- 2-D transposed convolution k4 s2 for the bf16 mixed-precision mode: the 2-D twin of
// convT_bf16.hip (forward of the generators' Conv2DTranspose layers with Dropout, and the input-gradient of every
// k4 s2 VALID convolution with the skip-gradient add and LeakyReLU' gate), bf16 operands, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16, bf16 stores.  Views are (N, 1, H, W, C).
//
//   out[o][co] = sum over (j, t) with o = 2 j + t - p of in[j][ci] * w[t][co][ci]            (per axis)
//
// Per axis o + p = 2 Q + r (parity class r): the taps reaching o are t = r + 2 c, c in {0, 1}, from j = Q - c.  The
// four (r_y, r_x) classes of one Q read the same 2x2 input neighbourhood, so for a fixed r_y the operator is a GEMM
//
//   D[Q voxels][(r_x, co)] = sum_{(c_y, c_x, ci)} X[Q - c][ci] * B[(c, ci)][(r_x, co)],   K = 4 C_in,
//
// with the two x-classes side by side in N (one contiguous 2*C_out run of two adjacent output voxels).  C_in = 8 is
// exactly one k-step.  A workgroup owns (n, a band of Q_y rows) and runs BOTH r_y classes over one LDS patch (their B
// fragments stay in registers); tiles of 16 Q voxels run across row ends.  Dropout keep bits follow the fp32 2-D path:
// drawn in the epilogue (keep_mode 1 writes the mask), read back by the backward (keep_mode 2).
#include "bf16_common.h"
#include <cstdio>
#include <cstdlib>

namespace convt2d_bf16 {

using namespace tem_bf16;

struct Ep {
  float slope;
  const u16 *gate; int32_t gN, gH, gW; float gate_slope;
  const u16 *add;  int32_t aN, aH, aW, aoy, aox, aHh, aWw;
  int32_t dropout;
  DropoutStream ds;
  const uint32_t *step_dev;
  int32_t doz, doy, dox, dD, dH, dW;
  uint8_t *keep_mask;
  int32_t keep_mode;
  int32_t gbytes, abytes, mbytes;                // extents (bytes) of the gate / add views and of the keep mask: buffer ranges
};

struct Dev {
  const u16 *in;
  int32_t iN, iH, iW, H, W;
  u16 *out;
  int32_t oN, oH, oW, OH, OW;
  int32_t P;
  int32_t Qlo_x, nQx, Qlo_y, nQy;              // Q ranges (union over the parity classes)
  int32_t TY, nband;                           // Q_y rows per workgroup, bands
  int32_t cols, rows;                          // patch extents (voxels): nQx + 1, TY + 1
  uint32_t magicQx, magicCols;
  Ep ep;
};

// EPM: compiled epilogue -- 0: run-time flags (forward with Dropout); 2: input-gradient (gate, optional skip-gradient
// add, no Dropout)
template <int CI, int CO, int PF, int EPM>
__global__ __launch_bounds__(256) void convT2d_bf16_k(Dev p, const u16 *__restrict__ wgt) {
  constexpr int NT = 2 * CO / 16;                 // n-tiles over the columns (r_x, co)
  constexpr int WPN = 4 / NT;                     // waves per n-tile (tile subsets)
  constexpr int NSTEP = 4 * CI / 32;              // k-steps of 32: k = (tap4, ci), a lane's 8 k-values = 8 channels of one tap
  constexpr int CPV = CI / 8;                     // 16-byte chunks per voxel
  constexpr int TPITCH = 20;
  static_assert(NT == 1 || NT == 2 || NT == 4, "C_out in {8, 16, 32}");
  static_assert(CI % 8 == 0 && NSTEP >= 1, "C_in a multiple of 8");
  extern __shared__ __attribute__((aligned(16))) u16 lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kq = lane >> 4;

  int b = (int)xcd_contiguous_block(blockIdx.x, gridDim.x);     // neighbouring bands share a halo row: one L2
  const int band = b % p.nband;
  const int n = b / p.nband;
  const int Qy0 = p.Qlo_y + band * p.TY;
  const int nrow = min(p.TY, p.nQy - band * p.TY);             // Q_y rows of this band

  // ---- B fragments of this wave's n-tile for both r_y classes: k-step st multiplies channels c0 .. c0+7 of input
  // voxel Q - (c_y, c_x), tap4 = (c_y, c_x)
  const int nt = wave % NT;
  const int ncol = nt * 16 + m;                   // column (r_x, co)
  const int rx = ncol / CO, co = ncol - rx * CO;
  bf16x8 B[2][NSTEP];
#pragma unroll
  for (int ry = 0; ry < 2; ++ry) {
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
      const int e0 = 32 * st + 8 * kq, tap4 = e0 / CI, c0 = e0 - tap4 * CI;
      const int cy = tap4 >> 1, cx = tap4 & 1;
      const int tap = (ry + 2 * cy) * 4 + (rx + 2 * cx);
      B[ry][st] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(wgt + ((tap * CO + co) * CI + c0)));
    }
  }

  // ---- input patch: rows j_y = Qy0-1 .. Qy0+nrow-1; cols j_x = Qlo_x-1 .. Qlo_x+nQx-1
  {
    const int total = (nrow + 1) * p.cols * CPV;
    uint4 pf[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int id = tid + i * 256;
      const int vox = id / CPV, c = (id - vox * CPV) * 8;
      const int r = (int)__umulhi((uint32_t)vox, p.magicCols), cx = vox - r * p.cols;
      const int jy = Qy0 - 1 + r, jx = p.Qlo_x - 1 + cx;
      const bool ok = id < total && (unsigned)jy < (unsigned)p.H && (unsigned)jx < (unsigned)p.W;
      pf[i] = ok ? *reinterpret_cast<const uint4 *>(p.in + (n * p.iN + jy * p.iH + jx * p.iW + c))
                 : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int id = tid + i * 256;
      if (id < total) {
        const int vox = id / CPV, c = (id - vox * CPV) * 8;
        *reinterpret_cast<uint4 *>(lds + vox * CI + c) = pf[i];   // 16-byte aligned: CI and c are multiples of 8
      }
    }
  }
  __syncthreads();

  // A gather: k-step st, lane group kq -> tap4 = (c_y, c_x), first channel c0: voxel (row qy + 1 - cy, col qx + 1 - cx)
  int aoff[NSTEP];
#pragma unroll
  for (int st = 0; st < NSTEP; ++st) {
    const int e0 = 32 * st + 8 * kq, tap4 = e0 / CI, c0 = e0 - tap4 * CI;
    const int cy = tap4 >> 1, cx = tap4 & 1;
    aoff[st] = ((1 - cy) * p.cols + (1 - cx)) * CI + c0;
  }
  const int padded = (p.rows * p.cols * CI + 7) & ~7;         // bf16 elements; 16-byte aligned
  float *tp = reinterpret_cast<float *>(lds + padded) + wave * (16 * TPITCH);
  const int ti = lane >> 2, tcq = lane & 3;                   // transposed role: Q voxel of the tile, column quad
  const int ecol = nt * 16 + tcq * 4;                         // first of this lane's 4 columns
  const int erx = ecol / CO, eco = ecol - erx * CO;
  const int L = nrow * p.nQx;                                 // linearised Q voxels of the band
  const int ntiles = (L + 15) >> 4;
  const Ep &ep = p.ep;
  DropoutStream ds = ep.ds;
  if (ep.dropout && ep.step_dev) ds.step = *ep.step_dev;

  auto a_base = [&](int t) -> const u16 * {
    const int v = min(t * 16 + m, L - 1);                     // lanes past the band recompute its last voxel, never stored
    const int qy = p.nQx == 1 ? v : (int)__umulhi((uint32_t)v, p.magicQx), qx = v - qy * p.nQx;
    return lds + (qy * p.cols + qx) * CI;
  };
  // epilogue in two halves (see convT_bf16.hip): `prep` issues the gate / skip-gradient / keep-byte loads ahead of the
  // tile's MFMA chain, `finish` consumes them
  const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void *)ep.gate, 0, ep.gate ? ep.gbytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc((void *)ep.add, 0, ep.add ? ep.abytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc((void *)ep.keep_mask, 0, ep.keep_mode == 2 ? ep.mbytes : 0, 0x00020000);
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  struct Prep { int oy, ox; bool valid; uint2 g4, a4; uint32_t kb; };
  auto drop_elem = [&](int oy, int ox) -> uint64_t {
    return ((((uint64_t)n * ep.dD + ep.doz) * ep.dH + (oy + ep.doy)) * ep.dW + (ox + ep.dox)) * (uint64_t)CO + eco;
  };
  auto prep = [&](int t, int ry) -> Prep {
    Prep q;
    const int v = t * 16 + ti;
    const int qy = p.nQx == 1 ? v : (int)__umulhi((uint32_t)v, p.magicQx), qx = v - qy * p.nQx;
    q.oy = 2 * (Qy0 + qy) + ry - p.P; q.ox = 2 * (p.Qlo_x + qx) + erx - p.P;
    q.valid = v < L && (unsigned)q.oy < (unsigned)p.OH && (unsigned)q.ox < (unsigned)p.OW;
    int goff = q.valid ? (n * ep.gN + q.oy * ep.gH + q.ox * ep.gW + eco) * 2 : (int)0x80000000;
    asm volatile("" : "+v"(goff));
    const u32x2 g = __builtin_amdgcn_raw_buffer_load_b64(grs, goff, 0, 0);
    q.g4 = make_uint2(g.x, g.y);
    const int ay = q.oy - ep.aoy, ax = q.ox - ep.aox;
    const bool ain = q.valid && (unsigned)ay < (unsigned)ep.aHh && (unsigned)ax < (unsigned)ep.aWw;
    int aoff2 = ain ? (n * ep.aN + ay * ep.aH + ax * ep.aW + eco) * 2 : (int)0x80000000;
    asm volatile("" : "+v"(aoff2));
    const u32x2 a = __builtin_amdgcn_raw_buffer_load_b64(ars, aoff2, 0, 0);
    q.a4 = make_uint2(a.x, a.y);
    q.kb = 0;
    if (EPM != 2) {
      int moff = q.valid ? (int)(uint32_t)(drop_elem(q.oy, q.ox) >> 3) : (int)0x80000000;
      asm volatile("" : "+v"(moff));
      q.kb = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(mrs, moff, 0, 0);
    }
    return q;
  };
  auto finish = [&](const f32x4 &acc, const Prep &q) {
#pragma unroll
    for (int r = 0; r < 4; ++r) tp[(kq * 4 + r) * TPITCH + m] = acc[r];
    __builtin_amdgcn_s_waitcnt(0xc07f);                       // lgkmcnt(0): this wave's own LDS writes have landed
    const float4 v4 = *reinterpret_cast<const float4 *>(tp + ti * TPITCH + tcq * 4);
    const int oy = q.oy, ox = q.ox;
    const bool valid = q.valid;
    float vv[4] = {v4.x + bf2f((u16)(q.a4.x & 0xffffu)), v4.y + bf2f((u16)(q.a4.x >> 16)),
                   v4.z + bf2f((u16)(q.a4.y & 0xffffu)), v4.w + bf2f((u16)(q.a4.y >> 16))};
    if (EPM == 2 || ep.gate) {
      vv[0] = bf2f((u16)(q.g4.x & 0xffffu)) > 0.f ? vv[0] : ep.gate_slope * vv[0];
      vv[1] = bf2f((u16)(q.g4.x >> 16)) > 0.f ? vv[1] : ep.gate_slope * vv[1];
      vv[2] = bf2f((u16)(q.g4.y & 0xffffu)) > 0.f ? vv[2] : ep.gate_slope * vv[2];
      vv[3] = bf2f((u16)(q.g4.y >> 16)) > 0.f ? vv[3] : ep.gate_slope * vv[3];
    }
    if (EPM == 0 && ep.dropout) {                             // kernel-uniform
      const uint64_t e = drop_elem(oy, ox);
      uint32_t bits;
      if (ep.keep_mode == 2) {
        bits = (q.kb >> (uint32_t)(e & 4u)) & 15u;              // (fetched by prep; zero for lanes without a voxel)
      } else {
        const Philox128 ph = ds.block(e >> 7);
        const uint32_t eb = (uint32_t)(e & 127);
        bits = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) bits |= (DropoutStream::bit(ph, eb + c) ? 1u : 0u) << c;
        if (ep.keep_mode == 1) {
          // a byte of the mask = the 8 channels eco&~7 .. +7 of one voxel = this lane's nibble and its neighbour's
          const uint32_t other = (uint32_t)__shfl_xor((int)bits, 1, 64);
          if (valid && !(tcq & 1)) ep.keep_mask[e >> 3] = (uint8_t)(bits | (other << 4));
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) vv[c] = ((bits >> c) & 1u) ? 2.f * vv[c] : 0.f;
    }
    if (valid) {
      if (ep.slope != 1.f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) vv[c] = vv[c] > 0.f ? vv[c] : ep.slope * vv[c];
      }
      *reinterpret_cast<uint2 *>(p.out + (n * p.oN + oy * p.oH + ox * p.oW + eco)) =
          make_uint2(f2bf(vv[0]) | ((uint32_t)f2bf(vv[1]) << 16), f2bf(vv[2]) | ((uint32_t)f2bf(vv[3]) << 16));
    }
  };

  // two tiles per iteration (independent accumulator chains interleave)
#pragma unroll
  for (int ry = 0; ry < 2; ++ry) {
    for (int t = wave / NT; t < ntiles; t += 2 * WPN) {       // wave-uniform
      const int t2 = t + WPN;
      const bool two = t2 < ntiles;
      const u16 *s0 = a_base(t), *s1 = a_base(two ? t2 : t);
      const Prep q0 = prep(t, ry), q1 = prep(two ? t2 : t, ry);
      f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        const bf16x8 a0 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(s0 + aoff[st]));
        const bf16x8 a1 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(s1 + aoff[st]));
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, B[ry][st], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, B[ry][st], acc1, 0, 0, 0);
      }
      finish(acc0, q0);
      if (two) finish(acc1, q1);
    }
  }
}

// ------------------------------------------------------------------------------------------ host
constexpr int LDS_MAX = 64 * 1024;

template <int CI, int CO, int PF>
int run(Dev p, int N, const u16 *w, hipStream_t st, bool dry, int epm, char *name, int name_len) {
  constexpr int CPV = CI / 8;
  constexpr size_t TP_BYTES = 4 * 16 * 20 * 4;
  // o + P = 2Q + r  =>  Q in [floor(P/2), floor((O-1+P)/2)]
  p.Qlo_x = floordiv2(p.P); p.nQx = floordiv2(p.OW - 1 + p.P) - p.Qlo_x + 1;
  p.Qlo_y = floordiv2(p.P); p.nQy = floordiv2(p.OH - 1 + p.P) - p.Qlo_y + 1;
  if (p.nQx < 1 || p.nQy < 1) return TEM_ESHAPE;
  p.cols = p.nQx + 1;
  // rows per band: as many as the loader's registers and the LDS budget allow, up to ~16 tiles per class, and at least
  // ~2 workgroups per CU when the launch has the rows for it
  int TY = 0;
  for (int ty = 1; ty <= p.nQy && ty <= 64; ++ty) {
    const size_t chunks = (size_t)(ty + 1) * p.cols * CPV;
    const size_t bytes = (size_t)(ty + 1) * p.cols * CI * 2 + 16 + TP_BYTES;
    if (chunks > (size_t)PF * 256 || bytes > LDS_MAX) break;
    if (ty > 1 && (size_t)N * ((p.nQy + ty - 1) / ty) < 512) break;
    TY = ty;
    if ((ty * p.nQx + 15) / 16 >= 16) break;
  }
  if (TY < 1) return TEM_EUNSUPPORTED;
  p.TY = TY; p.rows = TY + 1;
  p.nband = (p.nQy + TY - 1) / TY;
  p.magicQx = magic_for(p.nQx);
  p.magicCols = magic_for(p.cols);
  if (dry) {
    if (name) snprintf(name, name_len, "convT2d_bf16_k<%d, %d, %d, %d>", CI, CO, PF, epm);
    return TEM_OK;
  }
  const size_t lds_bytes = (((size_t)p.rows * p.cols * CI + 7) & ~(size_t)7) * 2 + TP_BYTES;
  const int nblocks = N * p.nband;
  if (tem_debug_flags() & 8)
    fprintf(stderr, "convT2d_bf16<%d,%d> O=%dx%d P=%d: nQ=%dx%d TY=%d bands=%d blocks=%d lds=%zu\n", CI, CO, p.OH, p.OW,
            p.P, p.nQy, p.nQx, p.TY, p.nband, nblocks, lds_bytes);
  if (epm == 2) hipLaunchKernelGGL((convT2d_bf16_k<CI, CO, PF, 2>), dim3((unsigned)nblocks), dim3(256), lds_bytes, st, p, w);
  else hipLaunchKernelGGL((convT2d_bf16_k<CI, CO, PF, 0>), dim3((unsigned)nblocks), dim3(256), lds_bytes, st, p, w);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

}  // namespace convt2d_bf16

// 2-D geometry (kd = sd = 1, pd = 0, kh = kw = 4, sh = sw = 2, ph = pw, depth-1 views): convT2d_bf16_k.
// TEM_EUNSUPPORTED for every other geometry (the caller goes on to the 3-D kernel).
int tem_conv_transpose2d_bf16_try(const tem_conv_args *a, hipStream_t st, bool dry, char *name, int name_len) {
  using namespace convt2d_bf16;
  const tem_view &i0 = a->in0, &o0 = a->out0;
  if (!(a->kd == 1 && a->sd == 1 && a->pd == 0 && a->kh == 4 && a->kw == 4 && a->sh == 2 && a->sw == 2 && a->ph == a->pw))
    return TEM_EUNSUPPORTED;
  if (i0.D != 1 || o0.D != 1) return TEM_EUNSUPPORTED;
  if (a->in1.ptr || a->out1.ptr || a->ep.bias) return TEM_EUNSUPPORTED;
  if (o0.N != i0.N) return TEM_ESHAPE;
  if (!fits32(i0) || !fits32(o0)) return TEM_EUNSUPPORTED;
  auto U = as_u16;
  if (!aligned(i0, 8, false) || !aligned(o0, 4, false)) return TEM_EUNSUPPORTED;     // 16-byte input chunks, 8-byte stores
  Dev p{};
  p.in = U(i0.ptr); p.iN = (int)i0.sN; p.iH = (int)i0.sH; p.iW = (int)i0.sW;
  p.H = i0.H; p.W = i0.W;
  p.out = const_cast<u16 *>(U(o0.ptr)); p.oN = (int)o0.sN; p.oH = (int)o0.sH; p.oW = (int)o0.sW;
  p.OH = o0.H; p.OW = o0.W;
  p.P = a->ph;
  if (const int rc = fill_epilogue<false, false>(p.ep, a->ep, o0)) return rc;
  const int CI = i0.C, CO = o0.C, N = i0.N;
  const int epm = (!p.ep.dropout && p.ep.gate) ? 2 : 0;
#define CT_CASE(ci, co, pf) if (CI == ci && CO == co) return run<ci, co, pf>(p, N, U(a->w), st, dry, epm, name, name_len);
  CT_CASE(16, 8, 12)     // g.u1b forward (Conv2DTranspose 16 -> 8, Dropout)
  CT_CASE(32, 16, 12)    // g.u2b forward
  CT_CASE(8, 8, 12)      // input-gradient of g.d1b
  CT_CASE(16, 16, 12)    // input-gradient of g.d2b
  CT_CASE(32, 32, 12)    // input-gradient of d.d2b / d.d3b
#undef CT_CASE
  return TEM_EUNSUPPORTED;
}
