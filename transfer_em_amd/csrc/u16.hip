// u16.hip -- the first link of the preparation chain: 16-bit volumes (uint16, or int16 with the sign bit flipped, so
// that the index u = v ^ 0x8000 keeps the order) counted and brought to uint8 by a table.
//   tem_u16_hist           counts[u] += occurrences of index u inside a box of a dense 16-bit block (one histogram of
//                          65,536 bins, or one per section)
//   tem_u16_lut_u8         dst[i] = lut[u(src[i])] (one table of 65,536 bytes, or one per section), the table staged
//   tem_u16_lut_u8_direct  in LDS / read straight from global memory (the same bytes; the timing tool holds both)
//
// tem_u16_hist.  65,536 32-bit counters are 256 KiB and a CU has 160 KiB of LDS, so the table is split by the high bit
// of u over two CLASSES of workgroups (blockIdx.y), tem_u8_hist2's form: a class-c workgroup of 1024 threads walks all
// voxels of its run of rows and counts those with u >> 15 == c into 32,768 private counters (128 KiB, one workgroup per
// CU), indexed u & 32767.  Every voxel is counted once, by its class; the bytes are read twice, the second time mostly
// out of L2 / Infinity Cache.  The counters are shared by all lanes (ds_add_u32): lanes of one instruction that hit one
// counter are served one after the other, so a constant block is the slow case -- and an exact one.  A counter sees at
// most the voxels its workgroup walks between two flushes, which the entry point keeps below 2^31.
// Flush: thread t walks counters t, t + 1024, ... and adds every non-zero one with ONE 64-bit global atomic add.
// Loads: the work item is a 16-byte-ADDRESS-aligned segment of a row (8 voxels); a segment wholly inside the row
// travels as one dwordx4, the (at most two) cut segments of a row voxel by voxel.  Nothing outside the box is read.
//
// Dealing.  The rows of the box, in (z, y) order, form nsec stretches that must be flushed apart: the sections with
// per_section, else the one whole box.  A stretch is cut into pps PIECES of rpp rows (the last may be shorter), and a
// workgroup takes ppw consecutive pieces; it flushes where its run leaves a stretch and at its end.  Why not
// tem_u8_hist's equal runs of rows: there a flush is 256 counters, here it is 32,768 LDS reads, 32,768 clears and an
// atomic per occupied bin, so a run boundary that falls inside a small section makes two workgroups pay a whole flush
// for a part of a section each.  With pieces no section is flushed more often than it is cut: a section of fewer than
// HIST16_ITEMS_PER_PIECE segments (32,768 voxels, one per counter) is never cut, whole small sections are chained in
// one workgroup (one flush each, the least a table per section allows), and a large section is cut only as far as
// HIST16_MAX_PARTS workgroups per class need it: pps = min(ceil(segments / 4096), max(1, 128 / nsec)).
#include "tem_common.h"

namespace {

constexpr int HIST16_THREADS = 1024;
constexpr int HIST16_BINS = 32768;             // per class
constexpr int HIST16_MAX_PARTS = 128;          // x 2 classes = one workgroup on each of 256 CUs
constexpr int HIST16_ITEMS_PER_PIECE = 4096;   // segments: 32,768 voxels, as many as a flush walks counters

__device__ __forceinline__ void hist16_add(uint32_t *h, uint32_t u, uint32_t cls) {
  if ((u >> 15) == cls) atomicAdd(&h[u & 32767u], 1u);
}

// every non-zero counter -> counts[i]; `clear` leaves the counters zero for the next run
__device__ __forceinline__ void hist16_flush(uint32_t *h, uint64_t *counts, bool clear) {
  __syncthreads();
  for (int i = threadIdx.x; i < HIST16_BINS; i += HIST16_THREADS) {
    const uint32_t c = h[i];
    if (c) {
      atomicAdd(reinterpret_cast<unsigned long long *>(counts + i), (unsigned long long)c);
      if (clear) h[i] = 0;
    }
  }
  if (clear) __syncthreads();
}

// first row of piece q: stretch q / pps, its piece q % pps (nyd rows per stretch, rpp per piece)
__device__ __forceinline__ int64_t hist16_row(int64_t q, int64_t pps, int64_t rpp, int64_t nyd) {
  const int64_t sec = q / pps;
  return sec * nyd + min((q - sec * pps) * rpp, nyd);
}

// src: the box's first voxel (z0, y0, x0).  Row r = zi * ny + yi of the box starts at src + (zi * H + yi) * W voxels.
// S: segments per row, an upper bound of ceil(((address of the row & 15) + 2 width) / 16) over all (even) alignments;
// magicS = magic_for(S).  flip: 0x8000 for int16 voxels.
__global__ __launch_bounds__(HIST16_THREADS) void u16_hist_k(const uint16_t *src, int64_t H, int64_t W, int ny, int width,
                                                             int64_t nrows, int64_t npieces, int64_t pps, int64_t rpp,
                                                             int64_t ppw, uint32_t S, uint32_t magicS, uint64_t *counts,
                                                             int per_section, uint32_t flip) {
  __shared__ uint32_t h[HIST16_BINS];
  for (int i = threadIdx.x; i < HIST16_BINS; i += HIST16_THREADS) h[i] = 0;
  __syncthreads();
  const uint32_t cls = blockIdx.y;
  const int64_t nyd = per_section ? (int64_t)ny : nrows;
  const int64_t q0 = (int64_t)blockIdx.x * ppw, q1 = min(q0 + ppw, npieces);
  int64_t r0 = hist16_row(q0, pps, rpp, nyd);
  const int64_t r1 = hist16_row(q1, pps, rpp, nyd);
  uint64_t *dst = counts + (int64_t)cls * HIST16_BINS;
  while (r0 < r1) {
    const int64_t zi = r0 / ny;
    const uint32_t y00 = (uint32_t)(r0 - zi * ny);                       // the run starts at row y00 of section zi
    const int64_t rend = per_section ? min(r1, (zi + 1) * ny) : r1;
    const uint32_t total = (uint32_t)(rend - r0) * S;                    // < 2^31: the entry point's bound
    for (uint32_t i = threadIdx.x; i < total; i += HIST16_THREADS) {
      // floor(i / S), exactly: the magic product is floor(i / S) or one above it for every i < 2^31 (tem_u8_hist2)
      uint32_t ri = S == 1 ? i : __umulhi(i, magicS);
      if (ri * S > i) --ri;                                              // ri S <= i + S < 2^32
      const uint32_t s = i - ri * S;
      const uint32_t yy = y00 + ri, dz = yy / (uint32_t)ny, y = yy - dz * (uint32_t)ny;   // y00, ri < 2^31
      const uint16_t *row = src + ((zi + dz) * H + y) * W;
      const int64_t m = (int64_t)(((uintptr_t)row & 15) >> 1);           // the row starts m voxels into a 16-byte line
      const int64_t lo = max((int64_t)8 * s - m, (int64_t)0), hi = min((int64_t)8 * s + 8 - m, (int64_t)width);
      if (hi - lo == 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + lo);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hist16_add(h, (w[j] & 0xffffu) ^ flip, cls);
          hist16_add(h, (w[j] >> 16) ^ flip, cls);
        }
      } else {
        for (int64_t x = lo; x < hi; ++x) hist16_add(h, (uint32_t)row[x] ^ flip, cls);
      }
    }
    r0 = rend;
    hist16_flush(h, dst + (per_section ? zi * 65536 : 0), r0 < r1);
  }
}

// ------------------------------------------------------------------------------------------------------- lut
constexpr int LUT16_THREADS = 1024;
constexpr int LUT16_MAX_GRID = 512;            // 2 workgroups of 64 KiB LDS on each of 256 CUs
constexpr int LUT16_ITEMS_PER_WG = 16384;      // 131,072 voxels: 256 KiB read and 128 KiB written per 64 KiB of table

// Block b: part b % pps of section b / pps (no per_section: one section, the whole block).  The work item is an
// 8-byte-ADDRESS-aligned group of dst (8 voxels): a group wholly inside the section leaves as one 8-byte store, its 16
// source bytes arrive as one dwordx4 where they are 16-byte aligned -- that is decided once per launch, by
// (src - 2 dst) & 15, and holds for two allocations -- and as 8 ushort loads otherwise; the section's first and last
// group go voxel by voxel where the section covers them only partly.  STAGED: the section's 64 KiB table is copied into
// LDS once per workgroup (4 dwordx4 per thread) and looked up there (ds_read_u8); else every lookup is a byte load from
// global memory.
template <bool STAGED>
__global__ __launch_bounds__(LUT16_THREADS) void u16_lut_u8_k(const uint16_t *src, uint8_t *dst, int64_t secvox,
                                                              const uint8_t *lut, int64_t zsec0, int per_section,
                                                              uint32_t pps, int64_t per, uint32_t flip) {
  __shared__ uint8_t staged[STAGED ? 65536 : 16];
  const int64_t sec = blockIdx.x / pps;
  const uint32_t part = blockIdx.x - (uint32_t)sec * pps;
  const uint8_t *t = lut + (per_section ? (zsec0 + sec) * 65536 : 0);
  if (STAGED) {
    if (((uintptr_t)t & 15) == 0) {
      for (int i = threadIdx.x; i < 4096; i += LUT16_THREADS)
        reinterpret_cast<uint4 *>(staged)[i] = reinterpret_cast<const uint4 *>(t)[i];
    } else {
      for (int i = threadIdx.x; i < 65536; i += LUT16_THREADS) staged[i] = t[i];
    }
    __syncthreads();
    t = staged;
  }
  const uint16_t *s0 = src + sec * secvox;
  uint8_t *d0 = dst + sec * secvox;
  const int m = (int)((uintptr_t)d0 & 7);
  const int64_t nitem = (m + secvox + 7) / 8;
  const int64_t i1 = min(nitem, (int64_t)(part + 1) * per);
  for (int64_t i = (int64_t)part * per + threadIdx.x; i < i1; i += LUT16_THREADS) {
    const int64_t lo = max(8 * i - m, (int64_t)0), hi = min(8 * i + 8 - m, secvox);
    if (hi - lo == 8) {
      const uint16_t *p = s0 + lo;
      uint32_t w[4];
      if (((uintptr_t)p & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (uint32_t)p[2 * j] | ((uint32_t)p[2 * j + 1] << 16);
      }
      uint32_t o[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        o[j] = (uint32_t)t[(w[2 * j] & 0xffffu) ^ flip] | ((uint32_t)t[(w[2 * j] >> 16) ^ flip] << 8) |
               ((uint32_t)t[(w[2 * j + 1] & 0xffffu) ^ flip] << 16) | ((uint32_t)t[(w[2 * j + 1] >> 16) ^ flip] << 24);
      *reinterpret_cast<uint2 *>(d0 + lo) = make_uint2(o[0], o[1]);
    } else {
      for (int64_t x = lo; x < hi; ++x) d0[x] = t[(uint32_t)s0[x] ^ flip];
    }
  }
}

template <bool STAGED>
int u16_lut_u8_launch(const uint16_t *src, int32_t D, int32_t H, int32_t W, uint8_t *dst, const uint8_t *lut,
                      int32_t per_section, int32_t zsec0, int32_t is_signed, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !dst || !lut || ((uintptr_t)src & 1) || D < 1 || H < 1 || W < 1 || zsec0 < 0 ||
      (per_section != 0 && per_section != 1) || (is_signed != 0 && is_signed != 1))
    return TEM_EINVAL;
  const int64_t nsec = per_section ? D : 1;
  const int64_t secvox = per_section ? (int64_t)H * W : (int64_t)D * H * W;
  const int64_t nitem = (secvox + 7 + 7) / 8;                            // groups of a section, any alignment
  // parts per section: LUT16_ITEMS_PER_WG groups per workgroup at least, about LUT16_MAX_GRID workgroups in all at most
  int64_t pps = (nitem + LUT16_ITEMS_PER_WG - 1) / LUT16_ITEMS_PER_WG, cap = (LUT16_MAX_GRID + nsec - 1) / nsec;
  pps = pps > cap ? cap : pps;
  const int64_t per = (nitem + pps - 1) / pps;
  pps = (nitem + per - 1) / per;
  if (nsec * pps > 0x7fffffff) return TEM_EINVAL;                        // more workgroups than one launch holds
  hipLaunchKernelGGL(u16_lut_u8_k<STAGED>, dim3((unsigned)(nsec * pps)), dim3(LUT16_THREADS), 0, (hipStream_t)stream, src,
                     dst, secvox, lut, (int64_t)zsec0, (int)per_section, (uint32_t)pps, per, is_signed ? 0x8000u : 0u);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

}  // namespace

extern "C" int tem_u16_hist(const uint16_t *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t z1, int32_t y0,
                            int32_t y1, int32_t x0, int32_t x1, uint64_t *counts, int32_t per_section, int32_t is_signed,
                            tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !counts || ((uintptr_t)src & 1) || ((uintptr_t)counts & 7) || D < 1 || H < 1 || W < 1 || z0 < 0 || z0 > z1 ||
      z1 > D || y0 < 0 || y0 > y1 || y1 > H || x0 < 0 || x0 > x1 || x1 > W || (per_section != 0 && per_section != 1) ||
      (is_signed != 0 && is_signed != 1))
    return TEM_EINVAL;
  const int64_t nz = z1 - z0, ny = y1 - y0, width = x1 - x0, nrows = nz * ny;
  if (nrows == 0 || width == 0) return TEM_OK;
  const int64_t S = (2 * width + 29) / 16;                               // segments per row, any (even) alignment
  const int64_t nsec = per_section ? nz : 1, nyd = per_section ? ny : nrows;
  const int64_t cap = nsec >= HIST16_MAX_PARTS ? 1 : HIST16_MAX_PARTS / nsec;
  const int64_t want = nyd >= (int64_t)HIST16_MAX_PARTS * HIST16_ITEMS_PER_PIECE
                           ? HIST16_MAX_PARTS
                           : (nyd * S + HIST16_ITEMS_PER_PIECE - 1) / HIST16_ITEMS_PER_PIECE;
  const int64_t pps0 = want < 1 ? 1 : (want > cap ? cap : want);
  const int64_t rpp = (nyd + pps0 - 1) / pps0;                           // rows per piece
  const int64_t pps = (nyd + rpp - 1) / rpp;                             // pieces per stretch, none empty
  const int64_t npieces = nsec * pps;
  const int64_t ppw = (npieces + HIST16_MAX_PARTS - 1) / HIST16_MAX_PARTS;   // above 1 only where pps == 1
  const int64_t parts = (npieces + ppw - 1) / ppw;
  // the 32-bit bound: a workgroup's counters and its item index both stay below 2^31 between two flushes
  if (rpp > (((int64_t)1 << 31) - 1) / (width > S ? width : S)) return TEM_EINVAL;
  const uint16_t *first = src + ((int64_t)z0 * H + y0) * W + x0;
  hipLaunchKernelGGL(u16_hist_k, dim3((unsigned)parts, 2), dim3(HIST16_THREADS), 0, (hipStream_t)stream, first, (int64_t)H,
                     (int64_t)W, (int)ny, (int)width, nrows, npieces, pps, rpp, ppw, (uint32_t)S, magic_for((int)S), counts,
                     (int)per_section, is_signed ? 0x8000u : 0u);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u16_lut_u8(const uint16_t *src, int32_t D, int32_t H, int32_t W, uint8_t *dst, const uint8_t *lut,
                              int32_t per_section, int32_t zsec0, int32_t is_signed, tem_stream_t stream) {
  return u16_lut_u8_launch<true>(src, D, H, W, dst, lut, per_section, zsec0, is_signed, stream);
}

extern "C" int tem_u16_lut_u8_direct(const uint16_t *src, int32_t D, int32_t H, int32_t W, uint8_t *dst, const uint8_t *lut,
                                     int32_t per_section, int32_t zsec0, int32_t is_signed, tem_stream_t stream) {
  return u16_lut_u8_launch<false>(src, D, H, W, dst, lut, per_section, zsec0, is_signed, stream);
}
