// hist_u8.hip -- the two byte kernels around tiled inference that look at intensities instead of moving them:
//   tem_u8_hist   counts[v] += occurrences of byte value v inside a box of a dense uint8 block (one histogram, or one
//                 per section)
//   tem_u8_lut    buf[i] = lut[buf[i]] in place (one table, or one per section)
// Both are one pass over the bytes.  The lut moves them at cache bandwidth; the histogram is bound by its 16 LDS adds
// per 16 bytes, not by the loads (figures in DESIGN.md).
//
// Rows are only as aligned as the caller's pointer, W and x0 allow, so both kernels cut their byte range at 16-byte
// ADDRESS boundaries: a segment that lies wholly inside the range travels as one dwordx4, the (at most two) cut
// segments of a row -- its head and its tail -- byte by byte, the valid bytes only.  Nothing outside the box (hist) or
// the buffer (lut) is read, and the lut writes exactly the bytes it read.
//
// tem_u8_hist.  The work is the box's rows in (z, y) order; a workgroup of 256 threads takes one contiguous run of
// them (the grid is capped at HIST_MAX_GRID workgroups, each loops) and spreads its threads over (row, segment) items,
// so that narrow rows still fill the lanes.  Counters are private to the workgroup: 32 copies of a 256-bin histogram
// of 32-bit counters in LDS, laid out [bin][copy], a lane adding into copy (lane & 31) with ds_add_u32.  The bank of
// counter (bin, copy) is (32 bin + copy) mod 32 = copy for every bin: the 32 lanes of a half wave always hit 32
// different banks, whatever the bytes are -- a constant image, the worst case of a shared histogram, costs what a
// random one does (lanes l and l + 32 share a counter, but the two halves of a wave are served in separate LDS cycles).
// One flush per run of rows: thread t sums the 32 copies of bin t (walking them from copy t & 31 on, so that the
// reads are conflict-free as well) in 64 bits and adds the sum with ONE 64-bit global atomic add (an ordinary vector
// atomic; zero sums are skipped: EM data fills a few dozen bins).  With per_section a run is cut where the section
// changes: the workgroup flushes into that section's row of counts, clears its copies and goes on.
// A 32-bit counter cannot wrap: it counts at most the voxels its workgroup sees between two flushes, and the entry
// point refuses (TEM_EINVAL) a box for which rows per workgroup x row width reaches 2^31.
#include "tem_common.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_COPIES = 32;
constexpr int HIST_MAX_GRID = 1024;        // 4 workgroups of 32 KiB LDS on each of 256 CUs

__device__ __forceinline__ void hist_add(uint32_t *h, uint32_t byte, uint32_t copy) {
  atomicAdd(&h[byte * HIST_COPIES + copy], 1u);
}

// thread t: bin t of the workgroup's copies -> counts[t]; `clear` leaves the copies zero for the next run
__device__ __forceinline__ void hist_flush(uint32_t *h, uint64_t *counts, bool clear) {
  __syncthreads();
  const uint32_t t = threadIdx.x;
  uint64_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < HIST_COPIES; ++j) {
    const uint32_t a = t * HIST_COPIES + ((j + t) & (HIST_COPIES - 1));
    s += h[a];
    if (clear) h[a] = 0;
  }
  if (s) atomicAdd(reinterpret_cast<unsigned long long *>(counts + t), (unsigned long long)s);
  if (clear) __syncthreads();
}

// src: the box's first byte (z0, y0, x0).  Row r = zi * ny + yi of the box starts at src + (zi * H + yi) * W.
// S: segments per row, an upper bound of ceil(((address & 15) + width) / 16) over all alignments; magicS = magic_for(S).
__global__ __launch_bounds__(HIST_THREADS) void u8_hist_k(const uint8_t *src, int64_t H, int64_t W, int ny, int width,
                                                          int64_t nrows, int64_t rpw, uint32_t S, uint32_t magicS,
                                                          uint64_t *counts, int per_section) {
  __shared__ uint32_t h[256 * HIST_COPIES];
  for (int i = threadIdx.x; i < 256 * HIST_COPIES; i += HIST_THREADS) h[i] = 0;
  __syncthreads();
  const uint32_t copy = threadIdx.x & (HIST_COPIES - 1);
  int64_t r0 = (int64_t)blockIdx.x * rpw;
  const int64_t r1 = min(r0 + rpw, nrows);
  while (r0 < r1) {
    const int64_t zi = r0 / ny;
    const uint32_t y00 = (uint32_t)(r0 - zi * ny);                       // the run starts at row y00 of section zi
    const int64_t rend = per_section ? min(r1, (zi + 1) * ny) : r1;
    const uint32_t total = (uint32_t)(rend - r0) * S;                    // < 2^31: the entry point's bound
    for (uint32_t i = threadIdx.x; i < total; i += HIST_THREADS) {
      const uint32_t ri = S == 1 ? i : __umulhi(i, magicS), s = i - ri * S;
      const uint32_t yy = y00 + ri, dz = yy / (uint32_t)ny, y = yy - dz * (uint32_t)ny;   // y00, ri < 2^31
      const uint8_t *row = src + ((zi + dz) * H + y) * W;
      const int64_t m = (int64_t)((uintptr_t)row & 15);                  // the row starts m bytes into a 16-byte line
      const int64_t lo = max((int64_t)16 * s - m, (int64_t)0), hi = min((int64_t)16 * s + 16 - m, (int64_t)width);
      if (hi - lo == 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + lo);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int k = 0; k < 4; ++k) hist_add(h, (w[j] >> (8 * k)) & 255u, copy);
        }
      } else {
        for (int64_t b = lo; b < hi; ++b) hist_add(h, row[b], copy);
      }
    }
    r0 = rend;
    hist_flush(h, counts + (per_section ? zi * 256 : 0), r0 < r1);
  }
}

// ---------------------------------------------------------------------------------------------------------- lut
// Block b: part b % bps of section b / bps (no per_section: one section, the whole buffer).  It copies its section's
// 256-byte table into LDS once, then maps its run of 16-byte lines of the section: whole lines as one dwordx4 load and
// one dwordx4 store, the section's first and last line byte by byte where the section covers them only partly.
__global__ __launch_bounds__(256) void u8_lut_k(uint8_t *buf, int64_t secbytes, const uint8_t *lut, int64_t zsec0,
                                                int per_section, uint32_t bps, int64_t per) {
  __shared__ uint8_t t[256];
  const int64_t sec = blockIdx.x / bps;
  const uint32_t part = blockIdx.x - (uint32_t)sec * bps;
  t[threadIdx.x] = lut[(per_section ? (zsec0 + sec) * 256 : 0) + threadIdx.x];
  __syncthreads();
  uint8_t *base = buf + sec * secbytes;
  const int m = (int)((uintptr_t)base & 15);
  const int64_t nline = (m + secbytes + 15) / 16;
  const int64_t l1 = min(nline, (int64_t)(part + 1) * per);
  for (int64_t l = (int64_t)part * per + threadIdx.x; l < l1; l += 256) {
    const int64_t lo = max(16 * l - m, (int64_t)0), hi = min(16 * l + 16 - m, secbytes);
    if (hi - lo == 16) {
      uint4 v = *reinterpret_cast<const uint4 *>(base + lo);
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w[j] = (uint32_t)t[w[j] & 255u] | ((uint32_t)t[(w[j] >> 8) & 255u] << 8) |
               ((uint32_t)t[(w[j] >> 16) & 255u] << 16) | ((uint32_t)t[w[j] >> 24] << 24);
      *reinterpret_cast<uint4 *>(base + lo) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (int64_t b = lo; b < hi; ++b) base[b] = t[base[b]];
    }
  }
}

}  // namespace

extern "C" int tem_u8_hist(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t z1, int32_t y0,
                           int32_t y1, int32_t x0, int32_t x1, uint64_t *counts, int32_t per_section,
                           tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!src || !counts || ((uintptr_t)counts & 7) || D < 1 || H < 1 || W < 1 || z0 < 0 || z0 > z1 || z1 > D || y0 < 0 ||
      y0 > y1 || y1 > H || x0 < 0 || x0 > x1 || x1 > W || (per_section != 0 && per_section != 1))
    return TEM_EINVAL;
  const int64_t nz = z1 - z0, ny = y1 - y0, width = x1 - x0, nrows = nz * ny;
  if (nrows == 0 || width == 0) return TEM_OK;
  const int64_t S = (width + 30) / 16;                                   // segments per row, any alignment
  // one workgroup per 256 items at least, HIST_MAX_GRID at most
  const int64_t want = nrows >= (int64_t)HIST_MAX_GRID * HIST_THREADS ? HIST_MAX_GRID
                                                                   : (nrows * S + HIST_THREADS - 1) / HIST_THREADS;
  const int64_t grid0 = want < 1 ? 1 : (want > HIST_MAX_GRID ? HIST_MAX_GRID : want);
  const int64_t rpw = (nrows + grid0 - 1) / grid0;
  const int64_t grid = (nrows + rpw - 1) / rpw;
  // the 32-bit bound: a workgroup's counters and its item index both stay below 2^31 between two flushes
  if (rpw > (((int64_t)1 << 31) - 1) / (width > S ? width : S)) return TEM_EINVAL;
  const uint8_t *first = src + ((int64_t)z0 * H + y0) * W + x0;
  hipLaunchKernelGGL(u8_hist_k, dim3((unsigned)grid), dim3(HIST_THREADS), 0, (hipStream_t)stream, first, (int64_t)H,
                     (int64_t)W, (int)ny, (int)width, nrows, rpw, (uint32_t)S, magic_for((int)S), counts,
                     (int)per_section);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}

extern "C" int tem_u8_lut(uint8_t *buf, int32_t D, int32_t H, int32_t W, const uint8_t *lut, int32_t per_section,
                          int32_t zsec0, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!buf || !lut || D < 1 || H < 1 || W < 1 || zsec0 < 0 || (per_section != 0 && per_section != 1)) return TEM_EINVAL;
  const int64_t nsec = per_section ? D : 1;
  const int64_t secbytes = per_section ? (int64_t)H * W : (int64_t)D * H * W;
  const int64_t nline = (secbytes + 15 + 15) / 16;                        // lines of a section, any alignment
  // parts per section: 4 lines per thread at least, about 2048 workgroups in all at most
  int64_t bps = (nline + 1023) / 1024, cap = (2048 + nsec - 1) / nsec;
  bps = bps > cap ? cap : bps;
  const int64_t per = (nline + bps - 1) / bps;
  bps = (nline + per - 1) / per;
  if (nsec * bps > 0x7fffffff) return TEM_EUNSUPPORTED;
  hipLaunchKernelGGL(u8_lut_k, dim3((unsigned)(nsec * bps)), dim3(256), 0, (hipStream_t)stream, buf, secbytes, lut,
                     (int64_t)zsec0, (int)per_section, (uint32_t)bps, per);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
