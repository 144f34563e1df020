// hist2_u8.hip -- tem_u8_hist2: the 256 x 256 joint histogram of two boxes of the same extents, one in each of two
// dense uint8 blocks:  counts[256 u + v] += #{voxels with a == u and b == v}.  Everything point-wise about a pair of
// volumes (RMSE, MAE, PSNR, correlation, mutual information, both marginals, the paired intensity map) is a function
// of this table (utils.compare_from_joint, utils.regression_lut).
//
// Counters.  65,536 32-bit counters are 256 KiB and a CU has 160 KiB of LDS, so the table is split by the high bit of
// `a` over two CLASSES of workgroups (blockIdx.y): a class-c workgroup walks all voxels of its run of rows and counts
// those with a >> 7 == c into 32,768 private 32-bit counters (128 KiB of LDS, one workgroup of 1024 threads per CU),
// indexed ((a & 127) << 8) | b.  Every voxel is counted exactly once, by the one class it belongs to; the bytes are
// read twice, the second time mostly out of L2 / Infinity Cache.  The 32-bit no-wrap argument is tem_u8_hist's: a
// counter sees at most the voxels of its workgroup's run, which the entry point keeps below 2^31.  The counters are
// shared by all lanes (ds_add_u32): lanes of one instruction that hit the same counter are served one after the other,
// so a constant pair is the slow case -- and an exact one.
// Flush, once per workgroup: thread t walks counters t, t + 1024, ... and adds every non-zero one to
// counts[32768 c + i] with ONE ordinary 64-bit global atomic add; zero counters are skipped (an EM pair fills a band
// around the diagonal).  The box's rows are dealt in equal contiguous runs to at most HIST2_MAX_PARTS workgroups per
// class, a small box to fewer (one per HIST2_ITEMS_PER_WG items), so the flush traffic is bounded by
// 2 x 128 x occupied bins atomics.
//
// Loads.  The two rows of a voxel run are in general misaligned differently, so the work item is a 16-byte-ADDRESS-
// aligned segment of a's row (as in tem_u8_hist): a segment wholly inside the row travels as one dwordx4 of `a`, and
// its 16 partners of `b` as the (four or five) naturally aligned dwords that hold them -- one dwordx4 where b's run
// happens to be 16-byte aligned too -- shifted into place in registers; each of those dwords holds at least one byte of
// b's box.  The (at most two) cut segments of a row go byte by byte on both sides.  No byte outside the boxes is read.
#include "tem_common.h"

namespace {

constexpr int HIST2_THREADS = 1024;
constexpr int HIST2_BINS = 32768;              // per class: 128 values of a x 256 values of b
constexpr int HIST2_MAX_PARTS = 128;           // x 2 classes = one workgroup on each of 256 CUs
constexpr int HIST2_ITEMS_PER_WG = 4096;       // a small box: one workgroup (per class) per this many segments

__device__ __forceinline__ void hist2_add(uint32_t *h, uint32_t u, uint32_t v, uint32_t cls) {
  if ((u >> 7) == cls) atomicAdd(&h[((u & 127u) << 8) | v], 1u);
}

// a0 / b0: the boxes' first bytes.  Row r = zi * ny + yi of the boxes starts at a0 + (zi * Ha + yi) * Wa and at
// b0 + (zi * Hb + yi) * Wb.  S: segments per row, an upper bound of ceil(((address of a's row & 15) + nx) / 16) over
// all alignments; magicS = magic_for(S) = ceil(2^32 / S).
__global__ __launch_bounds__(HIST2_THREADS) void u8_hist2_k(const uint8_t *a0, int64_t Ha, int64_t Wa, const uint8_t *b0,
                                                            int64_t Hb, int64_t Wb, int ny, int nx, int64_t nrows,
                                                            int64_t rpw, uint32_t S, uint32_t magicS, uint64_t *counts) {
  __shared__ uint32_t h[HIST2_BINS];
  for (int i = threadIdx.x; i < HIST2_BINS; i += HIST2_THREADS) h[i] = 0;
  __syncthreads();
  const uint32_t cls = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = min(r0 + rpw, nrows);
  const int64_t zi = r0 / ny;
  const uint32_t y00 = (uint32_t)(r0 - zi * ny);                         // the run starts at row y00 of section zi
  const uint32_t total = (uint32_t)(r1 - r0) * S;                        // < 2^31: the entry point's bound
  for (uint32_t i = threadIdx.x; i < total; i += HIST2_THREADS) {
    // floor(i / S), exactly: the magic product is floor(i / S) or one above it for every i < 2^31 (its excess over
    // i / S is i (S magicS - 2^32) / (S 2^32) < 1/2), and it is one above for wide rows late in a run -- one step back
    uint32_t ri = S == 1 ? i : __umulhi(i, magicS);
    if (ri * S > i) --ri;                                                // ri S <= i + S < 2^32
    const uint32_t s = i - ri * S;
    const uint32_t yy = y00 + ri, dz = yy / (uint32_t)ny, y = yy - dz * (uint32_t)ny;     // y00, ri < 2^31
    const uint8_t *arow = a0 + ((zi + dz) * Ha + y) * Wa;
    const uint8_t *brow = b0 + ((zi + dz) * Hb + y) * Wb;
    const int64_t m = (int64_t)((uintptr_t)arow & 15);                   // a's row starts m bytes into a 16-byte line
    const int64_t lo = max((int64_t)16 * s - m, (int64_t)0), hi = min((int64_t)16 * s + 16 - m, (int64_t)nx);
    if (hi - lo == 16) {
      const uint4 va = *reinterpret_cast<const uint4 *>(arow + lo);
      const uint32_t wa[4] = {va.x, va.y, va.z, va.w};
      const uint8_t *pb = brow + lo;                                     // b's 16 bytes: [pb, pb + 16)
      const uint32_t sh = (uint32_t)((uintptr_t)pb & 3);
      uint32_t wb[4];
      if (((uintptr_t)pb & 15) == 0) {
        const uint4 vb = *reinterpret_cast<const uint4 *>(pb);
        wb[0] = vb.x, wb[1] = vb.y, wb[2] = vb.z, wb[3] = vb.w;
      } else {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(pb - sh);   // the aligned dword of b's first byte
        uint32_t w[5];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = q[j];
        w[4] = sh ? q[4] : 0u;                                           // holds bytes of the run only when it is cut
#pragma unroll
        for (int j = 0; j < 4; ++j) wb[j] = (uint32_t)((((uint64_t)w[j + 1] << 32) | w[j]) >> (8 * sh));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) hist2_add(h, (wa[j] >> (8 * k)) & 255u, (wb[j] >> (8 * k)) & 255u, cls);
      }
    } else {
      for (int64_t x = lo; x < hi; ++x) hist2_add(h, arow[x], brow[x], cls);
    }
  }
  __syncthreads();
  uint64_t *dst = counts + (int64_t)cls * HIST2_BINS;
  for (int i = threadIdx.x; i < HIST2_BINS; i += HIST2_THREADS) {
    const uint32_t c = h[i];
    if (c) atomicAdd(reinterpret_cast<unsigned long long *>(dst + i), (unsigned long long)c);
  }
}

}  // namespace

extern "C" int tem_u8_hist2(const uint8_t *a, int32_t Da, int32_t Ha, int32_t Wa, int32_t az0, int32_t ay0, int32_t ax0,
                            const uint8_t *b, int32_t Db, int32_t Hb, int32_t Wb, int32_t bz0, int32_t by0, int32_t bx0,
                            int32_t nz, int32_t ny, int32_t nx, uint64_t *counts, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!a || !b || !counts || ((uintptr_t)counts & 7) || Da < 1 || Ha < 1 || Wa < 1 || Db < 1 || Hb < 1 || Wb < 1 ||
      az0 < 0 || ay0 < 0 || ax0 < 0 || bz0 < 0 || by0 < 0 || bx0 < 0 || nz < 0 || ny < 0 || nx < 0)
    return TEM_EINVAL;
  if ((int64_t)az0 + nz > Da || (int64_t)ay0 + ny > Ha || (int64_t)ax0 + nx > Wa || (int64_t)bz0 + nz > Db ||
      (int64_t)by0 + ny > Hb || (int64_t)bx0 + nx > Wb)
    return TEM_EINVAL;
  const int64_t nrows = (int64_t)nz * ny, width = nx;
  if (nrows == 0 || width == 0) return TEM_OK;
  const int64_t S = (width + 30) / 16;                                   // segments per row, any alignment
  const int64_t want = nrows >= (int64_t)HIST2_MAX_PARTS * HIST2_ITEMS_PER_WG
                           ? HIST2_MAX_PARTS
                           : (nrows * S + HIST2_ITEMS_PER_WG - 1) / HIST2_ITEMS_PER_WG;
  const int64_t parts0 = want < 1 ? 1 : (want > HIST2_MAX_PARTS ? HIST2_MAX_PARTS : want);
  const int64_t rpw = (nrows + parts0 - 1) / parts0;
  const int64_t parts = (nrows + rpw - 1) / rpw;
  // the 32-bit bound: a workgroup's counters and its item index both stay below 2^31
  if (rpw > (((int64_t)1 << 31) - 1) / (width > S ? width : S)) return TEM_EINVAL;
  const uint8_t *a0 = a + ((int64_t)az0 * Ha + ay0) * Wa + ax0;
  const uint8_t *b0 = b + ((int64_t)bz0 * Hb + by0) * Wb + bx0;
  hipLaunchKernelGGL(u8_hist2_k, dim3((unsigned)parts, 2), dim3(HIST2_THREADS), 0, (hipStream_t)stream, a0, (int64_t)Ha,
                     (int64_t)Wa, b0, (int64_t)Hb, (int64_t)Wb, (int)ny, (int)nx, nrows, rpw, (uint32_t)S,
                     magic_for((int)S), counts);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
