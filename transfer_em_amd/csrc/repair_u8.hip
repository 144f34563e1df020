// repair_u8.hip -- tem_u8_repair_z: bad voxels of a dense uint8 block filled along z from the nearest good voxels of
// their own column, in place (include/tem_hip.h has the rule).  A voxel is bad by a byte mask, by a per-section flag or
// by its value; a bad voxel's result needs the nearest good voxel at most R = max_gap planes below (value a, distance
// d0) and above (b, d1): linear between the two, or a copy of the one that exists.
//
// The kernel is a march along z.  A thread owns four x-consecutive columns -- one dword of every plane -- and keeps,
// per column, the last good value and the plane it was seen in.  No look-ahead buffer:
//   * a bad voxel with a good one at most R below is written with that value at once (right if nothing good follows
//     within R, provisional otherwise);
//   * the next good voxel, at z1, back-fills the bad voxels of [max(zlast + 1, z1 - R), z1 - 1] with their final value:
//     linear where zlast is at most R below them, else the copy from above.
// A column belongs to one thread, so its writes need no ordering, and the sources are good voxels, which nobody
// writes.  RP_AHEAD planes are loaded before the first of them is consumed, so that a thread has that many loads in
// flight; the state is then updated in plane order (issuing the next batch ahead of this one's update, with or without
// a register copy between the two, gained nothing: DESIGN.md).  The division by 2 n (n = d0 + d1 <= 64) is a multiply-high by
// ceil(2^32 / 2n), exact for numerators below 2^15 (they stay below 2^15: 2 x 255 x 64 + 64).
//
// Alignment.  With a plane stride H W that is a multiple of 4 (and a mask whose address is congruent to buf's mod 4)
// the dword at (buf & ~3) + 4 g + z H W is aligned in every plane: group g is then read with one dword load per plane
// and a changed plane written with one dword store (the four bytes are the thread's own columns).  The first and the
// last group of a plane, where they reach outside it, and every group of any other stride, take the byte path: the
// same march with up to four byte loads per plane and byte stores of the changed bytes only; columns outside the
// plane are never bad, so they are neither read nor written.  Back-fill is byte stores on both paths.
//
// z-runs.  Where the columns are too few to fill the chip, the core is cut into runs along z (blockIdx.y): a run starts
// its state R planes below its first plane and scans R planes past its last, writing its own planes only.  A run's halo
// planes belong to its neighbours, which write bad voxels there while it reads them.  With a mask or section flags that
// is harmless -- a bad voxel's byte is never used -- but with missing_value badness IS the byte, so such a launch is one
// run.
//
// Counts: bad and repaired core voxels are counted per thread, summed in the wave by shuffles and across the waves
// through LDS, and one thread issues at most two 64-bit global atomic adds per workgroup (zero sums skipped).
#include "tem_common.h"

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_AHEAD = 8;              // planes in flight per thread
constexpr int RP_NONE = -64;             // "no good voxel seen": z - RP_NONE > 32 >= R for every z >= 0
constexpr int RP_TARGET_WAVES = 2048;    // 8 per CU: what the run count aims for

struct RepairArgs {
  uint8_t *buf;
  const uint8_t *mask, *sections;
  uint64_t *counts;
  int64_t P, G;                          // plane stride H W; groups of 4 columns per plane
  int D, zsec0, c0, c1, runlen, missing, R, wide, m;
};

template <bool WIDE>
__device__ __forceinline__ uint32_t rp_load(const uint8_t *p, uint32_t valid) {
  if constexpr (WIDE) {
    return *reinterpret_cast<const uint32_t *>(p);
  } else {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((valid >> k) & 1u) w |= (uint32_t)p[k] << (8 * k);
    return w;
  }
}

// bit k: byte k of w is non-zero
__device__ __forceinline__ uint32_t rp_nonzero(uint32_t w) {
  return ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
}

// The march of one group over the planes [max(zs - R, 0), min(ze + R, D)), writing planes [zs, ze) only.  `col` is the
// column of byte 0 (it may lie up to 3 columns outside the plane on the byte path), `valid` the bytes inside the plane.
template <bool WIDE>
__device__ __forceinline__ void rp_march(const RepairArgs &a, int64_t col, uint32_t valid, int zs, int ze,
                                         const uint32_t *magic, uint32_t &nbad, uint32_t &nrep) {
  const int R = a.R;
  const int z0 = max(zs - R, 0), z1 = min(ze + R, a.D);
  const uint32_t miss4 = a.missing >= 0 ? (uint32_t)a.missing * 0x01010101u : 0u;
  uint32_t lastw = 0;
  int zl[4] = {RP_NONE, RP_NONE, RP_NONE, RP_NONE};
  for (int zb = z0; zb < z1; zb += RP_AHEAD) {
    uint32_t w[RP_AHEAD], mk[RP_AHEAD], sec[RP_AHEAD];
#pragma unroll
    for (int j = 0; j < RP_AHEAD; ++j) {
      const int z = zb + j;
      w[j] = mk[j] = sec[j] = 0;
      if (z < z1) {
        const int64_t off = (int64_t)z * a.P + col;
        w[j] = rp_load<WIDE>(a.buf + off, valid);
        if (a.mask) mk[j] = rp_load<WIDE>(a.mask + off, valid);
        if (a.sections) sec[j] = a.sections[(int64_t)a.zsec0 + z];
      }
    }
#pragma unroll
    for (int j = 0; j < RP_AHEAD; ++j) {
      const int z = zb + j;
      if (z >= z1) break;
      uint32_t bad = rp_nonzero(mk[j]);
      if (a.missing >= 0) bad |= 15u ^ rp_nonzero(w[j] ^ miss4);
      if (sec[j]) bad = 15u;
      bad &= valid;
      if (bad == 0 && zl[0] == z - 1 && zl[1] == z - 1 && zl[2] == z - 1 && zl[3] == z - 1) {   // the common plane
        lastw = w[j];
        zl[0] = zl[1] = zl[2] = zl[3] = z;
        continue;
      }
      const bool inw = z >= zs && z < ze;
      uint32_t nw = w[j];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t byte = 0xffu << (8 * k);
        if (!((bad >> k) & 1u)) {
          if (zl[k] != z - 1 && ((valid >> k) & 1u)) {                  // a run of bad voxels ends here: back-fill
            const uint32_t va = (lastw >> (8 * k)) & 0xffu, vb = (w[j] >> (8 * k)) & 0xffu;
            const int lo = max(max(zl[k] + 1, z - R), zs), hi = min(z, ze);
            for (int zz = lo; zz < hi; ++zz) {
              const int d1 = z - zz, d0 = zz - zl[k];
              uint32_t v = vb;
              if (d0 <= R) {
                const uint32_t n = (uint32_t)(d0 + d1);
                v = __umulhi(2u * (va * (uint32_t)d1 + vb * (uint32_t)d0) + n, magic[n]);
              } else {
                ++nrep;                                                  // nothing below: repaired only now
              }
              a.buf[(int64_t)zz * a.P + col + k] = (uint8_t)v;
            }
          }
          lastw = (lastw & ~byte) | (w[j] & byte);
          zl[k] = z;
        } else if (inw) {
          ++nbad;
          if (z - zl[k] <= R) {                                          // the copy from below, final or provisional
            nw = (nw & ~byte) | (lastw & byte);
            ++nrep;
          }
        }
      }
      if (nw != w[j]) {
        uint8_t *p = a.buf + (int64_t)z * a.P + col;
        if constexpr (WIDE) {
          *reinterpret_cast<uint32_t *>(p) = nw;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (((nw ^ w[j]) >> (8 * k)) & 0xffu) p[k] = (uint8_t)(nw >> (8 * k));
        }
      }
    }
  }
}

__device__ __forceinline__ uint32_t rp_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

__global__ __launch_bounds__(RP_THREADS) void u8_repair_z_k(RepairArgs a) {
  __shared__ uint32_t magic[65];                   // magic[n] = ceil(2^32 / 2n), n = 2...64
  __shared__ uint32_t red[2][RP_THREADS / 64];
  const int t = threadIdx.x;
  if (t >= 2 && t <= 64) magic[t] = 0xffffffffu / (2u * (uint32_t)t) + 1u;
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * RP_THREADS + t;
  const int zs = a.c0 + (int)blockIdx.y * a.runlen, ze = min(zs + a.runlen, a.c1);
  uint32_t nbad = 0, nrep = 0;
  if (g < a.G) {
    const int64_t col = 4 * g - a.m;
    uint32_t valid = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (col + k >= 0 && col + k < a.P) valid |= 1u << k;
    if (a.wide && valid == 15u)
      rp_march<true>(a, col, valid, zs, ze, magic, nbad, nrep);
    else
      rp_march<false>(a, col, valid, zs, ze, magic, nbad, nrep);
  }
  if (a.counts) {
    nbad = rp_wave_sum(nbad);                      // a wave counts at most 256 columns x D planes: below 2^32 for the
    nrep = rp_wave_sum(nrep);                      // D <= 2^21 the entry point admits
    if ((t & 63) == 0) { red[0][t >> 6] = nbad; red[1][t >> 6] = nrep; }
    __syncthreads();
    if (t == 0) {
      uint64_t b = 0, r = 0;
#pragma unroll
      for (int i = 0; i < RP_THREADS / 64; ++i) { b += red[0][i]; r += red[1][i]; }
      if (r) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts), (unsigned long long)r);
      if (b - r) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + 1), (unsigned long long)(b - r));
    }
  }
}

}  // namespace

extern "C" int tem_u8_repair_z(uint8_t *buf, int32_t D, int32_t H, int32_t W, int32_t zsec0, int32_t c0, int32_t c1,
                               const uint8_t *mask, const uint8_t *sections, int32_t missing, int32_t max_gap,
                               uint64_t *counts, tem_stream_t stream) {
  TEM_CLEAR_ERR();
  if (!buf || D < 1 || H < 1 || W < 1 || zsec0 < 0 || max_gap < 1 || max_gap > 32 || c0 < 0 || c0 > c1 || c1 > D ||
      missing < -1 || missing > 255 || (!mask && !sections && missing < 0) || ((uintptr_t)counts & 7))
    return TEM_EINVAL;
  if (D > (1 << 21)) return TEM_EUNSUPPORTED;      // the 32-bit counters of a wave (see the kernel)
  if (c0 == c1) return TEM_OK;
  RepairArgs a;
  a.buf = buf, a.mask = mask, a.sections = sections, a.counts = counts;
  a.P = (int64_t)H * W;
  a.D = D, a.zsec0 = zsec0, a.c0 = c0, a.c1 = c1, a.missing = missing, a.R = max_gap;
  a.wide = a.P % 4 == 0 && (!mask || (((uintptr_t)mask ^ (uintptr_t)buf) & 3) == 0);
  a.m = a.wide ? (int)((uintptr_t)buf & 3) : 0;
  a.G = (a.P + a.m + 3) / 4;
  const int64_t blocks = (a.G + RP_THREADS - 1) / RP_THREADS;
  if (blocks > 0x7fffffff) return TEM_EUNSUPPORTED;
  // z-runs: enough waves to fill the chip, each run at least 4 R planes long (it scans 2 R more); one run where
  // badness is the byte itself (see the head of this file)
  const int ncore = c1 - c0;
  int64_t nruns = 1;
  if (missing < 0) {
    const int64_t waves = (a.G + 63) / 64;
    const int64_t want = (RP_TARGET_WAVES + waves - 1) / waves, most = ncore / (4 * max_gap);
    nruns = want < most ? want : most;
    if (nruns < 1) nruns = 1;
  }
  a.runlen = (int)((ncore + nruns - 1) / nruns);
  nruns = (ncore + a.runlen - 1) / a.runlen;       // <= RP_TARGET_WAVES
  hipLaunchKernelGGL(u8_repair_z_k, dim3((unsigned)blocks, (unsigned)nruns), dim3(RP_THREADS), 0, (hipStream_t)stream, a);
  TEM_CHECK_LAUNCH();
  return TEM_OK;
}
