// The parts and pieces that the kernels along z share (zcorr_u8.hip, zlags_u8.hip, resamplez_u8.hip): a 16-byte piece
// of a uint8 block at any address, loaded as the naturally aligned words that hold at least one of its bytes.
#pragma once
#include "tem_common.h"

namespace {

constexpr int ZC_THREADS = 256;
constexpr int ZC_MAX_TILE = 2048;
constexpr int ZC_WANT_GRID = 1024;               // workgroups the run length aims at (4 on each of 256 CUs)

// The n (1...16) bytes at p as four words, the bytes past n zero.
__device__ __forceinline__ void zc_load(const uint8_t *p, int n, uint32_t (&w)[4]) {
  const uint32_t a = (uint32_t)((uintptr_t)p & 3);
  if (!((uintptr_t)p & 15)) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - a);
    uint32_t r[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) r[j] = 4 * j < (int)a + n ? q[j] : 0u;  // word j: bytes [4 j - a, 4 j + 4 - a) of the piece
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_alignbyte(r[j + 1], r[j], a);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nb = n - 4 * j;
    if (nb < 4) w[j] = nb <= 0 ? 0u : w[j] & ((1u << (8 * nb)) - 1u);
  }
}

__device__ __forceinline__ uint32_t zc_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace
