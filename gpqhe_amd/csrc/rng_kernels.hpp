// rng_kernels.hpp -- the reference's deterministic randombytes (src/rng.c:36-77, SUPERCOP's surf generator) addressed by POSITION
// (include/gpqhe_hip.h, "random bytes on the device").
//   The generator runs in counter mode: in[0..3] is a 128-bit block counter, incremented BEFORE each block (:69), in[4..11] stay 0, and a
//   block depends on nothing but its counter.  A block hands out the low bytes of out[7], out[6], .., out[0] in that order
//   (`*x = out[--outleft]`, :73, truncates a uint32_t).  So byte k of the stream is the low byte of out[7 - k % 8] of the block with
//   counter k / 8 + 1, and any slice is the work of independent lanes.
//   surf_block      one block as the little-endian 64-bit word of its 8 stream bytes; host and device
//   surf_stream_k   bytes [pos, pos + len) of the stream into dst[0..len): one aligned 16-byte chunk of the destination per lane
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpq {

struct SurfSeed { uint32_t w[32]; };
struct U128 { uint64_t lo, hi; };

__host__ __device__ __forceinline__ uint32_t surf_rotl(uint32_t x, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, 32 - b);                                 // one v_alignbit_b32
#else
  return (x << b) | (x >> (32 - b));
#endif
}

// surf(), src/rng.c:46-63, for the counter (c0, c1, c2, c3) = in[0..3]; the 8 bytes it hands out, first byte lowest
__host__ __device__ __forceinline__ uint64_t surf_block(const SurfSeed &s, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
  uint32_t t[12], o[8];
  t[0] = c0 ^ s.w[12]; t[1] = c1 ^ s.w[13]; t[2] = c2 ^ s.w[14]; t[3] = c3 ^ s.w[15];
#pragma unroll
  for (int i = 4; i < 12; ++i) t[i] = s.w[12 + i];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = s.w[24 + i];
  uint32_t x = t[11], sum = 0;
#pragma unroll
  for (int loop = 0; loop < 2; ++loop) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sum += 0x9e3779b9u;
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const unsigned b = (i & 3) == 0 ? 5u : (i & 3) == 1 ? 7u : (i & 3) == 2 ? 9u : 13u;
        x = t[i] += (((x ^ s.w[i]) + sum) ^ surf_rotl(x, b));                     // MUSH(i, b), :44
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] ^= t[i + 4];
  }
  const uint32_t lo = (o[7] & 255u) | ((o[6] & 255u) << 8) | ((o[5] & 255u) << 16) | (o[4] << 24);
  const uint32_t hi = (o[3] & 255u) | ((o[2] & 255u) << 8) | ((o[1] & 255u) << 16) | (o[0] << 24);
  return lo | ((uint64_t)hi << 32);
}

// the block that holds stream bytes [8 idx, 8 idx + 8): its counter is idx + 1.  idx is taken mod 2^125 (a 128-bit BYTE position has
// no more blocks), so the counter never wraps.
__host__ __device__ __forceinline__ uint64_t surf_block_at(const SurfSeed &s, U128 idx) {
  idx.hi &= 0x1fffffffffffffffull;
  const uint64_t lo = idx.lo + 1, hi = idx.hi + (lo == 0);
  return surf_block(s, (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
__host__ __device__ __forceinline__ U128 u128_add(U128 a, uint64_t b) {
  U128 r{a.lo + b, a.hi};
  r.hi += r.lo < b;
  return r;
}

// dst[0..len) <- stream bytes [pos, pos + len).  Lane t owns the aligned 16-byte chunk t of the destination, counted from dst rounded
// down to 16: the chunk's stream position is `start` + 16 t, where start = pos - (dst & 15) mod 2^128 (the bytes in front of dst are
// never produced).  start % 8 == 0 -- every caller that slices a stream at multiples of 8 into an aligned buffer -- makes a chunk two
// whole blocks; otherwise it straddles three and is funnel-shifted together.  A chunk inside [dst, dst + len) leaves as one 16-byte
// store; the first and last chunk of an unaligned destination go byte by byte, inside the bounds only.  seed, start and the bounds are
// kernel arguments: wave-uniform, the branch on start % 8 included.  Cost of the other phases: the block a chunk shares with its
// neighbour is computed by both lanes, three blocks for 16 bytes, 1.5 times the work of the aligned phase (no exchange between lanes).
struct SurfStreamArgs {
  uint8_t *base;          // dst rounded down to 16 bytes
  uint32_t head;          // dst - base, 0..15
  uint64_t end;           // head + len: the bytes [head, end) of the chunks are written
  U128 start;             // stream position of base[0], mod 2^128
  SurfSeed seed;
};

// lane t's chunk (host and device: the bounds logic runs under a host sanitizer as it stands)
__host__ __device__ __forceinline__ void surf_chunk(const SurfStreamArgs &a, uint64_t t) {
  const uint64_t off = 16 * t;
  if (off >= a.end) return;
  const U128 s = u128_add(a.start, off);
  const unsigned r = (unsigned)(s.lo & 7);                                         // == start % 8 for every lane
  const U128 idx{(s.lo >> 3) | (s.hi << 61), s.hi >> 3};
  uint64_t w0 = surf_block_at(a.seed, idx), w1 = surf_block_at(a.seed, u128_add(idx, 1));
  if (r) {
    const uint64_t w2 = surf_block_at(a.seed, u128_add(idx, 2));
    w0 = (w0 >> (8 * r)) | (w1 << (64 - 8 * r));
    w1 = (w1 >> (8 * r)) | (w2 << (64 - 8 * r));
  }
  uint8_t *p = a.base + off;
  const unsigned lo = t == 0 ? a.head : 0u, hi = a.end - off < 16 ? (unsigned)(a.end - off) : 16u;
  if (lo == 0 && hi == 16) {
    *(uint4 *)p = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    return;
  }
  for (unsigned j = lo; j < hi; ++j) p[j] = (uint8_t)((j < 8 ? w0 : w1) >> (8 * (j & 7)));
}

__global__ __launch_bounds__(256) void surf_stream_k(SurfStreamArgs a) { surf_chunk(a, (uint64_t)blockIdx.x * 256 + threadIdx.x); }

}  // namespace gpq
