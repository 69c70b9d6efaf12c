// enc_kernels.hpp -- the samplers and the encryptor's own kernels (include/gpqhe_hip.h, "samplers and encryption on the device").
//   sample_zo_k, sample_error_k   src/sample.c:112-131, :60-82: the caller's random BYTES -> small slabs int8_t[count][n]
//   sample_uniform_k              src/sample.c:133-141 with loadmpi_littleendian (src/types.c:166-184): bytes -> word planes
//   small_to_rns_k, small_to_big_k  a small slab as canonical residues [batch][dim][n] / as a sign-extended big slab
//   enc_tail_k                    out = smod(+-x + m + e, 2^logq), the loops of src/he-encrypt.c:60-66 and :92-98 in one pass
// The byte inputs sit at ANY byte address (a caller slices one stream).  Global memory is only ever read through aligned 16-byte or 4-byte
// words that hold at least one byte of the input, and shifted into place in registers; what does not fill a lane's 16 bytes goes byte by byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tables.hpp"

namespace gpq {

// p[0..15] as four little-endian dwords, for any p: two aligned 16-byte loads (one when p is aligned), funnel-shifted by p & 15.
// Every byte of p[0..15] must be readable; the second load is only issued when it holds one of them.
__device__ __forceinline__ uint4 load16_any(const uint8_t *p) {
  const unsigned a = (unsigned)((uintptr_t)p & 15);
  const uint4 *q = (const uint4 *)(p - a);
  const uint4 lo = q[0];
  uint4 hi = make_uint4(0, 0, 0, 0);
  if (a) hi = q[1];
  uint64_t x0 = lo.x | ((uint64_t)lo.y << 32), x1 = lo.z | ((uint64_t)lo.w << 32);
  uint64_t x2 = hi.x | ((uint64_t)hi.y << 32), x3 = hi.z | ((uint64_t)hi.w << 32);
  if (a & 8) { x0 = x1; x1 = x2; x2 = x3; }
  const unsigned s = (a & 7) * 8;
  if (s) { x0 = (x0 >> s) | (x1 << (64 - s)); x1 = (x1 >> s) | (x2 << (64 - s)); }
  return make_uint4((unsigned)x0, (unsigned)(x0 >> 32), (unsigned)x1, (unsigned)(x1 >> 32));
}
// p[0..3] as one little-endian dword, for any p: one or two aligned dword loads
__device__ __forceinline__ unsigned load4_any(const uint8_t *p) {
  const unsigned a = (unsigned)((uintptr_t)p & 3);
  const unsigned *q = (const unsigned *)(p - a);
  unsigned v = q[0];
  if (a) v = (v >> (8 * a)) | (q[1] << (32 - 8 * a));
  return v;
}

// sample_zero_center, src/sample.c:112-121: bit 2i of the bytes' little-endian integer clear -> 0, else bit 2i + 1 clear -> +1, else -1.
// One input byte makes four coefficients, so the whole call is ONE stream: `nbytes` = count n/4 bytes in, 4 nbytes coefficients out.
__device__ __forceinline__ unsigned zo_expand(unsigned byte) {                 // four int8 coefficients of one byte, packed
  unsigned r = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned two = (byte >> (2 * k)) & 3;
    r |= ((two & 1) ? ((two & 2) ? 0xFFu : 1u) : 0u) << (8 * k);
  }
  return r;
}
struct SampleZoArgs { const uint8_t *in; int8_t *out; size_t nbytes; };

__global__ __launch_bounds__(256) void sample_zo_k(SampleZoArgs a) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool wide = ((uintptr_t)a.out & 15) == 0;                                // 16-byte stores need the output aligned: else all by bytes
  const size_t nvec = wide ? a.nbytes / 4 : 0;                                    // lanes with 4 bytes in, 16 coefficients out
  if (t < nvec) {
    const unsigned v = load4_any(a.in + 4 * t);
    *(uint4 *)(a.out + 16 * t) = make_uint4(zo_expand(v & 255), zo_expand((v >> 8) & 255), zo_expand((v >> 16) & 255), zo_expand(v >> 24));
    return;
  }
  const size_t b = 4 * nvec + (t - nvec);                                         // the tail (or everything), one input byte per thread
  if (b >= a.nbytes) return;
  const unsigned r = zo_expand(a.in[b]);
#pragma unroll
  for (int k = 0; k < 4; ++k) a.out[4 * b + k] = (int8_t)(r >> (8 * k));
}

// sample_discrete_gaussian, src/sample.c:60-72, through the table of its 65536 possible byte pairs (gpq_sample_error_table): no floating
// point here.  table[(b0 << 8 | b1)] = the two int8 coefficients as one 16-bit word; 128 KiB, L2-resident.  Pairs start at even coefficient
// indices and n is even, so the call is one stream of `nbytes` = count n bytes.
struct SampleErrorArgs { const uint8_t *in; int8_t *out; const uint16_t *table; size_t nbytes; };

__device__ __forceinline__ unsigned error_pairs(const uint16_t *__restrict__ table, unsigned w) {        // four bytes -> four coefficients
  const unsigned lo = table[((w & 255) << 8) | ((w >> 8) & 255)], hi = table[(((w >> 16) & 255) << 8) | (w >> 24)];
  return lo | (hi << 16);
}

__global__ __launch_bounds__(256) void sample_error_k(SampleErrorArgs a) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool wide = ((uintptr_t)a.out & 15) == 0;
  const size_t nvec = wide ? a.nbytes / 16 : 0;                                   // lanes with 16 bytes in, 16 coefficients out
  if (t < nvec) {
    const uint4 v = load16_any(a.in + 16 * t);
    *(uint4 *)(a.out + 16 * t) = make_uint4(error_pairs(a.table, v.x), error_pairs(a.table, v.y), error_pairs(a.table, v.z), error_pairs(a.table, v.w));
    return;
  }
  const size_t b = 16 * nvec + 2 * (t - nvec);                                    // the tail (or everything), one pair per thread
  if (b + 1 >= a.nbytes) return;
  const unsigned e = a.table[((unsigned)a.in[b] << 8) | a.in[b + 1]];
  a.out[b] = (int8_t)e; a.out[b + 1] = (int8_t)(e >> 8);
}

// sample_uniform, src/sample.c:133-141: coefficient c = the low `nbits` bits of the little-endian integer of its nb = nbits / 8 + 1 bytes
// (the rest of the last byte -- all of it when nbits % 8 == 0 -- is consumed and dropped); NOT reduced, NOT centred.
// Rows of nb bytes in, word planes out (word j of coefficient i at j n + i).  A workgroup stages the bytes of kUniformTile coefficients in
// LDS: they are contiguous in global memory, so they are read 16 bytes per lane whatever nb is, and scattered into rows of `stride` bytes
// (a multiple of 8 with stride / 8 odd: the 64-bit reads of 32 consecutive rows then fall on distinct banks).  Each wave then writes 64
// consecutive words of one plane per instruction.  W = 32 (nb <= 256): 64 rows of 264 bytes = 16.5 KiB.
constexpr unsigned kUniformTile = 64;
struct SampleUniformArgs {
  const uint8_t *in; uint64_t *out;
  size_t ncoef;                 // count n
  unsigned nbits, nb, W, logn;
  unsigned stride;              // LDS bytes per coefficient
  unsigned magic;               // ceil(2^32 / nb): o / nb = umulhi(o, magic) for o < 2^14 + 16, nb <= 256
};

__device__ __forceinline__ void uniform_scatter(uint8_t *lds, const SampleUniformArgs &a, unsigned o, unsigned byte) {
  const unsigned c = a.nb == 1 ? o : __umulhi(o, a.magic);
  lds[c * a.stride + (o - c * a.nb)] = (uint8_t)byte;
}

__global__ __launch_bounds__(256) void sample_uniform_k(SampleUniformArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t uniform_lds[];
  const size_t c0 = (size_t)blockIdx.x * kUniformTile;
  const unsigned rows = a.ncoef - c0 < kUniformTile ? (unsigned)(a.ncoef - c0) : kUniformTile;
  const uint8_t *__restrict__ src = a.in + c0 * a.nb;
  const unsigned len = rows * a.nb;
  unsigned head = (unsigned)((0 - (uintptr_t)src) & 15);
  if (head > len) head = len;
  const unsigned nvec = (len - head) / 16, tail0 = head + 16 * nvec;
  if (threadIdx.x < head) uniform_scatter(uniform_lds, a, threadIdx.x, src[threadIdx.x]);
  if (threadIdx.x < len - tail0) uniform_scatter(uniform_lds, a, tail0 + threadIdx.x, src[tail0 + threadIdx.x]);
  for (unsigned v = threadIdx.x; v < nvec; v += 256) {
    const uint4 q = *(const uint4 *)(src + head + 16 * v);
    // lanes 8 apart would write the same LDS bank (16 bytes per lane = 4 banks): each group of 8 lanes starts one dword later
    const unsigned rot = 4 * ((threadIdx.x >> 3) & 3);
#pragma unroll
    for (unsigned k = 0; k < 16; ++k) {
      const unsigned b = (k + rot) & 15;
      const unsigned w = (b & 8) ? ((b & 4) ? q.w : q.z) : ((b & 4) ? q.y : q.x);
      uniform_scatter(uniform_lds, a, head + 16 * v + b, (w >> (8 * (b & 3))) & 255);
    }
  }
  __syncthreads();
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane >= rows) return;
  const size_t c = c0 + lane;
  uint64_t *__restrict__ dst = a.out + (((c >> a.logn) * a.W) << a.logn) + (c & (((size_t)1 << a.logn) - 1));
  for (unsigned j = wave; j < a.W; j += 4) {
    uint64_t w = 0;
    if (64 * j < a.nbits) {                                                        // (then 8 j + 8 <= stride)
      w = *(const uint64_t *)(uniform_lds + lane * a.stride + 8 * j);
      const unsigned keep = a.nbits - 64 * j;
      if (keep < 64) w &= (1ull << keep) - 1;
    }
    dst[(size_t)j << a.logn] = w;
  }
}

// A small slab as canonical residues: slab[k][d][i] = x >= 0 ? x : p_d + x (|x| < 128 < p_d).  What rns_decompose makes of the small
// polynomial, without its W-word integer ever existing.
struct SmallToRnsArgs { const int8_t *small; uint64_t *slab; const LimbTab *tabs; unsigned dim, logn; };

__global__ __launch_bounds__(256) void small_to_rns_k(SmallToRnsArgs a) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (1u << a.logn)) return;
  const int64_t x = a.small[((size_t)blockIdx.y << a.logn) + i];
  uint64_t *__restrict__ dst = a.slab + ((size_t)blockIdx.y * a.dim << a.logn) + i;
  for (unsigned d = 0; d < a.dim; ++d) dst[(size_t)d << a.logn] = x >= 0 ? (uint64_t)x : a.tabs[d].k.p + (uint64_t)x;
}

// ... and as a sign-extended big slab of W words
struct SmallToBigArgs { const int8_t *small; uint64_t *big; unsigned W, logn; };

__global__ __launch_bounds__(256) void small_to_big_k(SmallToBigArgs a) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (1u << a.logn)) return;
  const int64_t x = a.small[((size_t)blockIdx.y << a.logn) + i];
  uint64_t *__restrict__ dst = a.big + ((size_t)blockIdx.y * a.W << a.logn) + i;
  dst[0] = (uint64_t)x;
  for (unsigned j = 1; j < a.W; ++j) dst[(size_t)j << a.logn] = (uint64_t)(x >> 63);
}

// out = smod(sign x + m + e, 2^logq) on big slabs of W words: mpi_neg / mpi_add / mpi_addm / mpi_smod of src/he-encrypt.c:60-66, :92-98 and
// src/he-kem.c:60-65 in one pass (smod as bridge_addsub: keep logq bits, sign-extend from bit logq - 1).  m: big slab or null; e: small slab
// or null; negate: x enters as -x.  out may be x (each thread reads a word before it writes it).
struct EncTailArgs { uint64_t *out; const uint64_t *x; const uint64_t *m; const int8_t *e; unsigned W, logn, logq, negate; };

__global__ __launch_bounds__(256) void enc_tail_k(EncTailArgs a) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (1u << a.logn)) return;
  const size_t base = ((size_t)blockIdx.y * a.W << a.logn) + i;
  const uint64_t ev = a.e ? (uint64_t)(int64_t)a.e[((size_t)blockIdx.y << a.logn) + i] : 0;
  const uint64_t es = (uint64_t)((int64_t)ev >> 63), flip = a.negate ? ~0ull : 0;
  const unsigned sb = a.logq - 1;
  uint64_t carry = a.negate ? 1 : 0, qsign = 0;                                     // -x = ~x + 1
  for (unsigned j = 0; j < a.W; ++j) {
    const size_t o = base + ((size_t)j << a.logn);
    const unsigned __int128 t = (unsigned __int128)(a.x[o] ^ flip) + (a.m ? a.m[o] : 0) + (j ? es : ev) + carry;
    uint64_t v = (uint64_t)t;
    carry = (uint64_t)(t >> 64);
    const unsigned lo = 64 * j;
    if (lo + 64 > sb && lo <= sb) qsign = 0 - ((v >> (sb - lo)) & 1);
    if (lo >= a.logq) v = qsign;
    else if (lo + 64 > a.logq) {
      const uint64_t mask = (1ull << (a.logq - lo)) - 1;
      v = (v & mask) | (qsign & ~mask);
    }
    a.out[o] = v;
  }
}

}  // namespace gpq
