// dcd_kernels.hpp -- he_dcd on the device (src/he-encode.c:66-74, :114-117; src/canemb.c:43-60): one workgroup decodes one plaintext in LDS
// (he_dcd_lds), or, for more slots than its LDS holds, one workgroup per block and then one lane per column (he_dcd_block, he_dcd_cols, below).
// he_ecd_lds (ecd_kernels.hpp) run the other way, on the same plan: the root table T[t] = zetas[t m / (4 slots)] the CALLER supplied and the
// table 5^j mod 4 slots.  The kernel contains no trigonometry.
//
// (a) gather: slot i reads coefficient i gap (real part) and i gap + n/2 (imaginary part), gap = n / (2 slots); word j of a coefficient at
//     j n.  2 slots W words are read, nothing else of the slab.
// (b) mpi_to_double (src/types.c:77-106) is `num = num * 2 + bit` from the top bit down in double arithmetic -- neither correctly rounded
//     nor truncating.  For a magnitude of L bits: L <= 53 is exact.  Beyond that the first 53 bits M are exact; the 54th bit b makes
//     2 M + b, a tie between 2 M and 2 M + 2 that round-to-nearest-even resolves to the even mantissa: M' = M + (b & M & 1).  Every later bit
//     is at most a quarter of the last place and rounds away.  The result is M' 2^(L - 53), +inf once that reaches 2^1024 (a 32-word slab
//     can).  The sign is applied last (:94).  The magnitude of a negative coefficient is the multiword negation read as unsigned, so that
//     -2^(64 W - 1) has its image.
// (c) x / nu with the IEEE-rounded division, real and imaginary part on their own: nu is a general double after he_mul / he_rs, and a
//     product with the reciprocal differs in the last place.
// (d) canemb: bit reversal, then for len = 2, 4, .., slots every pair (u, b) = (x[i+j], x[i+j+len/2]) becomes u + v, u - v with
//     v = b * zetas[(5^j mod 4 len) m / (4 len)] = b * T[(5^j mod 4 len) << (logslots - loglen)].
//
// Every double operation is rounded on its own, as gcc compiles the reference for x86-64 (no fused multiply-add): the complex product is
// (ac - bd, ad + bc) from four products, one difference and one sum.  Contraction is off for this whole header and the arithmetic uses
// plain operators only, for the reasons at the top of ecd_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecd_kernels.hpp"

#pragma clang fp contract(off)

namespace gpq {

struct DcdArgs {
  const uint64_t *in;       // [count][W][n], two's complement
  double *out;              // [count][slots] (re, im) pairs
  const double2 *roots;     // T[0 .. 4 slots], (re, im)
  const uint32_t *pow5;     // 5^j mod 4 slots, j < max(slots / 2, 1)
  double nu;
  unsigned slots, logslots, logn, W;
  unsigned logblock;        // slots = 2^k B with B = 2^logblock < slots: he_dcd_block, he_dcd_cols
};

// mpi_to_double of the W-word two's complement integer whose word j is at words[j << logn]
__device__ inline double dcd_to_double(const uint64_t *words, unsigned logn, unsigned W) {
  const bool neg = (words[(size_t)(W - 1) << logn] >> 63) != 0;
  // the magnitude word by word from the bottom (the carry of the negation lasts while the words below are zero); only the highest
  // non-zero word `hi`, the word below it `lo` and its index `top` are kept
  uint64_t hi = 0, lo = 0, below = 0;
  unsigned top = 0;
  bool carry = true;
  for (unsigned j = 0; j < W; ++j) {
    const uint64_t x = words[(size_t)j << logn];
    uint64_t m = x;
    if (neg) { m = ~x + (carry ? 1u : 0u); carry = carry && x == 0; }
    if (m) { hi = m; lo = below; top = j; }
    below = m;
  }
  if (!hi) return 0.0;                                               // :82-83 (+0: a negative value is never zero)
  const unsigned hbits = 64u - (unsigned)__clzll((long long)hi), L = 64u * top + hbits;
  double num;
  if (L <= 53) {
    num = (double)hi;                                                // exact
  } else {
    // the top 54 bits of the magnitude from the 128-bit window (hi, lo) (top > 0) or (0, hi)
    const unsigned __int128 win = top ? (((unsigned __int128)hi << 64) | lo) : (unsigned __int128)hi;
    const unsigned wbits = top ? 64u + hbits : hbits;                // >= 54
    const uint64_t t54 = (uint64_t)(win >> (wbits - 54u));
    const uint64_t M = t54 >> 1, b = t54 & 1u;
    const uint64_t Mr = M + (b & M & 1u);                            // <= 2^53: exact as a double
    const unsigned e = L - 53u;
    if (e > 1023u) {
      num = __longlong_as_double(0x7ff0000000000000ll);              // at least 2^(L-1) >= 2^1076
    } else {
      const double scale = __longlong_as_double((long long)(e + 1023u) << 52);   // 2^e, a normal double
      num = (double)Mr * scale;                                      // exact below 2^1024, +inf from there
    }
  }
  return neg ? -num : num;
}

// one pair of src/canemb.c:54-56: v = b w, then u + v and u - v; four products, one difference, one sum: contraction is off
__device__ inline void dcd_bfly(double &ur, double &ui, double &br, double &bi, const double2 w) {
  const double vr = br * w.x - bi * w.y;
  const double vi = br * w.y + bi * w.x;
  const double sr = ur + vr, si = ui + vi, dr = ur - vr, di = ui - vi;
  ur = sr;
  ui = si;
  br = dr;
  bi = di;
}

// the root of pair j < len/2 of the stage len = 2^loglen (src/canemb.c:52), in the plan's table for 2^logslots slots
__device__ inline double2 dcd_root(const DcdArgs &a, unsigned j, unsigned loglen) {
  return a.roots[(a.pow5[j] & ((4u << loglen) - 1)) << (a.logslots - loglen)];
}

// src/canemb.c:46-59 for len = 2, .., 2^top on the 2^top values in LDS: the pairs of one stage are disjoint, so each stage is in place
// behind one barrier
__device__ inline void dcd_stages_lds(double *re, double *im, const DcdArgs &a, unsigned top, unsigned tid, unsigned nthreads) {
  const unsigned half = (1u << top) >> 1;
  for (unsigned loglen = 1; loglen <= top; ++loglen) {
    const unsigned mid = 1u << (loglen - 1);
    for (unsigned b = tid; b < half; b += nthreads) {
      const unsigned j = b & (mid - 1), lo = ((b >> (loglen - 1)) << loglen) + j, hi = lo + mid;
      dcd_bfly(re[lo], im[lo], re[hi], im[hi], dcd_root(a, j, loglen));
    }
    __syncthreads();
  }
}

// (a)-(c) for part (0: real, 1: imaginary) of slot i of plaintext `in`
__device__ inline double dcd_slot(const DcdArgs &a, const uint64_t *in, unsigned i, unsigned part) {
  const unsigned coeff = (i << (a.logn - 1 - a.logslots)) + (part << (a.logn - 1));
  return dcd_to_double(in + coeff, a.logn, a.W) / a.nu;
}

__global__ void __launch_bounds__(kEcdMaxThreads) he_dcd_lds(DcdArgs a) {
  extern __shared__ double dcd_lds[];
  double *re = dcd_lds, *im = dcd_lds + a.slots;
  const unsigned slots = a.slots, pt = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  const uint64_t *in = a.in + (((size_t)pt * a.W) << a.logn);
  // (a)-(c), and the bit reversal of (d) on the way in: bitrev_vec leaves old[brv(i)] at i, so slot i is stored at brv(i)
  for (unsigned e = tid; e < 2 * slots; e += nthreads) {
    const unsigned i = e & (slots - 1), part = e >> a.logslots;
    const double x = dcd_slot(a, in, i, part);
    const unsigned r = a.logslots ? __brev(i) >> (32 - a.logslots) : 0;
    (part ? im : re)[r] = x;
  }
  __syncthreads();
  dcd_stages_lds(re, im, a, a.logslots, tid, nthreads);
  double2 *out = (double2 *)a.out + (size_t)pt * slots;
  for (unsigned i = tid; i < slots; i += nthreads) out[i] = make_double2(re[i], im[i]);
}

// ---- more slots than one workgroup holds: slots = 2^LK B, two kernels, the mirror of ecd_kernels.hpp's --------------------------------------
// (a') he_dcd_block: position b B + r of the bit-reversed vector is slot brv_B(r) 2^LK + brv_LK(b), so block b gathers the slots
//      i = q 2^LK + brv_LK(b), converts and divides them as above, stores slot q's at brv_B(q), runs the stages len = 2 .. B in LDS and
//      writes its B values to z at b B.
// (b') he_dcd_cols: the stages len = 2 B .. slots pair element h B + r only with elements of its own column r: a lane owns one column,
//      2^LK values in registers, read from and written to z in place (16-byte accesses, consecutive lanes consecutive r).  The pair
//      (h, h + lenh/2) of the column, lenh = 2^s, is the pair j = (h mod lenh/2) B + r of the stage len = 2^s B.
__global__ void __launch_bounds__(kEcdMaxThreads) he_dcd_block(DcdArgs a) {
  extern __shared__ double dcd_block_lds[];
  const unsigned B = 1u << a.logblock, lk = a.logslots - a.logblock;
  double *re = dcd_block_lds, *im = dcd_block_lds + B;
  const unsigned blk = blockIdx.y, pt = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  const uint64_t *in = a.in + (((size_t)pt * a.W) << a.logn);
  const unsigned low = __brev(blk) >> (32 - lk);                   // lk >= 1
  for (unsigned e = tid; e < 2 * B; e += nthreads) {
    const unsigned q = e & (B - 1), part = e >> a.logblock;
    const double x = dcd_slot(a, in, (q << lk) + low, part);
    const unsigned r = a.logblock ? __brev(q) >> (32 - a.logblock) : 0;
    (part ? im : re)[r] = x;
  }
  __syncthreads();
  dcd_stages_lds(re, im, a, a.logblock, tid, nthreads);
  double2 *out = (double2 *)a.out + (size_t)pt * a.slots + ((size_t)blk << a.logblock);
  for (unsigned t = tid; t < B; t += nthreads) out[t] = make_double2(re[t], im[t]);
}

template <unsigned LK>
__global__ void __launch_bounds__(kEcdColThreads) he_dcd_cols(DcdArgs a) {
  constexpr unsigned K = 1u << LK;
  const unsigned B = 1u << a.logblock, r = blockIdx.y * blockDim.x + threadIdx.x, pt = blockIdx.x;
  if (r >= B) return;
  double2 *z = (double2 *)a.out + (size_t)pt * a.slots;
  double xr[K], xi[K];
#pragma unroll
  for (unsigned h = 0; h < K; ++h) { const double2 v = z[(h << a.logblock) + r]; xr[h] = v.x; xi[h] = v.y; }
#pragma unroll
  for (unsigned s = 1; s <= LK; ++s) {
    const unsigned half = 1u << (s - 1);
#pragma unroll
    for (unsigned p = 0; p < K / 2; ++p) {
      const unsigned jh = p & (half - 1), lo = ((p / half) * 2 * half) + jh, hi = lo + half;
      dcd_bfly(xr[lo], xi[lo], xr[hi], xi[hi], dcd_root(a, (jh << a.logblock) + r, a.logblock + s));
    }
  }
#pragma unroll
  for (unsigned h = 0; h < K; ++h) z[(h << a.logblock) + r] = make_double2(xr[h], xi[h]);
}

}  // namespace gpq
