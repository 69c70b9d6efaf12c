// ecd_kernels.hpp -- he_ecd on the device (src/he-encode.c:53-64, :107-111; src/canemb.c:62-81): one workgroup encodes one slot vector in LDS
// (he_ecd_lds), or, for more slots than its LDS holds, three kernels share the vector (he_ecd_cols, he_ecd_block, he_ecd_slab, below).
//
// invcanemb is executed as the reference writes it: for len = slots, slots/2, .., 2 every pair (a, b) = (x[i+j], x[i+j+len/2]) becomes
// u = a + b, v = (a - b) * zetas[k] with k = (4 len - 5^j mod 4 len) * m / (4 len), then the bit reversal and the division by `slots`.
// The m-th roots the encoder reads are the 4 slots + 1 entries T[t] = zetas[t m / (4 slots)], which the CALLER supplies (gpq_ecd_plan_create):
// the kernel contains no trigonometry, so its words follow the caller's table under any libm.  5^j mod 4 len = (5^j mod 4 slots) mod 4 len,
// one uint32 table per plan.
//
// Every double operation below is rounded on its own, as gcc compiles the reference for x86-64 (no fused multiply-add): the complex product
// is (ac - bd, ad + bc) from four products, one difference and one sum.  hipcc contracts a*b + c into v_fma_f64 by default, which changes
// words (coefficients of 2^61: most of them at 64 slots and more), so contraction is off for this whole header.  Plain operators only: the
// __dmul_rn / __dadd_rn family is defined in the HIP headers, outside the pragma, and its operations DO fuse once inlined here.
//
// Scaling: x / slots and x * 2^logDelta are exact (powers of two); round() is C's (half away from zero), as src/he-encode.c:61-62.  A value
// that is not finite or whose magnitude reaches 2^63 has no defined image (src/types.c:225-245 is the identity below 2^64 only, and a
// W-word two's complement slab of the sign-extended int64 holds |v| < 2^63): it is stored as 0 and counted in *bad.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace gpq {

constexpr unsigned kEcdMaxSlots = 8192;     // per workgroup: 16 bytes per slot in LDS, 128 KiB of the CU's 160 KiB
constexpr unsigned kEcdMaxThreads = 1024;

struct EcdArgs {
  const double *src;        // n1 == 0: [count][slots] (re, im) pairs; n1 > 0: the slots x slots row-major matrix of (re, im) pairs
  uint64_t *out;            // [count][W][n]
  const double2 *roots;     // T[0 .. 4 slots], (re, im)
  const uint32_t *pow5;     // 5^j mod 4 slots, j < max(slots / 2, 1)
  uint32_t *bad;            // may be null
  double delta;             // 2^logDelta
  double inv_slots;         // 1 / slots
  unsigned slots, logslots, logn, W;
  unsigned n1;              // > 0: vector k of the call is zrotdiag(A, k, -(k - k % n1)) (src/he-algo.c:29-43, :63-72)
  // slots = 2^k B with B = 2^logblock < slots (he_ecd_cols, he_ecd_block, he_ecd_slab): the context's hand-off memory
  unsigned logblock;
  double2 *hand;            // [count][slots] (re, im): the vector after the k highest stages
  long long *ints;          // [count][2][slots]: the rounded real parts, then the rounded imaginary parts, by slot
};

// round(x / slots * Delta) as the int64 the slab stores; *offending counts what has no image
__device__ inline long long ecd_round(double x, const EcdArgs &a, unsigned *offending) {
  const double r = round(x * a.inv_slots * a.delta);
  if (!(fabs(r) < 9223372036854775808.0)) {       // NaN, infinity, |r| >= 2^63
    ++*offending;
    return 0;
  }
  return (long long)r;
}

// the element t of vector `vec` as the encoder reads it: the vector itself, or the rotated diagonal gathered from the matrix
__device__ inline double2 ecd_load(const EcdArgs &a, unsigned vec, unsigned t) {
  if (a.n1 == 0) return ((const double2 *)a.src)[(size_t)vec * a.slots + t];
  const unsigned shift = vec - vec % a.n1, mask = a.slots - 1;
  const unsigned u = (t + a.slots - shift) & mask;                 // rotdiag[t] = diag[(t - shift) mod slots], diag[u] = A[u][(vec + u) mod slots]
  return ((const double2 *)a.src)[(size_t)u * a.slots + ((vec + u) & mask)];
}

// one pair of src/canemb.c:71-72: u = a + b, v = (a - b) w, four products, one difference, one sum: contraction is off
__device__ inline void ecd_bfly(double &ar, double &ai, double &br, double &bi, const double2 w) {
  const double dr = ar - br, di = ai - bi, sr = ar + br, si = ai + bi;
  ar = sr;
  ai = si;
  br = dr * w.x - di * w.y;
  bi = dr * w.y + di * w.x;
}

// the root of pair j < len/2 of the stage len = 2^loglen (src/canemb.c:70), in the plan's table for 2^logslots slots
__device__ inline double2 ecd_root(const EcdArgs &a, unsigned j, unsigned loglen) {
  const unsigned idx_mask = (4u << loglen) - 1;
  return a.roots[((idx_mask + 1) - (a.pow5[j] & idx_mask)) << (a.logslots - loglen)];
}

// src/canemb.c:64-77 for len = 2^top, .., 2 on the 2^top values in LDS: the pairs of one stage are disjoint, so each stage is in place
// behind one barrier.  Every group of 2^top consecutive elements of the vector runs the same pairs with the same roots.
__device__ inline void ecd_stages_lds(double *re, double *im, const EcdArgs &a, unsigned top, unsigned tid, unsigned nthreads) {
  const unsigned half = (1u << top) >> 1;
  for (unsigned loglen = top; loglen >= 1; --loglen) {
    const unsigned mid = 1u << (loglen - 1);
    for (unsigned b = tid; b < half; b += nthreads) {
      const unsigned j = b & (mid - 1), lo = ((b >> (loglen - 1)) << loglen) + j, hi = lo + mid;
      ecd_bfly(re[lo], im[lo], re[hi], im[hi], ecd_root(a, j, loglen));
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kEcdMaxThreads) he_ecd_lds(EcdArgs a) {
  extern __shared__ double ecd_lds[];
  double *re = ecd_lds, *im = ecd_lds + a.slots;
  const unsigned slots = a.slots, vec = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  for (unsigned t = tid; t < slots; t += nthreads) { const double2 v = ecd_load(a, vec, t); re[t] = v.x; im[t] = v.y; }
  __syncthreads();
  ecd_stages_lds(re, im, a, a.logslots, tid, nthreads);
  // bit reversal (:78), / slots (:79-80), * Delta and round (src/he-encode.c:61-62): slot i takes x[brv(i)]; the integers replace the doubles
  // in place, pair by pair
  unsigned offending = 0;
  long long *ire = (long long *)re, *iim = (long long *)im;
  for (unsigned i = tid; i < slots; i += nthreads) {
    const unsigned j = a.logslots ? __brev(i) >> (32 - a.logslots) : 0;
    if (j < i) continue;
    const double xr = re[i], xi = im[i], yr = re[j], yi = im[j];
    ire[i] = ecd_round(yr, a, &offending); iim[i] = ecd_round(yi, a, &offending);
    if (j != i) { ire[j] = ecd_round(xr, a, &offending); iim[j] = ecd_round(xi, a, &offending); }
  }
  if (offending && a.bad) atomicAdd(a.bad, offending);
  __syncthreads();
  // the whole [W][n] slab of this vector, every word once: slot i at coefficient i gap (real part) and i gap + n/2 (imaginary part)
  // as W sign-extended words, zero everywhere else
  const unsigned n = 1u << a.logn, loggap = a.logn - 1 - a.logslots, gap_mask = (1u << loggap) - 1, nh_mask = (n >> 1) - 1;
  uint64_t *out = a.out + (size_t)vec * a.W * n;
  const unsigned total = a.W << a.logn;
  for (unsigned e = tid; e < total; e += nthreads) {
    const unsigned coeff = e & (n - 1), word = e >> a.logn;
    uint64_t v = 0;
    if ((coeff & gap_mask) == 0) {
      const unsigned slot = (coeff & nh_mask) >> loggap;
      const long long x = (coeff >> (a.logn - 1)) ? iim[slot] : ire[slot];
      v = word ? (uint64_t)(x >> 63) : (uint64_t)x;
    }
    out[e] = v;
  }
}

// ---- more slots than one workgroup holds: slots = 2^LK B, three kernels ------------------------------------------------------------------
// (a) he_ecd_cols: the LK highest stages, len = slots .. 2 B.  len/2 is a multiple of B there, so element h B + r meets only elements of
//     its own column r: a lane owns one column, 2^LK values in registers, and consecutive lanes take consecutive r (16-byte accesses, 1 KiB
//     per wave).  The pair (h, h + lenh/2) of the column, lenh = 2^(LK - s), is the pair j = (h mod lenh/2) B + r of the stage len = slots >> s.
// (b) he_ecd_block: the stages len = B .. 2 stay inside the B consecutive elements of one block: ecd_stages_lds on one block per workgroup.
//     The bit reversal of position b B + r is brv_B(r) 2^LK + brv_LK(b): that slot's rounded pair goes to `ints` ([slots] real parts, then
//     [slots] imaginary parts) in natural slot order.
// (c) he_ecd_slab: every word of [W][n] once, two coefficients (16 bytes) per lane and word, from `ints`.
constexpr unsigned kEcdMaxSplit = 3;        // slots / B <= 8
constexpr unsigned kEcdColThreads = 256, kEcdSlabThreads = 256;

template <unsigned LK>
__global__ void __launch_bounds__(kEcdColThreads) he_ecd_cols(EcdArgs a) {
  constexpr unsigned K = 1u << LK;
  const unsigned B = 1u << a.logblock, r = blockIdx.y * blockDim.x + threadIdx.x, vec = blockIdx.x;
  if (r >= B) return;
  double xr[K], xi[K];
#pragma unroll
  for (unsigned h = 0; h < K; ++h) { const double2 v = ecd_load(a, vec, (h << a.logblock) + r); xr[h] = v.x; xi[h] = v.y; }
#pragma unroll
  for (unsigned s = 0; s < LK; ++s) {
    const unsigned half = K >> (s + 1);
#pragma unroll
    for (unsigned p = 0; p < K / 2; ++p) {
      const unsigned jh = p & (half - 1), lo = ((p / half) * 2 * half) + jh, hi = lo + half;
      ecd_bfly(xr[lo], xi[lo], xr[hi], xi[hi], ecd_root(a, (jh << a.logblock) + r, a.logslots - s));
    }
  }
  double2 *hand = a.hand + (size_t)vec * a.slots;
#pragma unroll
  for (unsigned h = 0; h < K; ++h) hand[(h << a.logblock) + r] = make_double2(xr[h], xi[h]);
}

__global__ void __launch_bounds__(kEcdMaxThreads) he_ecd_block(EcdArgs a) {
  extern __shared__ double ecd_block_lds[];
  const unsigned B = 1u << a.logblock, lk = a.logslots - a.logblock;
  double *re = ecd_block_lds, *im = ecd_block_lds + B;
  const unsigned blk = blockIdx.y, vec = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  const double2 *hand = a.hand + (size_t)vec * a.slots + ((size_t)blk << a.logblock);
  for (unsigned t = tid; t < B; t += nthreads) { const double2 v = hand[t]; re[t] = v.x; im[t] = v.y; }
  __syncthreads();
  ecd_stages_lds(re, im, a, a.logblock, tid, nthreads);
  unsigned offending = 0;
  long long *ire = a.ints + (size_t)vec * 2 * a.slots, *iim = ire + a.slots;
  const unsigned low = __brev(blk) >> (32 - lk);                   // lk >= 1
  for (unsigned t = tid; t < B; t += nthreads) {
    const unsigned slot = ((a.logblock ? __brev(t) >> (32 - a.logblock) : 0) << lk) + low;
    ire[slot] = ecd_round(re[t], a, &offending);
    iim[slot] = ecd_round(im[t], a, &offending);
  }
  if (offending && a.bad) atomicAdd(a.bad, offending);
}

__global__ void __launch_bounds__(kEcdSlabThreads) he_ecd_slab(EcdArgs a) {
  const unsigned n = 1u << a.logn, loggap = a.logn - 1 - a.logslots, gap_mask = (1u << loggap) - 1, nh_mask = (n >> 1) - 1;
  const unsigned coeff = 2 * (blockIdx.y * blockDim.x + threadIdx.x), vec = blockIdx.x;          // n is even: a pair never straddles a word
  if (coeff >= n) return;
  const long long *part = a.ints + (size_t)vec * 2 * a.slots + ((coeff >> (a.logn - 1)) ? a.slots : 0);
  long long x0 = 0, x1 = 0;
  if ((coeff & gap_mask) == 0) {
    const unsigned slot = (coeff & nh_mask) >> loggap;
    x0 = part[slot];
    if (loggap == 0) x1 = part[slot + 1];                          // gap 1: the odd coefficient is a slot too (slots >= 2 in this path)
  }
  ulonglong2 *out = (ulonglong2 *)(a.out + (size_t)vec * a.W * n + coeff);
  out[0] = make_ulonglong2((unsigned long long)x0, (unsigned long long)x1);
  const ulonglong2 ext = make_ulonglong2((unsigned long long)(x0 >> 63), (unsigned long long)(x1 >> 63));
  for (unsigned word = 1; word < a.W; ++word) out[(size_t)word << (a.logn - 1)] = ext;
}

}  // namespace gpq
