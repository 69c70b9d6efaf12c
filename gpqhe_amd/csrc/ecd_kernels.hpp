// ecd_kernels.hpp -- he_ecd on the device (src/he-encode.c:53-64, :107-111; src/canemb.c:62-81): one workgroup encodes one slot vector in LDS.
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

constexpr unsigned kEcdMaxSlots = 8192;     // 16 bytes per slot in LDS: 128 KiB of the CU's 160 KiB
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

__global__ void __launch_bounds__(kEcdMaxThreads) he_ecd_lds(EcdArgs a) {
  extern __shared__ double ecd_lds[];
  double *re = ecd_lds, *im = ecd_lds + a.slots;
  const unsigned slots = a.slots, vec = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  // load: the vector itself, or the rotated diagonal gathered from the matrix
  if (a.n1 == 0) {
    const double2 *z = (const double2 *)a.src + (size_t)vec * slots;
    for (unsigned t = tid; t < slots; t += nthreads) { const double2 v = z[t]; re[t] = v.x; im[t] = v.y; }
  } else {
    const double2 *A = (const double2 *)a.src;
    const unsigned shift = vec - vec % a.n1, mask = slots - 1;
    for (unsigned t = tid; t < slots; t += nthreads) {
      const unsigned u = (t + slots - shift) & mask;             // rotdiag[t] = diag[(t - shift) mod slots], diag[u] = A[u][(vec + u) mod slots]
      const double2 v = A[(size_t)u * slots + ((vec + u) & mask)];
      re[t] = v.x; im[t] = v.y;
    }
  }
  __syncthreads();
  // src/canemb.c:64-77: the pairs of one stage are disjoint, so each stage is in place behind one barrier
  const unsigned half = slots >> 1;
  for (unsigned loglen = a.logslots; loglen >= 1; --loglen) {
    const unsigned mid = 1u << (loglen - 1), idx_mask = (4u << loglen) - 1, tstride = a.logslots - loglen;
    for (unsigned b = tid; b < half; b += nthreads) {
      const unsigned j = b & (mid - 1), lo = ((b >> (loglen - 1)) << loglen) + j, hi = lo + mid;
      const unsigned k = ((idx_mask + 1) - (a.pow5[j] & idx_mask)) << tstride;
      const double2 w = a.roots[k];
      const double ar = re[lo], ai = im[lo], br = re[hi], bi = im[hi];
      const double dr = ar - br, di = ai - bi;
      re[lo] = ar + br;
      im[lo] = ai + bi;
      re[hi] = dr * w.x - di * w.y;                              // four products, one difference, one sum: contraction is off
      im[hi] = dr * w.y + di * w.x;
    }
    __syncthreads();
  }
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

}  // namespace gpq
