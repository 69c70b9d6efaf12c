// constpt_kernels.hpp -- device fragment of bridge.hip: he_mulpt / he_addpt / he_subpt by the plaintext of he_const_pt
// (src/he-encode.c:119-125), m = a + b x^h with h = n/2 and every other coefficient 0.  In Z[x]/(x^n + 1) the product with a coefficient
// vector c is
//   v[k]     = a c[k]     - b c[k + h]
//   v[k + h] = a c[k + h] + b c[k]             (k < h)
// so he_mulpt (src/he-mult.c:159-196) needs no residue, no transform and no CRT: out = smod(v, 2^logql) is one pass over the big slabs.
// With he_rs behind it (src/he-rescale.c:33-54, Delta = 2^s, 1 <= s <= 63) the result is smod(rdiv(smod(v, 2^logql), 2^s), 2^(logql - s)); the
// inner smod changes v by a multiple of 2^logql, which rdiv carries to a multiple of 2^(logql - s) (the remainder mod 2^s is untouched, s < logql),
// and the outer smod drops it: bits [0, logql - s) of the result are bits [s, logql) of v plus rescale_coefficient's rounding carry.
// Big slabs are word-major (word j of coefficient i at j n + i): threads run along i, so every word plane a wavefront touches is one
// contiguous run of 8-byte words, as in bridge_big_addsub.  Words are walked in ascending order and a word is written only after the next
// one of the same coefficients was read, so out may be the input of the same polynomial.
#pragma once
namespace gpq {

// +-x times a 64-bit magnitude, word by word (two's complement, wrapping at 2^(64 W)): the negation's carry and the product's high word ride along
struct ScaledWords {
  uint64_t hi;
  unsigned negc;
  __device__ __forceinline__ explicit ScaledWords(unsigned neg) : hi(0), negc(neg) {}
  __device__ __forceinline__ uint64_t next(uint64_t x, uint64_t mag, unsigned neg) {
    if (neg) { x = ~x + negc; negc &= x == 0; }            // -x = ~x + 1
    const uint64_t lo = mag * x, w = lo + hi;
    hi = __umul64hi(mag, x) + (w < lo);                     // mag x + hi < 2^128
    return w;
  }
};

// word j of a coefficient that is centred mod 2^logql: the low logql bits kept, sign-extended from bit logql - 1.  qsign is set by the word
// that holds that bit and read by the words above it (ascending j).
__device__ __forceinline__ uint64_t centre_word(uint64_t v, unsigned j, unsigned logql, uint64_t &qsign) {
  const unsigned sb = logql - 1, base = 64 * j;
  if (base + 64 > sb && base <= sb) qsign = 0 - ((v >> (sb - base)) & 1);
  if (base >= logql) return qsign;
  if (base + 64 > logql) {
    const uint64_t mask = (1ull << (logql - base)) - 1;
    return (v & mask) | (qsign & ~mask);
  }
  return v;
}

// The words of v on their way out: shifted right by s with rescale_coefficient's rounding (remainder > 2^(s-1): bit s-1 set and a lower bit
// set; both lie in word 0 for s <= 63), centred mod 2^lq.  s = 0: the plain smod.  Word j leaves when word j + 1 of v is known.
struct RescaledOut {
  uint64_t prev, carry, qsign;
  __device__ __forceinline__ RescaledOut() : prev(0), carry(0), qsign(0) {}
  __device__ __forceinline__ uint64_t word(unsigned j, uint64_t next, unsigned s, unsigned lq) {
    uint64_t w = prev;
    if (s) {
      w = (prev >> s) | (next << (64 - s));
      if (j == 0) carry = ((prev >> (s - 1)) & 1) && (prev & ((1ull << (s - 1)) - 1));
    }
    const uint64_t w1 = w + carry;
    carry = w1 < w;
    prev = next;
    return centre_word(w1, j, lq, qsign);
  }
};

// is the coefficient read so far the sign extension of its low logql bits?  (what every call of this library returns for q_l = 2^logql)
struct CentredCheck {
  uint64_t ext;
  unsigned bad;
  __device__ __forceinline__ CentredCheck() : ext(0), bad(0) {}
  __device__ __forceinline__ void word(uint64_t x, unsigned j, unsigned logql) {
    const unsigned sb = logql - 1, js = sb >> 6, bit = sb & 63;
    if (j == js) { ext = 0 - ((x >> bit) & 1); bad |= ((x ^ ext) >> bit) != 0; }
    else if (j > js) bad |= x != ext;
  }
};

struct MulptConstArgs {
  uint64_t *out0, *out1;          // c0 / c1 of the batch: [batch][W][n]
  const uint64_t *in0, *in1;
  uint64_t ma, mb;                // |a|, |b|
  unsigned na, nb;                // a < 0, b < 0
  unsigned W, logn, s, logql;     // s = log2(Delta) of the fused he_rs (0: none)
  unsigned *bad;                  // nullptr, or the counter of non-centred input coefficients
};

// B = false (b == 0, the usual case): one thread per coefficient, out = a c.  B = true: one thread per pair (k, k + h).
// Grid y = 2 ciphertext + (0: c0, 1: c1).
template <bool B>
__global__ __launch_bounds__(256) void he_mulpt_const(MulptConstArgs a) {
  const unsigned n = 1u << a.logn, h = n >> 1, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= (B ? h : n)) return;
  const size_t base = ((size_t)(blockIdx.y >> 1) * a.W << a.logn) + k;
  const uint64_t *in = ((blockIdx.y & 1) ? a.in1 : a.in0) + base;      // (may be out: no __restrict__)
  uint64_t *out = ((blockIdx.y & 1) ? a.out1 : a.out0) + base;
  const unsigned lq = a.logql - a.s;
  const bool chk = a.bad != nullptr;                                   // (uniform)
  ScaledWords ax(a.na), ay(a.na), bx(a.nb), by(a.nb ^ 1u);             // a c[k], a c[k+h], b c[k], -b c[k+h]
  RescaledOut lo, hi;
  CentredCheck cx, cy;
  unsigned clo = 0, chi = 0;
  uint64_t x = in[0], y = B ? in[h] : 0;
  for (unsigned j = 0; j < a.W; ++j) {
    uint64_t xn = 0, yn = 0;                                           // the next words are read before this step's stores
    if (j + 1 < a.W) {
      xn = in[(size_t)(j + 1) << a.logn];
      if (B) yn = in[((size_t)(j + 1) << a.logn) + h];
    }
    if (chk) { cx.word(x, j, a.logql); if (B) cy.word(y, j, a.logql); }
    uint64_t vlo = ax.next(x, a.ma, a.na), vhi = 0;
    if (B) {
      const uint64_t t = by.next(y, a.mb, a.nb ^ 1u), s1 = vlo + t, s2 = s1 + clo;
      clo = (s1 < vlo) | (s2 < s1);
      vlo = s2;
      const uint64_t u = ay.next(y, a.ma, a.na), r = bx.next(x, a.mb, a.nb), r1 = u + r, r2 = r1 + chi;
      chi = (r1 < u) | (r2 < r1);
      vhi = r2;
    }
    if (j) {
      out[(size_t)(j - 1) << a.logn] = lo.word(j - 1, vlo, a.s, lq);
      if (B) out[((size_t)(j - 1) << a.logn) + h] = hi.word(j - 1, vhi, a.s, lq);
    } else {
      lo.prev = vlo;
      hi.prev = vhi;
    }
    x = xn;
    y = yn;
  }
  // the last word: bits from beyond word W - 1 would land at 64 W - s >= logql - s and above, which centre_word replaces
  out[(size_t)(a.W - 1) << a.logn] = lo.word(a.W - 1, 0, a.s, lq);
  if (B) out[((size_t)(a.W - 1) << a.logn) + h] = hi.word(a.W - 1, 0, a.s, lq);
  if (chk) {
    const unsigned cnt = cx.bad + cy.bad;
    if (cnt) atomicAdd(a.bad, cnt);
  }
}

struct AddptConstArgs {
  uint64_t *out0, *out1;
  const uint64_t *in0, *in1;
  int64_t a, b;
  unsigned sub, W, logn, logql;
};

// he_addpt / he_subpt (src/he-add.c:80-123): out_c0 = smod(c0 +- m, 2^logql), out_c1 = smod(c1, 2^logql); m has two coefficients.
// One thread per coefficient, grid y as above.  c - t = c + ~t + 1 on the sign-extended words of t, so t = INT64_MIN needs no care.
__global__ __launch_bounds__(256) void he_addpt_const(AddptConstArgs a) {
  const unsigned n = 1u << a.logn, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t base = ((size_t)(blockIdx.y >> 1) * a.W << a.logn) + i;
  const bool c1 = blockIdx.y & 1;
  const uint64_t *in = (c1 ? a.in1 : a.in0) + base;
  uint64_t *out = (c1 ? a.out1 : a.out0) + base;
  const int64_t t = c1 ? 0 : i == 0 ? a.a : i == (n >> 1) ? a.b : 0;
  const bool neg = a.sub && t != 0;
  const uint64_t t0 = neg ? ~(uint64_t)t : (uint64_t)t, text = neg ? ~(uint64_t)(t >> 63) : (uint64_t)(t >> 63);
  unsigned carry = neg ? 1u : 0u;
  uint64_t qsign = 0;
  for (unsigned j = 0; j < a.W; ++j) {
    const uint64_t x = in[(size_t)j << a.logn], y = j ? text : t0, s1 = x + y, s2 = s1 + carry;
    carry = (s1 < x) | (s2 < s1);
    out[(size_t)j << a.logn] = centre_word(s2, j, a.logql, qsign);
  }
}

}  // namespace gpq
