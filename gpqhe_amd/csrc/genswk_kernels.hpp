// genswk_kernels.hpp -- device side of gpq_he_genswk_batch (bridge_genswk.hpp): the kernel genswk_crt_tail.
//
// he_genswk (src/he-kem.c:96-101) reduces -p1 sk + e + P sp and p1 modulo M = P 2^k (k = logqL).  With X = p1 sk as poly_rns2mpi
// delivers it (centred mod P', the product of the dimmul primes, P | P'), the value v = -X + e + P sp mod M is fixed by CRT over the
// coprime pair (P, 2^k):
//   a  = v mod P   = (e - aX) mod P,                 aX = X mod P in [0, P): the CRT of the first dimP limbs of the product slab
//   z2 = v mod 2^k = (-c2 + e + P sp) mod 2^k,       c2 = X mod 2^k: the low words of the CRT of all dimmul limbs
//   v  = a + P h,  h = (z2 - a) P^-1 mod 2^k  in [0, 2^k)
// and mpi_smod's centring  v >= floor(M/2) = P 2^(k-1)  ->  v - M  holds exactly when bit k-1 of h is set (a < P), i.e. the key
// coefficient is a + P hs with hs = h read as a signed k-bit integer.  p1 itself is a raw sample below 2^nbits <= 2M: it loses
// [p1 >= floor(M/2)] + [p1 >= M + floor(M/2)] times M.
//
// One lane per coefficient.  Its multiword operands live in LDS as [word][lane] planes (64-bit words of consecutive lanes: no bank
// conflicts, no lane reads another's column, so the kernel has no barrier); every loop runs over run-time word counts and there is no
// per-thread array.  The three products (P sp low, (z2 - a) P^-1 low, P hs) are formed column by column in a three-word accumulator
// and each result word is stored as it completes.  The lane body is host-callable so that a CPU build can run it word for word.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gpq {

constexpr unsigned kGenswkKeysPerLaunch = 32;   // Galois elements travel as kernel arguments: no upload, nothing for a graph to re-read

struct GenswkTailArgs {
  const uint64_t *aX;        // [keys][WP][n]   X mod P in [0, P)
  const uint64_t *c2;        // [keys][W2][n]   X centred mod 2^k (the low k bits are what counts)
  const int8_t *e;           // [keys][n]
  const uint64_t *p1;        // [keys][W][n]    the raw sample
  const int8_t *sk_small;    // [n]             gathered form: the secret
  const uint64_t *sp;        // [keys][Wsp][n]  slab form: the hidden polynomials
  uint64_t *p0, *p1c;        // [keys][W][n]
  const uint64_t *P, *Pinv;  // P[WP];  P^-1 mod 2^(64 W2) [W2]
  const uint64_t *M, *Mh, *M3h;   // P 2^k, floor(M/2), M + floor(M/2): [LM] each
  unsigned WP, W2, W, Wsp, LM, logn, k;
  unsigned ginv[kGenswkKeysPerLaunch];   // gathered form: g^-1 mod 2n of each key of the launch
};

typedef unsigned __int128 gs_u128;

// (c2 : c1 : c0) += x * y
__host__ __device__ __forceinline__ void gs_mac(uint64_t &c0, uint64_t &c1, uint64_t &c2, uint64_t x, uint64_t y) {
  const gs_u128 p = (gs_u128)x * y;
  gs_u128 s = (gs_u128)c0 + (uint64_t)p;
  c0 = (uint64_t)s;
  s = (gs_u128)c1 + (uint64_t)(p >> 64) + (uint64_t)(s >> 64);
  c1 = (uint64_t)s;
  c2 += (uint64_t)(s >> 64);
}

// `lds`: this lane's column of the planes, words S apart; (WP + 3 W2 + W) words per lane
template <bool GATHER>
__host__ __device__ inline void genswk_tail_lane(const GenswkTailArgs &a, unsigned key, unsigned i, uint64_t *lds, unsigned S) {
  const unsigned WP = a.WP, W2 = a.W2, W = a.W, logn = a.logn;
  const size_t n = (size_t)1 << logn;
  uint64_t *A = lds, *SP = A + (size_t)WP * S, *D = SP + (size_t)W2 * S, *H = D + (size_t)W2 * S, *Q = H + (size_t)W2 * S;
  const int64_t ev = a.e[(size_t)key * n + i];
  const uint64_t esign = (uint64_t)(ev >> 63);

  // a = (e - aX) mod P: e - aX lies in [-P - 10, 11], so P is added at most twice
  {
    const uint64_t *ax = a.aX + ((size_t)key * WP << logn) + i;
    uint64_t borrow = 0;
    for (unsigned j = 0; j < WP; ++j) {
      const gs_u128 t = (gs_u128)(j ? esign : (uint64_t)ev) - ax[(size_t)j << logn] - borrow;
      A[(size_t)j * S] = (uint64_t)t;
      borrow = (uint64_t)(t >> 64) & 1;
    }
    int64_t top = (int64_t)esign - (int64_t)borrow;            // the word above: 0, -1 or -2
    for (int round = 0; round < 2; ++round) {
      const uint64_t m = top < 0 ? ~0ull : 0;
      uint64_t carry = 0;
      for (unsigned j = 0; j < WP; ++j) {
        const gs_u128 t = (gs_u128)A[(size_t)j * S] + (a.P[j] & m) + carry;
        A[(size_t)j * S] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
      }
      top += (int64_t)carry;
    }
  }

  // D = -c2 + e + P sp - a  (mod 2^(64 W2); the bits from k on are never read)
  {
    const uint64_t *c2 = a.c2 + ((size_t)key * W2 << logn) + i;
    uint64_t mag = 0, neg = 0;
    if (GATHER) {                                              // sp[i] = sk[i'] or -sk[i' - n], i' = i g^-1 mod 2n
      const unsigned src = (unsigned)(((uint64_t)i * a.ginv[key]) & (2 * n - 1));
      int v = a.sk_small[src & (n - 1)];
      if (src >= n) v = -v;
      neg = v < 0 ? ~0ull : 0;
      mag = (uint64_t)(v < 0 ? -v : v);
    } else {
      const uint64_t *sp = a.sp + ((size_t)key * a.Wsp << logn) + i;
      uint64_t fill = 0;
      for (unsigned j = 0; j < W2; ++j) {
        uint64_t w = fill;
        if (j < a.Wsp) { w = sp[(size_t)j << logn]; if (j + 1 == a.Wsp) fill = (uint64_t)((int64_t)w >> 63); }
        SP[(size_t)j * S] = w;
      }
    }
    uint64_t carry = 2 + (neg & 1);                            // the +1 of each two's complement below
    uint64_t m0 = 0, m1 = 0, m2 = 0;
    for (unsigned j = 0; j < W2; ++j) {
      uint64_t v;
      if (GATHER) {
        const gs_u128 t = (gs_u128)(j < WP ? a.P[j] : 0) * mag + m0;
        v = (uint64_t)t ^ neg;
        m0 = (uint64_t)(t >> 64);
      } else {
        const unsigned top = j < WP ? j : WP - 1;
        for (unsigned t = 0; t <= top; ++t) gs_mac(m0, m1, m2, a.P[t], SP[(size_t)(j - t) * S]);
        v = m0; m0 = m1; m1 = m2; m2 = 0;
      }
      const uint64_t aj = j < WP ? A[(size_t)j * S] : 0;
      const gs_u128 s = (gs_u128)carry + ~c2[(size_t)j << logn] + (j ? esign : (uint64_t)ev) + v + ~aj;
      D[(size_t)j * S] = (uint64_t)s;
      carry = (uint64_t)(s >> 64);
    }
  }

  // h = D P^-1 mod 2^k, stored as hs: sign-extended from bit k - 1
  uint64_t hfill;
  {
    uint64_t c0 = 0, c1 = 0, c2 = 0, w = 0;
    for (unsigned j = 0; j < W2; ++j) {
      for (unsigned t = 0; t <= j; ++t) gs_mac(c0, c1, c2, a.Pinv[t], D[(size_t)(j - t) * S]);
      w = c0; c0 = c1; c1 = c2; c2 = 0;
      if (j + 1 < W2) H[(size_t)j * S] = w;
    }
    const unsigned kb = a.k - 64 * (W2 - 1);                   // bits of the top word: 1..64
    hfill = 0 - ((w >> (kb - 1)) & 1);
    if (kb < 64) { const uint64_t mask = (1ull << kb) - 1; w = (w & mask) | (hfill & ~mask); }
    H[(size_t)(W2 - 1) * S] = w;
  }

  // p0 = a + P hs in W words of two's complement
  {
    uint64_t *dst = a.p0 + ((size_t)key * W << logn) + i;
    uint64_t c0 = 0, c1 = 0, c2 = 0;
    for (unsigned j = 0; j < W; ++j) {
      const unsigned top = j < WP ? j : WP - 1;
      for (unsigned t = 0; t <= top; ++t) gs_mac(c0, c1, c2, a.P[t], j - t < W2 ? H[(size_t)(j - t) * S] : hfill);
      if (j < WP) gs_mac(c0, c1, c2, A[(size_t)j * S], 1);
      dst[(size_t)j << logn] = c0;
      c0 = c1; c1 = c2; c2 = 0;
    }
  }

  // p1c = smod(p1, M): p1 - m M with m = [p1 >= floor(M/2)] + [p1 >= M + floor(M/2)]
  {
    const uint64_t *src = a.p1 + ((size_t)key * W << logn) + i;
    uint64_t *dst = a.p1c + ((size_t)key * W << logn) + i;
    uint64_t b1 = 0, b2 = 0;
    for (unsigned j = 0; j < W; ++j) {
      const uint64_t w = src[(size_t)j << logn];
      Q[(size_t)j * S] = w;
      const gs_u128 t1 = (gs_u128)w - (j < a.LM ? a.Mh[j] : 0) - b1, t2 = (gs_u128)w - (j < a.LM ? a.M3h[j] : 0) - b2;
      b1 = (uint64_t)(t1 >> 64) & 1;
      b2 = (uint64_t)(t2 >> 64) & 1;
    }
    const uint64_t m = (1 - b1) + (1 - b2);
    uint64_t mc = 0, borrow = 0;
    for (unsigned j = 0; j < W; ++j) {
      const gs_u128 mm = (gs_u128)(j < a.LM ? a.M[j] : 0) * m + mc;
      mc = (uint64_t)(mm >> 64);
      const gs_u128 t = (gs_u128)Q[(size_t)j * S] - (uint64_t)mm - borrow;
      dst[(size_t)j << logn] = (uint64_t)t;
      borrow = (uint64_t)(t >> 64) & 1;
    }
  }
}

#if defined(__HIPCC__)
template <bool GATHER>
__global__ __launch_bounds__(256) void genswk_crt_tail(GenswkTailArgs a) {
  extern __shared__ uint64_t genswk_planes[];
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << a.logn)) return;
  genswk_tail_lane<GATHER>(a, blockIdx.y, i, genswk_planes + threadIdx.x, blockDim.x);
}
#endif

}  // namespace gpq
