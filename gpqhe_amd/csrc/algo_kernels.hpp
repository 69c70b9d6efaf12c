// algo_kernels.hpp -- device fragment of bridge.hip: the additive glue of the evaluators of src/he-algo.c:131-458 (he_inv, he_sqrt, he_sigmoid,
// he_log, he_exp) as ONE pass.  Between their products those functions call he_neg, he_add, he_sub, he_addpt, he_subpt (src/he-add.c:32-140),
// he_moddown (src/he-rescale.c:56-70) and he_copy_ct, and each of these is "add, then mpi_smod(., q_l)" (src/types.c:108-113).  Every q_l is a power
// of two and q_(l-1) divides q_l, so smod(smod(u, 2^k) + v, 2^m) = smod(u + v, 2^m) for m <= k: a chain of them is the wrapping sum of its terms
// followed by the LAST smod ("Evaluators").  With x^h = x^(n/2):
//   out.c0 = smod(s_0 x_0.c0 + .. + s_(K-1) x_(K-1).c0 + (a + b x^h), 2^logql)
//   out.c1 = smod(s_0 x_0.c1 + .. + s_(K-1) x_(K-1).c1,               2^logql)         K <= 3, s_k = +-1, a and b he_const_pt's integers (0: none)
// Big slabs are word-major (word j of coefficient i at j n + i): one lane per coefficient, so every word plane a wavefront touches is one contiguous
// run of 8-byte words, and one carry chain over the words.  A lane reads word j of every term before it writes word j of its own coefficient and
// touches no other coefficient, so out may be any of the inputs in the same position.  No workspace, no LDS.
// PT (gpq_he_lin_pt): he_addpt / he_subpt by ONE dense plaintext m (src/he-add.c:80-123) is one more addend of c0's chain,
//   out.c0 = smod(.. + msign m + (a + b x^h), 2^logql),
// m a W-word big slab of one polynomial shared by the whole batch and read by the c0 half of the grid only.
#pragma once
#include "constpt_kernels.hpp"   // centre_word
namespace gpq {

struct LinConstArgs {
  uint64_t *out0, *out1;          // c0 / c1 of the batch: [batch][W][n]
  const uint64_t *x0[3], *x1[3];
  int64_t a, b;
  unsigned neg;                   // bit k: s_k = -1
  unsigned W, logn, logql;
  const uint64_t *m;              // PT: the plaintext, [W][n], no batch stride
  unsigned mneg;                  // PT: 1 where msign = -1
};

// Grid y = 2 ciphertext + (0: c0, 1: c1).  -x = ~x + 1 on the words of x: the ones of the negated terms enter as the carry into word 0.
template <unsigned K, bool PT = false>
__global__ __launch_bounds__(256) void he_lin_const(LinConstArgs a) {
  const unsigned n = 1u << a.logn, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t base = ((size_t)(blockIdx.y >> 1) * a.W << a.logn) + i;
  const bool c1 = blockIdx.y & 1;
  const uint64_t *in[K];
  uint64_t flip[K];
#pragma unroll
  for (unsigned k = 0; k < K; ++k) {
    in[k] = (c1 ? a.x1[k] : a.x0[k]) + base;                              // (may be out: no __restrict__)
    flip[k] = 0 - (uint64_t)((a.neg >> k) & 1u);
  }
  uint64_t *out = (c1 ? a.out1 : a.out0) + base;
  const int64_t t = c1 ? 0 : i == 0 ? a.a : i == (n >> 1) ? a.b : 0;
  const uint64_t t0 = (uint64_t)t, text = (uint64_t)(t >> 63);
  uint64_t carry = __popc(a.neg & ((1u << K) - 1u)), qsign = 0;           // at most K + 1 afterwards: K + 1 addends and a carry of at most K
  const bool pt = PT && !c1;                                              // (uniform over the block)
  const uint64_t *m = PT ? a.m + i : nullptr, mflip = PT ? 0 - (uint64_t)a.mneg : 0;
  if (pt) carry += a.mneg;                                                // PT: one addend and one unit of carry more, K + 2
  for (unsigned j = 0; j < a.W; ++j) {
    const uint64_t y = j ? text : t0;
    uint64_t acc = carry + y, c = acc < y;
#pragma unroll
    for (unsigned k = 0; k < K; ++k) {
      const uint64_t x = in[k][(size_t)j << a.logn] ^ flip[k];
      acc += x;
      c += acc < x;
    }
    if (pt) {
      const uint64_t x = m[(size_t)j << a.logn] ^ mflip;
      acc += x;
      c += acc < x;
    }
    carry = c;
    out[(size_t)j << a.logn] = centre_word(acc, j, a.logql, qsign);
  }
}

}  // namespace gpq
