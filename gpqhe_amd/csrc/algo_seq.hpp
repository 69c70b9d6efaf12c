// algo_seq.hpp -- the evaluators of src/he-algo.c:131-548 (he_inv, he_sqrt, he_sigmoid, he_log, he_exp, he_cmp, he_cmppt), each written ONCE as a
// sequence over four operations on numbered ciphertext slots (slot 0 = the input, he_cmp's slot 1 = its second input, the others the reference's
// named temporaries):
//   mul(d, x, y)      he_mul(&d, &x, &y, rlk); he_rs(&d)                                  src/he-mult.c:88-156, src/he-rescale.c:33-54
//   mulc(d, x, re)    he_const_pt(&pt, re); he_mulpt(&d, &x, &pt); he_rs(&d)              src/he-encode.c:119-125, src/he-mult.c:159-196
//   mulpt(d, x)       he_mulpt(&d, &x, &pt) by the call's one dense plaintext; he_rs(&d)  (he_exp, :448-450)
//   lin(d, terms, ..) a chain of he_copy_ct / he_neg / he_add / he_addpt / he_subpt / he_moddown collapsed into one sum and one mpi_smod at
//                     the level the chain ends at (algo_kernels.hpp has the argument); terms may sit at higher levels: their he_moddown rides;
//                     he_cmppt's he_addpt by the call's one dense plaintext is a term of it (msign)
// plus alias(d, x) -- he_copy_ct of a value that is not written afterwards: a name, no work -- and ret(d), the function's result.
// Two implementations run the same text.  Book (here) is the host's: it replays l, nu and B call for call as the reference -- and mpi_shim.hip /
// shim_additive.hpp per call today -- compute them, knows every level's logql, limb counts and constants, and refuses what cannot run before
// anything is launched.  bridge_algo.hpp's AlgoDevice extends it with the launches.  Only public calls of gpqhe_hip.h are used, so that the
// MPI-typed surface (shim_evaluators.hpp) replays the bookkeeping with the very same text.
#pragma once
#include "../../include/gpqhe_hip.h"
#include "../../include/gpqhe_hip_algo.h"

#include <cstddef>
#include <cstdint>

namespace gpq_algo {

enum { SLOTS = 10 };                                   // the input and at most nine named temporaries (he_exp)
struct Term { int slot, sign; };

// the reference's bounds for the replay of B (struct he_ctx: Delta, bnd.Brs, bnd.Bmult[l]); a slab call has none and its B means nothing
struct Bounds { double Brs; const double *Bmult; unsigned l; };      // l = the input's level; Bmult is indexed by the level

inline int depth(int kind, unsigned iter) {
  switch (kind) {
    case GPQ_ALGO_INV: return (int)iter + 1;           // :129
    case GPQ_ALGO_SQRT: return 2 * (int)iter;
    case GPQ_ALGO_SIGMOID: case GPQ_ALGO_LOG: return 4;
    case GPQ_ALGO_EXP: return 4 + (int)iter;
    default: return -1;
  }
}
// named temporaries of each function (slot 0, the input, not counted)
inline unsigned temporaries(int kind) {
  switch (kind) {
    case GPQ_ALGO_INV: case GPQ_ALGO_SQRT: return 3;
    case GPQ_ALGO_SIGMOID: return 9;
    case GPQ_ALGO_LOG: return 7;
    case GPQ_ALGO_EXP: return 9;
    default: return 0;
  }
}

struct Book {
  gpq_ctx *c;
  unsigned W, batch, logn, nprimes, logqL, logql0, s, dimpt_m;
  bool sizing;                                         // also take the maximum of the per-level workspaces (gpq_he_algo_workspace_bytes)
  double Delta, Brs;
  const double *Bmult;
  unsigned l0;
  struct Val { bool live; unsigned lv; double nu, B; } v[SLOTS];
  int err = GPQ_OK;
  const char *why = "";
  unsigned nops = 0;                                   // operations that write a slot, so far
  int last_dst = -1, result = -1;
  bool last_mul_reads_input = false, uses_m = false;
  bool two = false;                                    // slot 1 is a second input ciphertext (he_cmp), centred mod 2^logql as slot 0
  double pt_nu = 0.0;                                  // nu of lin's dense plaintext (he_cmppt's pt->nu); a slab call passes Delta
  size_t ws = 0;
  // what the last operation decided, for the launch behind it
  unsigned dimP = 0, dimA = 0, dimB = 0, dim = 0;
  int64_t ca = 0;

  Book(gpq_ctx *c_, unsigned W_, unsigned batch_, unsigned logqL_, unsigned logql_, unsigned logDelta, unsigned dimpt_m_, bool sizing_,
       double nu0 = 1.0, double B0 = 0.0, const Bounds *bnd = nullptr)
      : c(c_), W(W_), batch(batch_), logn(c_ ? gpq_ctx_logn(c_) : 0), nprimes(c_ ? gpq_ctx_nprimes(c_) : 0), logqL(logqL_), logql0(logql_), s(logDelta),
        dimpt_m(dimpt_m_), sizing(sizing_), Delta(1.0), Brs(bnd ? bnd->Brs : 0.0), Bmult(bnd ? bnd->Bmult : nullptr), l0(bnd ? bnd->l : 0) {
    for (Val &x : v) x = Val{false, 0, 0, 0};
    v[0] = Val{true, 0, nu0, B0};
    if (!c) { fail("null context"); return; }
    if (s < 1 || s > 63) { fail("logDelta outside 1..63"); return; }
    if (logql0 < 1 || logql0 > logqL) { fail("1 <= logql <= logqL"); return; }
    Delta = (double)(1ull << s);
    pt_nu = Delta;
  }
  void second_input(double nu, double B) { two = true; v[1] = Val{true, 0, nu, B}; }
  bool is_input(int slot) const { return slot == 0 || (two && slot == 1); }
  bool fail(const char *w) { if (!err) { err = GPQ_ERR_INVALID; why = w; } return false; }
  unsigned logql(unsigned lv) const { return logql0 - lv * s; }
  unsigned lv(int slot) const { return v[slot].lv; }
  bool reachable(unsigned level) { return (uint64_t)level * s + 1 <= logql0 ? true : fail("a level would fall below logql = 1"); }
  unsigned mulpt_dim(unsigned level) const { return (logql(level) + 1 + s + logn) / 59u + 1; }   // src/he-mult.c:168 with pt->nu = Delta
  void wrote(int d, bool mul_reads_input) { ++nops; last_dst = d; last_mul_reads_input = mul_reads_input; }
  void rescaled(int d, unsigned level, double nu, double B) { v[d] = Val{true, level + 1, nu / Delta, B / Delta + Brs}; }   // src/he-rescale.c:36-38
  bool constant(double re) {
    int64_t cb = 0;
    return gpq_const_pt(re, 0.0, s, &ca, &cb) == GPQ_OK ? true : fail("a constant does not fit int64_t at this Delta");
  }

  bool mul(int d, int x, int y) {
    if (err) return false;
    if (!v[x].live || !v[y].live || v[x].lv != v[y].lv) return fail("he_mul: operands at different levels");      // assert at src/he-mult.c:90
    const unsigned level = v[x].lv;
    if (!reachable(level + 1)) return false;
    if (gpq_he_dims(c, logqL, logql(level), &dimP, &dimA, &dimB, nullptr) != GPQ_OK || dimA > nprimes || dimB > nprimes)
      return fail("the context has too few primes for he_mul at this q_L");
    if (sizing) {
      const size_t b = gpq_he_mul_workspace_bytes(c, W, dimA, dimB, dimP, batch);
      if (!b) return fail("gpq_he_mul_workspace_bytes refuses the shape");
      if (b > ws) ws = b;
    }
    const double nu = v[x].nu * v[y].nu;                                                       // src/he-mult.c:93
    // :94-95 read the operands' nu after :93 stored the product: where the destination is an operand, B is built from the new nu (mpi_shim.hip, he_mul)
    const double nu1 = d == x ? nu : v[x].nu, nu2 = d == y ? nu : v[y].nu;
    const double B = nu1 * v[y].B + nu2 * v[x].B + v[x].B * v[y].B + (Bmult ? Bmult[l0 - level] : 0.0);
    rescaled(d, level, nu, B);
    wrote(d, is_input(x) || is_input(y));
    return true;
  }
  // x = x^2 and y = y^2, two independent squarings at one level (he_cmp_core's an^2 and bn^2): the bookkeeping of the two he_mul + he_rs in the
  // reference's order; on the device ONE product over 2 batch ciphertexts, so the products' workspace is sized for that
  bool sq2(int x, int y) {
    if (err) return false;
    if (batch > 16383) return fail("he_cmp: a round squares 2 batch ciphertexts at once: batch <= 16383");
    const bool was = sizing;
    sizing = false;
    const bool ok = mul(x, x, x) && mul(y, y, y);
    sizing = was;
    if (ok && sizing) {
      const size_t b = gpq_he_mul_workspace_bytes(c, W, dimA, dimB, dimP, 2 * batch);     // (dims: the level both were at)
      if (!b) return fail("gpq_he_mul_workspace_bytes refuses the shape");
      if (b > ws) ws = b;
    }
    return ok;
  }
  bool mulc(int d, int x, double re) {
    if (err) return false;
    if (!v[x].live) return fail("he_mulpt: the operand has no value");
    const unsigned level = v[x].lv;
    if (!reachable(level + 1) || !constant(re)) return false;
    dim = mulpt_dim(level);
    if (dim > nprimes) return fail("the context has too few primes for he_mulpt");
    if (!gpq_he_mulpt_const_fits(c, ca, 0, logql(level), dim)) return fail("a constant does not fit he_mulpt's basis (gpq_he_mulpt_const_fits)");
    rescaled(d, level, v[x].nu * Delta, v[x].B * Delta);                                       // src/he-mult.c:163-164 with pt->nu = Delta
    wrote(d, false);
    return true;
  }
  bool mulpt(int d, int x) {
    if (err) return false;
    if (!v[x].live) return fail("he_mulpt: the operand has no value");
    const unsigned level = v[x].lv;
    if (!reachable(level + 1)) return false;
    dim = dimpt_m;
    if (dim < 1 || dim > mulpt_dim(level) || dim > nprimes) return fail("dimpt outside 1..the reference's limb count, or beyond the context's primes");
    if (sizing) {
      const size_t b = gpq_he_mulpt_workspace_bytes(c, dim, batch);
      if (b > ws) ws = b;
    }
    uses_m = true;
    rescaled(d, level, v[x].nu * Delta, v[x].B * Delta);                                       // he_ecd: pt->nu = Delta (src/he-encode.c:109)
    wrote(d, false);
    return true;
  }
  // d = sum of sign * term [+ csign * he_const_pt(re)] at level lv_out; nu: the running maximum of he_add / he_addpt (src/he-add.c:37, :84), B: the
  // running sum of he_add (:38), both in the order of the terms; he_neg, he_moddown and he_copy_ct leave them alone.  msign != 0: he_addpt (+1) /
  // he_subpt (-1) of the call's one dense plaintext after the terms: nu the larger of the sum's and pt->nu, B the sum's (:84-85)
  bool lin(int d, const Term *t, unsigned K, unsigned lv_out, bool has_c = false, double re = 0.0, int csign = 1, int msign = 0) {
    if (err) return false;
    if (K < 1 || K > 3) return fail("he_add: one to three terms");
    double nu = 0, B = 0;
    for (unsigned k = 0; k < K; ++k) {
      const Val &x = v[t[k].slot];
      if (!x.live || x.lv > lv_out) return fail("he_add: a term below the level of the sum");
      nu = k && nu >= x.nu ? nu : x.nu;
      B = k ? B + x.B : x.B;
    }
    if (!reachable(lv_out)) return false;
    if (msign) nu = nu >= pt_nu ? nu : pt_nu;
    ca = 0;
    if (has_c) {
      if (!constant(re)) return false;
      if (csign < 0) ca = -ca;
      nu = nu >= Delta ? nu : Delta;
    }
    v[d] = Val{true, lv_out, nu, B};
    wrote(d, false);
    return true;
  }
  bool alias(int d, int x) {
    if (err) return false;
    v[d] = v[x];
    last_dst = -1;
    return true;
  }
  bool ret(int d) {
    if (err) return false;
    result = d;
    return true;
  }
  bool result_is_last_write() const { return result >= 0 && last_dst == result; }
};

// ---- the sequences --------------------------------------------------------------------------------------------------------------------------
// he_inv's slots by name, and what it inverts: the sum of K <= 2 terms at one level (the caller's he_add in front of a nested he_inv rides in
// the two opening sums).  The default is the function on its own: the input, and the reference's three temporaries.
struct InvSlots { int TMP, AN, BN; Term src[2]; unsigned K; };
template <class O> void seq_inv(O &o, unsigned iter, const InvSlots &n = InvSlots{1, 2, 3, {{0, 1}, {0, 1}}, 1}, bool nested = false) {   // src/he-algo.c:131-164
  const int TMP = n.TMP, AN = n.AN, BN = n.BN;
  const Term neg[2] = {{n.src[0].slot, -n.src[0].sign}, {n.src[1].slot, -n.src[1].sign}};
  const unsigned lv = o.lv(n.src[0].slot);
  o.lin(AN, neg, n.K, lv + 1, true, 2);                                  // :145-148  tmp = -ct; an = tmp + two; he_moddown(&an)
  o.lin(BN, neg, n.K, lv, true, 1);                                      // :149      bn = tmp + one
  for (unsigned i = 0; i < iter; ++i) {
    o.mul(BN, BN, BN);                                                   // :151-152
    const Term b[1] = {{BN, 1}};
    o.lin(TMP, b, 1, o.lv(BN), true, 1);                                 // :153
    o.mul(AN, AN, TMP);                                                  // :154-155
  }
  if (!nested) o.ret(AN);                                                // :157 (nested: the caller reads AN)
}

template <class O> void seq_sqrt(O &o, unsigned iter) {                  // :166-206
  enum { CT, TMP, AN, BN };
  const Term ct[1] = {{CT, 1}};
  o.alias(AN, CT);                                                       // :184
  o.lin(BN, ct, 1, 0, true, 1, -1);                                      // :185  bn = ct - one
  for (unsigned i = 0; i < iter; ++i) {
    o.mulc(TMP, BN, 0.5);                                                // :188-189
    const Term nt[1] = {{TMP, -1}}, an[1] = {{AN, 1}}, bn[1] = {{BN, 1}};
    o.lin(TMP, nt, 1, o.lv(TMP), true, 1);                               // :190-191  -(tmp - one)
    o.lin(AN, an, 1, o.lv(AN) + 1);                                      // :192  he_moddown
    o.mul(AN, AN, TMP);                                                  // :193-194
    if (i + 1 == iter) break;                                            // the last round's bn (:196-202) feeds nothing: an is the result
    o.lin(TMP, bn, 1, o.lv(BN), true, 3, -1);                            // :196
    o.mulc(TMP, TMP, 0.25);                                              // :197-198
    o.mul(BN, BN, BN);                                                   // :199-200
    o.mul(BN, BN, TMP);                                                  // :201-202
  }
  o.ret(AN);                                                             // :205
}

template <class O> void seq_sigmoid(O &o) {                              // :208-277
  enum { CT, CT2, CT4, CT8, CT3X, CT13, CT7X, CT57, CT9X, RES };
  o.mul(CT2, CT, CT);                                                    // :223-224  l-1
  o.mul(CT4, CT2, CT2);                                                  // :226-227  l-2
  o.mul(CT8, CT4, CT4);                                                  // :229-230  l-3
  const Term c2[1] = {{CT2, 1}}, c9[1] = {{CT9X, 1}};
  o.mulc(CT3X, CT, -1. / 48);                                            // :232-234
  o.lin(CT13, c2, 1, o.lv(CT2), true, (1. / 4) / (-1. / 48));            // :236-237
  o.mul(CT13, CT3X, CT13);                                               // :238-239  l-2 (:240-241 ride in the closing sum)
  o.mulc(CT7X, CT, -17. / 80640);                                        // :243-245
  o.lin(CT57, c2, 1, o.lv(CT2), true, (1. / 480) / (-17. / 80640));      // :247-248
  o.mul(CT57, CT7X, CT57);                                               // :249-250  l-2
  o.mul(CT57, CT4, CT57);                                                // :251-252  l-3 (:253 rides)
  o.mulc(CT9X, CT, 31. / 1451520);                                       // :255-257  l-1
  o.lin(CT9X, c9, 1, o.lv(CT9X) + 2);                                    // :258-259
  o.mul(CT9X, CT9X, CT8);                                                // :260-261  l-4
  const Term sum[3] = {{CT13, 1}, {CT57, 1}, {CT9X, 1}};
  o.lin(RES, sum, 3, o.lv(CT9X), true, 1. / 2);                          // :240-241, :253, :263-266
  o.ret(RES);
}

// one of he_log's two halves: acc = ct8 + k6 x^6 + k4 x^4 + k2 x^2 + k0, then acc = (kx * x) * acc, x = ct (odd) or ct2 (even)
template <class O> void log_half(O &o, int ACC, int X, double k6, double k4, double k2, double k0, double kx) {
  enum { CT, CT2, CT4, CT8, CTODD, CTEVEN, CTTMP, RES };
  const Term acc[2] = {{ACC, 1}, {CTTMP, 1}}, tmp[1] = {{CTTMP, 1}};
  o.alias(ACC, CT8);                                                     // :301 / :327
  o.mulc(CTTMP, CT2, k6);                                                // :302-304 / :328-330  l-2
  o.mul(CTTMP, CTTMP, CT4);                                              // :305-306 / :331-332  l-3
  o.lin(ACC, acc, 2, o.lv(CT8));                                         // :307 / :333
  o.mulc(CTTMP, CT4, k4);                                                // :308-310 / :334-336  l-3
  o.lin(ACC, acc, 2, o.lv(CT8));                                         // :311 / :337
  o.mulc(CTTMP, CT2, k2);                                                // :312-314 / :338-340  l-2
  o.lin(ACC, acc, 2, o.lv(CT8), true, k0);                               // :315-318 / :341-344
  o.mulc(CTTMP, X, kx);                                                  // :319-321 / :345-347
  o.lin(CTTMP, tmp, 1, o.lv(CT8));                                       // :322-323 / :348
  o.mul(ACC, CTTMP, ACC);                                                // :324-325 / :349-350  l-4
}
template <class O> void seq_log(O &o) {                                  // :279-361
  enum { CT, CT2, CT4, CT8, CTODD, CTEVEN, CTTMP, RES };
  o.mul(CT2, CT, CT);                                                    // :292-293
  o.mul(CT4, CT2, CT2);                                                  // :295-296
  o.mul(CT8, CT4, CT4);                                                  // :298-299
  log_half(o, CTODD, CT, 9. / 7., 9. / 5., 9. / 3., 9, 1. / 9.);         // :300-325
  log_half(o, CTEVEN, CT2, 10. / 8., 10. / 6., 10. / 4., 10. / 2, -1. / 10.);   // :326-350
  const Term sum[2] = {{CTODD, 1}, {CTEVEN, 1}};
  o.lin(RES, sum, 2, o.lv(CTODD));                                       // :352
  o.ret(RES);
}

template <class O> void seq_exp(O &o, unsigned iter) {                   // :364-458
  enum { CT, ACT, CT2, CT4, CT01, CT23, CT45, CT67, CT4567, RES };
  o.mulpt(ACT, CT);                                                      // :448-450  act = (a / 2^iter) ct
  const Term act[1] = {{ACT, 1}};
  o.mul(CT2, ACT, ACT);                                                  // :379-380  l-1 (of he_exp_taylor's input)
  o.mul(CT4, CT2, CT2);                                                  // :382-383  l-2
  o.lin(CT01, act, 1, o.lv(ACT), true, 1.0);                             // :385-386
  o.mulc(CT01, CT01, 1.0);                                               // :387-388  l-1 (:389 rides)
  o.lin(CT23, act, 1, o.lv(ACT), true, 3.0);                             // :391-392
  o.mulc(CT23, CT23, 1.0 / 6);                                           // :393-395
  o.mul(CT23, CT2, CT23);                                                // :396-397  l-2
  o.lin(CT45, act, 1, o.lv(ACT), true, 5.0);                             // :402-403
  o.mulc(CT45, CT45, 1.0 / 120);                                         // :404-406  l-1 (:407 rides)
  o.lin(CT67, act, 1, o.lv(ACT), true, 7.0);                             // :409-410
  o.mulc(CT67, CT67, 1.0 / 5040);                                        // :411-413
  o.mul(CT67, CT2, CT67);                                                // :414-415  l-2
  const Term hi[2] = {{CT45, 1}, {CT67, 1}};
  o.lin(CT4567, hi, 2, o.lv(CT67));                                      // :407, :417
  o.mul(CT4567, CT4, CT4567);                                            // :418-419  l-3
  const Term sum[3] = {{CT01, 1}, {CT23, 1}, {CT4567, 1}};
  o.lin(RES, sum, 3, o.lv(CT4567));                                      // :389, :399-400, :421
  for (unsigned i = 0; i < iter; ++i) o.mul(RES, RES, RES);              // :452-455
  o.ret(RES);
}

// he_cmp (with_pt = false: slot 1 is the second ciphertext) and he_cmppt (the call's dense plaintext), src/he-algo.c:460-548.  Eight slots.
// The two he_inv are seq_inv's text on three slots of their own; he_cmp_core's bn = 1 - an (:485-486, :499-500) is written where the next
// round reads it, so the last one -- it feeds nothing -- is never computed (as he_sqrt's).
template <class O> void seq_cmp(O &o, unsigned iter, unsigned t, bool with_pt) {
  enum { CT, CT2, INV, AN, BN, ITMP, IAN, IBN };                         // (AN = CMP_AN, BN = CMP_BN)
  const Term sum[2] = {{CT, 1}, {CT2, 1}}, an[1] = {{AN, 1}}, nan[1] = {{AN, -1}};
  const InvSlots first{ITMP, IAN, IBN, {{INV, 1}, {INV, 1}}, 1}, round{ITMP, IAN, IBN, {{AN, 1}, {BN, 1}}, 2};
  if (with_pt) o.lin(INV, sum, 1, 0, false, 0.0, 1, 1);                  // :543  he_addpt(&an, ct, pt)
  else o.lin(INV, sum, 2, 0);                                            // :525  he_add(&an, ct1, ct2)   (:466 inv = an)
  o.mulc(INV, INV, 0.5);                                                 // :473-474  l-1
  seq_inv(o, iter, first, true);                                         // :475      l-2-iter, in IAN
  o.mulc(AN, CT, 0.5);                                                   // :477-478  l-1
  o.lin(AN, an, 1, o.lv(AN) + iter + 1);                                 // :479-480  iter + 1 he_moddown
  o.mul(AN, AN, IAN);                                                    // :482-483  l-3-iter
  for (unsigned r = 0; r < t; ++r) {
    o.lin(BN, nan, 1, o.lv(AN), true, 1);                                // :485-486 / :499-500  bn = -(an - one)
    o.sq2(AN, BN);                                                       // :489-492  an = an^2, bn = bn^2: independent and at one level, ONE product
    seq_inv(o, iter, round, true);                                       // :493-494  he_add(&inv, an, &bn) rides in he_inv's two sums
    o.lin(AN, an, 1, o.lv(AN) + iter + 1);                               // :495-496
    o.mul(AN, AN, IAN);                                                  // :497-498
  }
  o.ret(AN);                                                             // :527 / :545
}
enum { CMP_SINGLES = 4, CMP_AN = 3, CMP_BN = 4 };                        // INV and he_inv's three; an and bn (sq2) live side by side
// bridge_algo.hpp's allocator names the singles, their spare and the four halves of the two double buffers in one table of SLOTS entries
static_assert(CMP_SINGLES + 1 + 4 <= SLOTS, "he_cmp's buffers do not fit the evaluators' buffer table");

// (3 + iter)(1 + t), the levels he_cmp / he_cmppt consume; -1 beyond 4096 (64 words of 64 bits hold no more levels)
inline int cmp_depth(unsigned iter, unsigned t) {
  if (iter > 4096 || t > 4096) return -1;
  const uint64_t d = (uint64_t)(3 + iter) * (1 + t);
  return d > 4096 ? -1 : (int)d;
}

template <class O> bool run_cmp(O &o, unsigned iter, unsigned t, bool with_pt) {
  if (o.err) return false;
  const int d = cmp_depth(iter, t);
  if (d < 0) return o.fail("a level would fall below logql = 1");
  if (!o.reachable((unsigned)d)) return false;          // before any loop over iter or t
  seq_cmp(o, iter, t, with_pt);
  return o.err == GPQ_OK;
}

// false: refused (o.err, o.why)
template <class O> bool run(O &o, int kind, unsigned iter) {
  if (o.err) return false;
  if (iter > 4096) return o.fail("a level would fall below logql = 1");   // (64 words of 64 bits hold no more levels)
  const int d = depth(kind, iter);
  if (d < 0) return o.fail("unknown evaluator");
  if (!o.reachable((unsigned)d)) return false;          // before any loop over iter
  switch (kind) {
    case GPQ_ALGO_INV: seq_inv(o, iter); break;
    case GPQ_ALGO_SQRT: seq_sqrt(o, iter); break;
    case GPQ_ALGO_SIGMOID: seq_sigmoid(o); break;
    case GPQ_ALGO_LOG: seq_log(o); break;
    default: seq_exp(o, iter); break;
  }
  return o.err == GPQ_OK;
}

}  // namespace gpq_algo
