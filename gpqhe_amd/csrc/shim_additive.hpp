// shim_additive.hpp -- he_add / he_sub / he_addpt / he_subpt / he_neg (src/he-add.c:32-140), he_rot / he_conj (src/he-automorphism.c:87-115) with the reference's signatures.  Included inside mpi_shim.hip's extern "C" block.
// Part of the MPI-typed surface: one translation unit (mpi_shim.hip includes these fragments in order); split by concern in round 4.
#pragma once

// ---- src/he-add.c:32-140: he_add, he_sub, he_addpt, he_subpt, he_neg -----------------------------------------------------------
// Big-integer work only (mpi_addm / mpi_subm / mpi_neg, then mpi_smod), no RNS -- but GPQHE's algorithms interleave these with every
// product (he_inv: he_addpt between two he_mul, src/he-algo.c:146-155), each is 2n libgcrypt calls on the host (tens of milliseconds at
// n = 2^16), and a ciphertext the host has added to is one the device copies no longer match.  On the device they are one carry chain
// per coefficient and the centring the rescale kernels already do, on operands that are resident after the call before.
// kind 0: ct = a + b; 1: ct = a - b; 2: ct = a + pt; 3: ct = a - pt; 4: ct = -a (in place); 5: ct = a exactly (he_copy_ct, src/he-mem.c:88-97:
// no reduction -- 2n mpi_set on the host otherwise, and a copy the device knows nothing about)
static void additive(he_ct_t *ct, const he_ct_t *a, const he_ct_t *b, const he_pt_t *pt, int kind) {
  SHIM_CALL();
  need_hectx();
  if (kind < 2 && a->l != b->l) die("he_add / he_sub: operands at different levels");              // assert at src/he-add.c:35, :59
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, l = a->l;
  const double nu = kind >= 4 ? a->nu : kind < 2 ? (a->nu >= b->nu ? a->nu : b->nu) : (a->nu >= pt->nu ? a->nu : pt->nu);   // :37, :61, :84, :107
  const double B = kind >= 4 ? a->B : kind < 2 ? a->B + b->B : a->B;                                                     // :38, :62, :85, :108
  // a copy never looks at q_l (src/he-mem.c:88-97 copies whatever level the source claims)
  const std::vector<uint64_t> qw = kind == 5 ? std::vector<uint64_t>{2} : words_of(hectx.q[l], "he_add: q_l must be positive");
  const bool pow2 = is_pow2(qw);
  const unsigned nbq = kind == 5 ? 2 : G.mpi_get_nbits(hectx.q[l]), logql = nbq - 1;
  poly_mpi_t *out[2] = {&ct->c0, &ct->c1};
  if (logql == 0 && kind != 5) {                            // q_l = 1
    fill_minus_one(out[0], n); fill_minus_one(out[1], n);
    ct->l = l; ct->nu = nu; ct->B = B;
    return;
  }
  const unsigned Wout = kind == 5 ? 64 : logql / 64 + 1;    // the results are centred mod q_l (a copy keeps every word)
  // cpt: he_addpt / he_subpt by he_const_pt's plaintext (mpi_shim.hip, "constant plaintexts") -- the two integers ride in the launch and the
  // plaintext is no operand.  Returns false when the plaintext turns out to have another non-zero coefficient: nothing was written then.
  auto attempt = [&](const bool cpt, const int64_t ca, const int64_t cb) -> bool {
    const int count = kind >= 4 || cpt ? 2 : kind < 2 ? 4 : 3;
    const poly_mpi_t *in[4] = {&a->c0, &a->c1, kind < 2 ? &b->c0 : kind < 4 ? &pt->m : nullptr, kind < 2 ? &b->c1 : nullptr};
    bool dense = false;
    auto pass = [&](unsigned W, bool kept) -> bool {
      if (W > 32) die("he_add: coefficients wider than 2047 bits");
      const size_t big = (size_t)W * n;
      DevBuf scratch(192 * 8);
      ConstScan scan(cpt ? &pt->m : nullptr, n);
      StagedCall call(n, W, count, in, 2);
      call.speculate = kept; call.report_misfits = true; call.Wdown = Wout < W ? Wout : W;
      if (cpt) {
        call.side_parts = scan.parts; call.side = &scan.job; call.abort = &scan.dense;
        call.side_later = kept && all_operands_resident(in, count, n, W);   // the scan rides with the check of the resident copies
      }
      const StagedCall::Verdict v = call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
        int rc;
        if (kind == 5) {
          if (hipMemcpyAsync(o[0], x[0], big * 8, hipMemcpyDeviceToDevice, nullptr) != hipSuccess ||
              hipMemcpyAsync(o[1], x[1], big * 8, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) die("device copy failed");
          return;
        }
        if (cpt) {                                            // the sum, c1's copy and both mpi_smod in one launch
          if (gpq_he_addpt_const(c, o[0], o[1], x[0], x[1], ca, cb, kind & 1, W, logql, 1, nullptr) != GPQ_OK) die("he_addpt failed");
          return;
        }
        if (kind == 4) {
          rc = gpq_big_addsub(c, o[0], x[0], nullptr, W, 1, 2, nullptr);
          if (rc == GPQ_OK) rc = gpq_big_addsub(c, o[1], x[1], nullptr, W, 1, 2, nullptr);
        } else {
          rc = gpq_big_addsub(c, o[0], x[0], x[2], W, 1, kind & 1, nullptr);                          // c0 (+/-) the other c0 or the plaintext
          if (rc == GPQ_OK && kind < 2) rc = gpq_big_addsub(c, o[1], x[1], x[3], W, 1, kind & 1, nullptr);
          else if (rc == GPQ_OK && hipMemcpyAsync(o[1], x[1], big * 8, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) die("device copy failed");   // c1 mod q, :92, :115
        }
        if (rc == GPQ_OK)                                                                              // mpi_smod of both, :43-44 ...
          rc = pow2 ? gpq_he_rs(c, o[0], o[1], W, 0, logql, 1, nullptr)
                    : gpq_he_rs_general(c, o[0], o[1], W, 1ull, qw.data(), (unsigned)qw.size(), 1, scratch.p, nullptr);
        if (rc != GPQ_OK) die("he_add failed");
      }, out);
      if (v == StagedCall::Aborted) dense = true;
      return v != StagedCall::Misfit;
    };
    // wrapping sums are harmless below a power of two; any other q_l measures its operands first.  One bit of headroom: the sum of two
    // such integers still fits.  A copy keeps every word: any width of the resident copies serves it.
    width_ladder(in, count, n, pow2 || kind == 5, kind == 5 ? 1 : Wout, nbq, 1, pass);
    return !dense;
  };
  int64_t ca = 0, cb = 0;
  const bool candidate = (kind == 2 || kind == 3) && g_const_pt_on && pow2 && logql >= 1 && const_pt_candidate(&pt->m, n, &ca, &cb);
  if (candidate && attempt(true, ca, cb)) ++g_const_taken;
  else attempt(false, 0, 0);
  ct->l = l; ct->nu = nu; ct->B = B;
}
void he_add(he_ct_t *ct, const he_ct_t *ct1, const he_ct_t *ct2) { additive(ct, ct1, ct2, nullptr, 0); }
void he_sub(he_ct_t *ct, const he_ct_t *ct1, const he_ct_t *ct2) { additive(ct, ct1, ct2, nullptr, 1); }
void he_addpt(he_ct_t *dest, const he_ct_t *src, const he_pt_t *pt) { additive(dest, src, nullptr, pt, 2); }
void he_subpt(he_ct_t *dest, const he_ct_t *src, const he_pt_t *pt) { additive(dest, src, nullptr, pt, 3); }
void he_neg(he_ct_t *ct) { additive(ct, ct, nullptr, nullptr, 4); }
void he_copy_ct(he_ct_t *dest, const he_ct_t *src) { if (dest != src) additive(dest, src, nullptr, nullptr, 5); }      // src/he-mem.c:88-97

// he_rot / he_conj, src/he-automorphism.c:87-115: permute both polynomials, then he_swk (:40-85) in place
static void automorphism(he_ct_t *ct, const he_evk_t *evk, bool conj, unsigned rot) {
  SHIM_CALL();
  need_hectx();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, l = ct->l;
  const std::vector<uint64_t> qw = words_of(hectx.q[l], "he_rot/he_conj: q_l must be positive");
  const bool pow2 = is_pow2(qw);
  const unsigned nbq = G.mpi_get_nbits(hectx.q[l]), logql = nbq - 1, nbPqL = G.mpi_get_nbits(hectx.PqL);
  const unsigned dimB = (nbq + nbPqL + polyctx.logn) / 59 + 1, dimP = hectx.dim;                // src/he-automorphism.c:52
  const unsigned W = logql / 64 + 1;
  const size_t big = (size_t)W * n;
  DevBuf r0(big * 8), r1(big * 8), ws(pow2 ? gpq_he_swk_workspace_bytes(c, W, dimB, dimP, 1) : gpq_he_general_workspace_bytes(c, W, 0, dimB, dimP, 1));
  const poly_mpi_t *in[2] = {&ct->c0, &ct->c1};
  poly_mpi_t *out[2] = {&ct->c0, &ct->c1};
  StagedCall call(n, W, 2, in, 2);
  CallKey key(evk, dimB, n);
  key.ride(call);
  call.prepare();
  key.settle();
  call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
    int rc = conj ? gpq_poly_conj(c, r0.u64(), x[0], W, 1, nullptr) : gpq_poly_rot(c, r0.u64(), x[0], W, rot, 1, nullptr);              // :95-96 / :108-109
    if (rc == GPQ_OK) rc = conj ? gpq_poly_conj(c, r1.u64(), x[1], W, 1, nullptr) : gpq_poly_rot(c, r1.u64(), x[1], W, rot, 1, nullptr);
    if (rc == GPQ_OK)                                                                                                                       // :97 / :110
      rc = pow2 ? gpq_he_swk(c, o[0], o[1], r0.u64(), r1.u64(), key.k0, key.k1, W, logql, dimB, dimP, 1, ws.p, nullptr)
                : gpq_he_swk_general(c, o[0], o[1], r0.u64(), r1.u64(), key.k0, key.k1, W, qw.data(), (unsigned)qw.size(), dimB, dimP, 1,
                                     ws.p, nullptr);
    if (rc != GPQ_OK) die("he_rot/he_conj failed");
  }, out);
}
void he_conj(he_ct_t *ct, const he_evk_t *ck) { automorphism(ct, ck, true, 0); }
void he_rot(he_ct_t *ct, const int rot, const he_evk_t *rk) { automorphism(ct, &rk[rot], false, (unsigned)rot); }   // rk[rot], :110

