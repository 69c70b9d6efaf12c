// shim_evaluators.hpp -- he_inv / he_sqrt / he_sigmoid / he_log / he_exp / he_cmp / he_cmppt (src/he-algo.c:131-548) on the reference's own types, each as ONE staged
// call around one evaluator of gpqhe_hip_algo.h: the source is found resident or uploaded once, the key comes through the key cache, the
// result comes down once and is remembered.  Included inside mpi_shim.hip's extern "C" block.
// The names are gpq_shim_he_*: a library-side `he_inv` would shadow GPQHE's own under the first-definition rule (as for
// gpq_shim_he_dec_dcd); a GPQHE build forwards its functions under its GPQHE_HIP guard and keeps its loop for a 0 return.
// l / nu / B: algo_seq.hpp's Book replays the reference's bookkeeping call for call over the very text the device runs.

// 1: done.  0, dst untouched: a modulus on the way or Delta is no power of two, the depth does not fit the source's level, a constant does not fit,
// the source is not centred mod q_l, the context is not the one gpq_he_dims describes, or (he_exp) the host program has no he_ecd.
// he_cmp / he_cmppt (:460-548) go the same way, with a second operand: `kind` SHIM_CMP takes src2 (found resident or uploaded as src is, counted
// as src is; 0 also where the two levels differ -- the reference asserts), SHIM_CMPPT takes pt (converted and uploaded as he_exp's plaintext,
// W widened to its bits, 0 beyond 32 words; pt->nu enters the bookkeeping); t is their round count.
enum { SHIM_CMP = 100, SHIM_CMPPT = 101 };
static int shim_evaluator(he_ct_t *dst, const he_ct_t *src, const he_evk_t *rlk, int kind, unsigned iter, gpq_zc a, const he_ct_t *src2 = nullptr,
                          const he_pt_t *cpt = nullptr, unsigned t = 0) {
  SHIM_CALL();
  need_hectx();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, logn = polyctx.logn, l = src->l;
  const bool cmp = kind >= SHIM_CMP;
  if (kind == SHIM_CMP && src2->l != l) return 0;              // assert at src/he-add.c:35: the reference's loop decides
  const int depth = cmp ? gpq_he_cmp_depth(iter, t) : gpq_he_algo_depth(kind, iter);
  if (depth < 0 || iter > 30 || (unsigned)depth > l || l > hectx.L) return 0;
  const std::vector<uint64_t> dw = words_of(hectx.p, "he_algo: Delta must be positive");
  if (dw.size() != 1 || !is_pow2(dw)) return 0;
  const unsigned s = G.mpi_get_nbits(hectx.p) - 1;
  if (s < 1 || s > 63 || hectx.Delta != (double)(1ull << s)) return 0;
  const unsigned logql = G.mpi_get_nbits(hectx.q[l]) - 1, logqL = G.mpi_get_nbits(hectx.q[hectx.L]) - 1;
  if (!is_pow2(words_of(hectx.q[hectx.L], "he_algo: q_L must be positive"))) return 0;
  for (unsigned k = 0; k <= (unsigned)depth; ++k)              // every modulus on the way is the power of two the evaluator assumes
    if (!is_pow2(words_of(hectx.q[l - k], "he_algo: q_l must be positive")) || G.mpi_get_nbits(hectx.q[l - k]) - 1 + k * s != logql) return 0;
  unsigned dimP = 0, dimB = 0;
  if (logql < 1 || logql > logqL || gpq_he_dims(c, logqL, logql, &dimP, nullptr, &dimB, nullptr) != GPQ_OK || dimP != hectx.dim ||
      gpq_ctx_pbits(c, dimP) != G.mpi_get_nbits(hectx.P) || gpq_ctx_pbits(c, dimP) + logqL != G.mpi_get_nbits(hectx.PqL))
    return 0;                                                  // hectx is not what gpq_he_dims derives from (logn, q_L): the per-call functions read it as it is
  unsigned W = (logql + 1) / 64 + 1, dimpt = 0;
  // he_exp's one plaintext, encoded by the host program's he_ecd (src/he-algo.c:444-448)
  std::unique_ptr<DevBuf> dm;
  if (kind == GPQ_ALGO_EXP) {
    if (!he_ecd || !hectx.slots) return 0;
    a /= (1 << iter);                                                                          // :444
    std::vector<gpq_zc> coeff(hectx.slots, a);
    he_pt_t pt{0, {nullptr}};
    alloc_poly(&pt.m, n);
    he_ecd(&pt, coeff.data());
    const unsigned bits = max_bits(&pt.m, n);
    if (pt.nu != hectx.Delta || bits / 64 + 1 > 32) { free_poly(&pt.m, n); return 0; }
    if (bits / 64 + 1 > W) W = bits / 64 + 1;
    dimpt = (unsigned)((logql + 1 + log2(pt.nu) + logn) / 59u + 1);                            // src/he-mult.c:169
    std::vector<uint64_t> hm((size_t)W * n);
    to_slab(hm.data(), &pt.m, n, W);
    free_poly(&pt.m, n);
    dm.reset(new DevBuf(hm.size() * 8));
    up(*dm, hm);
  }
  if (kind == SHIM_CMPPT) {                                    // he_addpt's plaintext, any integers (:543): only its width is needed before the plan
    const unsigned bits = max_bits(&cpt->m, n);
    if (bits / 64 + 1 > 32) return 0;
    if (bits / 64 + 1 > W) W = bits / 64 + 1;
  }
  const gpq_algo::Bounds bnd{hectx.bnd.Brs, hectx.bnd.Bmult, l};
  gpq_algo::Book book(c, W, 1, logqL, logql, s, dimpt, false, src->nu, src->B, &bnd);
  if (kind == SHIM_CMP) book.second_input(src2->nu, src2->B);
  if (kind == SHIM_CMPPT) book.pt_nu = cpt->nu;
  if (!(cmp ? gpq_algo::run_cmp(book, iter, t, kind == SHIM_CMPPT) : gpq_algo::run(book, kind, iter))) return 0;   // the depth or a constant does not fit
  const size_t wsb = cmp ? gpq_he_cmp_workspace_bytes(c, kind == SHIM_CMPPT, W, logqL, logql, s, iter, t, 1)
                         : gpq_he_algo_workspace_bytes(c, kind, W, logqL, logql, s, iter, 1);
  const unsigned cdim = (logql + 1 + s + logn) / 59u + 1;
  if (!wsb || !gpq_he_mulpt_const_fits(c, 1, 0, logql, cdim)) return 0;
  if (kind == SHIM_CMPPT) {                                    // the plan accepts: now the plaintext is converted and uploaded
    std::vector<uint64_t> hm((size_t)W * n);
    to_slab(hm.data(), &cpt->m, n, W);
    dm.reset(new DevBuf(hm.size() * 8));
    up(*dm, hm);
  }
  static hipEvent_t counted = nullptr;
  if (!counted && hipEventCreateWithFlags(&counted, hipEventDisableTiming) != hipSuccess) die("hipEventCreate failed");
  HostBuf count(8);
  DevBuf bad(8), ws(wsb);
  const unsigned logqo = logql - (unsigned)depth * s;
  // he_cmp(&d, &ct, &ct, ..): one ciphertext on both sides is converted, uploaded and counted once (as he_mul's squaring)
  const bool twice = kind == SHIM_CMP && src2->c0.coeffs == src->c0.coeffs && src2->c1.coeffs == src->c1.coeffs;
  const bool second = kind == SHIM_CMP && !twice;
  const poly_mpi_t *in[4] = {&src->c0, &src->c1, second ? &src2->c0 : nullptr, second ? &src2->c1 : nullptr};
  poly_mpi_t *out[2] = {&dst->c0, &dst->c1};
  StagedCall call(n, W, second ? 4 : 2, in, 2);
  call.Wdown = logqo / 64 + 1 < W ? logqo / 64 + 1 : W;        // the result is centred mod q_(l - depth)
  CallKey key(rlk, dimB, n);
  key.ride(call);
  call.prepare();
  key.settle();
  call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
    // the slab contract is "centred mod q_l" and the caller's integers may be anything: one counting pass over the source (the product by 1
    // into scratch the evaluator overwrites), whose count comes down with the first bytes
    uint64_t *t0 = ws.u64(), *t1 = t0 + (size_t)W * n;
    if (hipMemsetAsync(bad.p, 0, 4, nullptr) != hipSuccess) die("device memset failed");
    if (gpq_he_mulpt_const(c, t0, t1, x[0], x[1], 1, 0, W, logql, cdim, 0, 1, (unsigned *)bad.p, nullptr) != GPQ_OK) die("he_algo: counting pass failed");
    if (second && gpq_he_mulpt_const(c, t0, t1, x[2], x[3], 1, 0, W, logql, cdim, 0, 1, (unsigned *)bad.p, nullptr) != GPQ_OK)   // both are "centred mod q_l"
      die("he_algo: counting pass failed");
    if (hipMemcpyAsync(count.p, bad.p, 4, hipMemcpyDeviceToHost, nullptr) != hipSuccess || hipEventRecord(counted, nullptr) != hipSuccess) die("download failed");
    int rc;
    switch (kind) {
      case GPQ_ALGO_INV: rc = gpq_he_inv(c, o[0], o[1], x[0], x[1], key.k0, key.k1, W, logqL, logql, s, iter, 1, ws.p, nullptr); break;
      case GPQ_ALGO_SQRT: rc = gpq_he_sqrt(c, o[0], o[1], x[0], x[1], key.k0, key.k1, W, logqL, logql, s, iter, 1, ws.p, nullptr); break;
      case GPQ_ALGO_SIGMOID: rc = gpq_he_sigmoid(c, o[0], o[1], x[0], x[1], key.k0, key.k1, W, logqL, logql, s, 1, ws.p, nullptr); break;
      case GPQ_ALGO_LOG: rc = gpq_he_log(c, o[0], o[1], x[0], x[1], key.k0, key.k1, W, logqL, logql, s, 1, ws.p, nullptr); break;
      case SHIM_CMP:
        rc = gpq_he_cmp(c, o[0], o[1], x[0], x[1], second ? x[2] : x[0], second ? x[3] : x[1], key.k0, key.k1, W, logqL, logql, s, iter, t, 1, ws.p, nullptr);
        break;
      case SHIM_CMPPT: rc = gpq_he_cmppt(c, o[0], o[1], x[0], x[1], dm->u64(), key.k0, key.k1, W, logqL, logql, s, iter, t, 1, ws.p, nullptr); break;
      default: rc = gpq_he_exp(c, o[0], o[1], x[0], x[1], dm->u64(), dimpt, key.k0, key.k1, W, logqL, logql, s, iter, 1, ws.p, nullptr); break;
    }
    if (rc != GPQ_OK) die("he_algo: the evaluator failed");
  });
  if (hipEventSynchronize(counted) != hipSuccess) die("download failed");
  if (*(volatile unsigned *)count.p) return 0;                  // not centred: the reference's loop decides what that means
  call.deliver(out);
  dst->l = l - (unsigned)depth;
  dst->nu = book.v[book.result].nu;
  dst->B = book.v[book.result].B;
  return 1;
}

int gpq_shim_he_inv(he_ct_t *dst, const he_ct_t *src, const he_evk_t *rlk, unsigned iter) { return shim_evaluator(dst, src, rlk, GPQ_ALGO_INV, iter, 0); }
int gpq_shim_he_sqrt(he_ct_t *dst, const he_ct_t *src, const he_evk_t *rlk, unsigned iter) { return shim_evaluator(dst, src, rlk, GPQ_ALGO_SQRT, iter, 0); }
int gpq_shim_he_sigmoid(he_ct_t *dst, const he_ct_t *src, const he_evk_t *rlk) { return shim_evaluator(dst, src, rlk, GPQ_ALGO_SIGMOID, 0, 0); }
int gpq_shim_he_log(he_ct_t *dst, const he_ct_t *src, const he_evk_t *rlk) { return shim_evaluator(dst, src, rlk, GPQ_ALGO_LOG, 0, 0); }
int gpq_shim_he_exp(he_ct_t *dst, _Complex double a, const he_ct_t *src, const he_evk_t *rlk, unsigned iter) {
  return shim_evaluator(dst, src, rlk, GPQ_ALGO_EXP, iter, a);
}
// he_cmp: alpha as the reference takes it, t by its expression (gpq_he_cmp_rounds: 0 outside 1..52, where that expression is undefined)
int gpq_shim_he_cmp(he_ct_t *dst, const he_ct_t *ct1, const he_ct_t *ct2, const he_evk_t *rlk, unsigned iter, unsigned alpha) {
  const int t = gpq_he_cmp_rounds(alpha);
  return t < 0 ? 0 : shim_evaluator(dst, ct1, rlk, SHIM_CMP, iter, 0, ct2, nullptr, (unsigned)t);
}
// he_cmppt: t, not alpha -- the reference's own expression (:537-538) is undefined for every alpha, and the library does not guess it
int gpq_shim_he_cmppt(he_ct_t *dst, const he_ct_t *ct, const he_pt_t *pt, const he_evk_t *rlk, unsigned iter, unsigned t) {
  return shim_evaluator(dst, ct, rlk, SHIM_CMPPT, iter, 0, nullptr, pt, t);
}
