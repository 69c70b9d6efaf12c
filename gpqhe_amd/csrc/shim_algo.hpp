// shim_algo.hpp -- he_gemv / he_sum / he_idx (src/he-algo.c:47-113) with the reference's signatures.  Included inside mpi_shim.hip's extern "C"
// block.  With q_l and q_(l-1) powers of two (and Delta = q_l / q_(l-1)) the whole body is one gpq_he_gemv: ct goes up once (or is used where
// it is resident), the diagonals he_ecd encodes go up once, the keys come through the key cache, ct_dest comes back once -- or, for a matrix seen
// before (shim_gemv_plans.hpp), one gpq_he_gemv_planned on the plan made then: no he_ecd, no conversion, no upload of diagonals.  Otherwise the
// reference's loop runs over this library's per-call functions: the same words, no speed-up.  l / nu / B are replayed on the host in the
// reference's order, as doubles.

typedef _Complex double gpq_zc;
typedef std::function<gpq_zc(unsigned, unsigned)> GemvMatrix;     // A[r * slots + c]

static void gemv_split(unsigned slots, unsigned *n1, unsigned *n2) {   // src/he-algo.c:51-54
  unsigned a = (unsigned)sqrt((double)slots);
  if (slots != a * a) a = (unsigned)sqrt((double)(2 * slots));
  *n1 = a;
  *n2 = slots / a;
}

static void zrotdiag_of(std::vector<gpq_zc> &rot, const GemvMatrix &A, unsigned m, unsigned idx, int r) {   // src/he-algo.c:29-42
  std::vector<gpq_zc> diag(m);
  for (unsigned i = 0; i < m; ++i) diag[i] = A(i % m, (idx + i) % m);
  rot.resize(m);
  for (unsigned i = 0; i < m; ++i) {
    int k = ((int)i + r) % (int)m;
    if (k < 0) k += (int)m;
    rot[i] = diag[k];
  }
}

static void alloc_poly(poly_mpi_t *p, unsigned n) {
  p->coeffs = (gpq_MPI *)calloc(n, sizeof(gpq_MPI));
  if (!p->coeffs) die("he_gemv: host allocation failed");
  for (unsigned i = 0; i < n; ++i) p->coeffs[i] = G.mpi_new(0);
}
static void free_poly(poly_mpi_t *p, unsigned n) {
  if (!p->coeffs) return;
  for (unsigned i = 0; i < n; ++i) G.mpi_release((MPI)p->coeffs[i]);
  free(p->coeffs);
  p->coeffs = nullptr;
}

// The reference's loop, call by call (:62-88), over this library's he_copy_ct / he_rot / he_mulpt / he_add / he_rs.
static void gemv_loop(he_ct_t *ct_dest, const GemvMatrix &A, const he_ct_t *ct, const he_evk_t *rk) {
  if (!he_ecd) die("he_gemv: the host program provides no he_ecd (src/he-encode.c)");
  const unsigned slots = hectx.slots, n = polyctx.n;
  unsigned n1, n2;
  gemv_split(slots, &n1, &n2);
  he_pt_t pt{0, {nullptr}};
  he_ct_t inner{}, outer{}, ct_rot{};
  alloc_poly(&pt.m, n);
  for (he_ct_t *t : {&inner, &outer, &ct_rot}) { alloc_poly(&t->c0, n); alloc_poly(&t->c1, n); }
  std::vector<gpq_zc> rd;
  for (unsigned i = 0; i < n2; ++i) {
    const int shift = (int)(i * n1);
    for (unsigned j = 0; j < n1; ++j) {
      additive(&ct_rot, ct, nullptr, nullptr, 5);                                                // he_copy_ct
      automorphism(&ct_rot, &rk[j], false, j);                                                   // he_rot(&ct_rot, j, rk)
      zrotdiag_of(rd, A, slots, shift + j, -shift);
      he_ecd(&pt, rd.data());
      he_mulpt(&ct_rot, &ct_rot, &pt);
      if (!j) additive(&inner, &ct_rot, nullptr, nullptr, 5);
      else additive(&inner, &inner, &ct_rot, nullptr, 0);
    }
    automorphism(&inner, &rk[shift], false, (unsigned)shift);
    if (!i) additive(&outer, &inner, nullptr, nullptr, 5);
    else additive(&outer, &outer, &inner, nullptr, 0);
  }
  if (ct_dest != &outer) additive(ct_dest, &outer, nullptr, nullptr, 5);
  rescale_common(ct_dest, true);                                                                 // he_rs
  free_poly(&pt.m, n);
  for (he_ct_t *t : {&inner, &outer, &ct_rot}) { free_poly(&t->c0, n); free_poly(&t->c1, n); }
}

// gpq_mpi_shim_set_device_ecd(1): the plan of a matrix not seen before, with the diagonals encoded ON THE DEVICE from the slots^2 entries
// (gpq_gemv_plan_create_from_matrix) instead of slots he_ecd calls, slots n conversions and an upload of slots W n words.  The roots are the
// host's own polyctx.ring.zetas, read by stride, so the words are those of an encoder that reads that table (src/he-encode.c does), under any
// libm; pt.nu is hectx.Delta as src/he-encode.c:109 sets it.  nullptr -- and the caller goes on as if the switch were off -- when a
// coefficient has no image (bad != 0), the plan is not exact, or the slot count exceeds what one workgroup holds.  `key` is consumed on success only.
static GemvPlanEntry *gemv_plan_on_device(gpq_ctx *c, GemvPlanKey &key, const GemvMatrix &A, const gpq_zc *raw, unsigned slots, unsigned logql, unsigned logDelta) {
  if (!polyctx.ring.zetas || slots > 8192 || slots > polyctx.n / 2) return nullptr;
  gpq_ecd_plan *ep = nullptr;
  if (gpq_ecd_plan_create(c, &ep, slots, (const double *)polyctx.ring.zetas, polyctx.m / 4) != GPQ_OK) die("he_gemv: cannot build the encoder's tables");
  std::vector<gpq_zc> built;
  if (!raw) {                                                      // he_sum / he_idx: the matrix they describe, slots^2 x 16 bytes
    built.resize((size_t)slots * slots);
    for (unsigned r = 0; r < slots; ++r)
      for (unsigned col = 0; col < slots; ++col) built[(size_t)r * slots + col] = A(r, col);
    raw = built.data();
  }
  const size_t bytes = (size_t)slots * slots * sizeof(gpq_zc);
  DevBuf dA(bytes);
  if (gpq_upload(dA.p, raw, bytes, nullptr) != GPQ_OK) die("upload failed");
  const unsigned dimpt = (logql + 1 + logDelta + polyctx.logn) / 59u + 1;                                          // src/he-mult.c:169 with nu = Delta
  gpq_gemv_plan *made = nullptr;
  const int rc = gpq_gemv_plan_create_from_matrix(c, &made, ep, (const double *)dA.p, logDelta, logql, dimpt, nullptr);
  gpq_ecd_plan_destroy(ep);
  if (rc == GPQ_ERR_INVALID) return nullptr;                       // a coefficient at or beyond 2^63: the host's encoder decides what that means
  if (rc != GPQ_OK) die("he_gemv: cannot build the plan");
  int exact = 0;
  (void)gpq_gemv_plan_info(made, nullptr, nullptr, nullptr, &exact);
  if (!exact) { gpq_gemv_plan_destroy(made); return nullptr; }
  const unsigned dbits = gpq_gemv_plan_diag_bits(made);
  GemvPlanEntry e;
  e.key = std::move(key); e.plan = made; e.nu = hectx.Delta; e.bits = dbits > logql + 1 ? dbits : logql + 1;
  return gemv_plan_insert(std::move(e));
}

// kind 0: he_gemv (raw = the caller's slots x slots matrix), 1: he_sum, 2: he_idx (idx): what the plan cache keys on (shim_gemv_plans.hpp)
static void gemv_impl(he_ct_t *ct_dest, const GemvMatrix &A, const he_ct_t *ct, const he_evk_t *rk, unsigned kind, unsigned idx, const gpq_zc *raw) {
  SHIM_CALL();
  need_hectx();
  if (!he_ecd && !g_device_ecd) die("he_gemv: the host program provides no he_ecd (src/he-encode.c)");
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, l = ct->l, slots = hectx.slots;
  if (!slots || l < 1) die("he_gemv: needs slots > 0 and a level to rescale to");
  unsigned n1, n2;
  gemv_split(slots, &n1, &n2);
  const std::vector<uint64_t> qw = words_of(hectx.q[l], "he_gemv: q_l must be positive"), qw1 = words_of(hectx.q[l - 1], "he_gemv: q_(l-1) must be positive");
  const unsigned logql = G.mpi_get_nbits(hectx.q[l]) - 1, logql1 = G.mpi_get_nbits(hectx.q[l - 1]) - 1;
  int e2 = 0;
  const bool delta_pow2 = std::frexp(hectx.Delta, &e2) == 0.5 && e2 >= 2 && (unsigned)(e2 - 1) == logql - logql1;
  std::set<unsigned> rots;
  for (unsigned j = 0; j < n1; ++j) rots.insert(j);
  for (unsigned i = 0; i < n2; ++i) rots.insert(i * n1);
  if (!is_pow2(qw) || !is_pow2(qw1) || !delta_pow2 || logql1 >= logql || rots.size() > g_key_slots) { gemv_loop(ct_dest, A, ct, rk); return; }
  // a plan for this very matrix at this level?  Then nothing is encoded, converted or uploaded for the diagonals.
  GemvPlanKey key;
  GemvPlanEntry *hit = nullptr;
  if (g_gemv_plan_slots) {
    key.kind = kind; key.idx = kind == 2 ? idx : 0; key.n = n; key.slots = slots; key.l = l; key.logql = logql; key.Delta = hectx.Delta;
    if (kind == 0) key.A.assign((const unsigned char *)raw, (const unsigned char *)raw + (size_t)slots * slots * sizeof(gpq_zc));
    hit = gemv_plan_find(key);
  }
  if (!hit && g_device_ecd && g_gemv_plan_slots) hit = gemv_plan_on_device(c, key, A, raw, slots, logql, logql - logql1);
  // otherwise the diagonals, encoded by the host program's he_ecd on the reference's vectors in the reference's order (:70-72)
  if (!hit && !he_ecd) die("he_gemv: the host program provides no he_ecd (src/he-encode.c)");
  std::vector<he_pt_t> pts(hit ? 0 : slots);
  std::vector<gpq_zc> rd;
  unsigned bits = logql + 1;
  bool same_nu = true;
  if (hit) bits = hit->bits;
  for (unsigned i = 0; i < n2 && !hit; ++i)
    for (unsigned j = 0; j < n1; ++j) {
      he_pt_t &pt = pts[i * n1 + j];
      pt.nu = 0;
      alloc_poly(&pt.m, n);
      zrotdiag_of(rd, A, slots, i * n1 + j, -(int)(i * n1));
      he_ecd(&pt, rd.data());
      const unsigned b = max_bits(&pt.m, n);
      if (b > bits) bits = b;
      same_nu = same_nu && pt.nu == pts[0].nu;
    }
  auto release_pts = [&]() { for (he_pt_t &pt : pts) free_poly(&pt.m, n); };
  if (!same_nu) { release_pts(); gemv_loop(ct_dest, A, ct, rk); return; }
  const double ptnu = hit ? hit->nu : pts[0].nu;                   // every diagonal's
  // l / nu / B as the reference's he_mulpt (src/he-mult.c:162-164), he_add (src/he-add.c:36-38) in loop order, he_copy_ct, he_rs (src/he-rescale.c:36-38)
  double onu = 0, oB = 0;
  for (unsigned i = 0; i < n2; ++i) {
    double inu = 0, iB = 0;
    for (unsigned j = 0; j < n1; ++j) {
      const double pnu = ct->nu * ptnu, pB = ct->B * ptnu;
      if (!j) { inu = pnu; iB = pB; } else { inu = inu >= pnu ? inu : pnu; iB = iB + pB; }
    }
    if (!i) { onu = inu; oB = iB; } else { onu = onu >= inu ? onu : inu; oB = oB + iB; }
  }
  const unsigned W = bits / 64 + 1;
  const unsigned nbPqL = G.mpi_get_nbits(hectx.PqL);
  const unsigned dimB = (logql + 1 + nbPqL + polyctx.logn) / 59 + 1, dimP = hectx.dim;                                // src/he-automorphism.c:52
  const unsigned dimpt = (unsigned)((logql + 1 + log2(ptnu) + polyctx.logn) / 59u + 1);                            // src/he-mult.c:169
  const size_t big = (size_t)W * n;
  gpq_gemv_plan *plan = hit ? hit->plan : nullptr;
  std::unique_ptr<DevBuf> dg;
  std::vector<uint64_t> hd;
  if (!hit) {
    hd.resize((size_t)slots * big);
    for (unsigned d = 0; d < slots; ++d) to_slab(hd.data() + d * big, &pts[d].m, n, W);
    release_pts();
    dg.reset(new DevBuf(hd.size() * 8));
    up(*dg, hd);
    if (g_gemv_plan_slots && W <= 32) {                             // a plan that is not exact (or does not fit the context) is not kept: today's path
      gpq_gemv_plan *made = nullptr;
      int exact = 0;
      if (gpq_gemv_plan_create(c, &made, (const uint64_t *)dg->p, slots, W, logql, dimpt, nullptr) != GPQ_OK) die("he_gemv: cannot build the plan");
      (void)gpq_gemv_plan_info(made, nullptr, nullptr, nullptr, &exact);
      if (exact) {
        GemvPlanEntry e;
        e.key = std::move(key); e.plan = made; e.nu = ptnu; e.bits = bits;
        plan = gemv_plan_insert(std::move(e))->plan;
      } else gpq_gemv_plan_destroy(made);
    }
  }
  if (plan) {                                                      // keys of the rotations the plan reads only (he_idx: rk[0] alone)
    std::vector<unsigned char> needed(slots, 0);
    (void)gpq_gemv_plan_rotations(plan, needed.data());
    for (auto it = rots.begin(); it != rots.end();) it = needed[*it] ? std::next(it) : rots.erase(it);
  }
  DevBuf ws(plan ? gpq_he_gemv_planned_workspace_bytes(c, plan, W, dimB, dimP, 1) : gpq_he_gemv_workspace_bytes(c, W, slots, dimB, dimP, dimpt, 1));
  std::vector<const uint64_t *> k0(slots, nullptr), k1(slots, nullptr);
  for (unsigned r : rots) {                                        // at most g_key_slots keys: none of them is evicted by the next one
    KeyPrint kp(&rk[r], dimB, n);
    if (kp.parts < 2) kp.task(0); else workers().run(kp.parts, kp.task);
    uint64_t *d0, *d1;
    key_on_device(kp, &d0, &d1);
    k0[r] = d0; k1[r] = d1;
  }
  const poly_mpi_t *in[2] = {&ct->c0, &ct->c1};
  poly_mpi_t *out[2] = {&ct_dest->c0, &ct_dest->c1};
  StagedCall call(n, W, 2, in, 2);
  call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
    const int rc = plan ? gpq_he_gemv_planned(c, o[0], o[1], x[0], x[1], plan, k0.data(), k1.data(), W, logql - logql1, dimB, dimP, 1, ws.p, nullptr)
                        : gpq_he_gemv(c, o[0], o[1], x[0], x[1], (const uint64_t *)dg->p, k0.data(), k1.data(), slots, W, logql, logql - logql1,
                                      dimB, dimP, dimpt, 1, ws.p, nullptr);
    if (rc != GPQ_OK) die("he_gemv failed");
  }, out);
  ct_dest->l = l - 1;                                                                          // he_copy_ct + he_rs
  ct_dest->nu = onu / hectx.Delta;
  ct_dest->B = oB / hectx.Delta + hectx.bnd.Brs;
}

void he_gemv(he_ct_t *ct_dest, const _Complex double *A, const he_ct_t *ct, const he_evk_t *rk) {
  const unsigned m = hectx.slots;
  gemv_impl(ct_dest, [A, m](unsigned r, unsigned col) { return A[(size_t)r * m + col]; }, ct, rk, 0, 0, A);
}
// he_sum, :95-103: A = ones in row 0 (the slots x slots matrix is never built: zrotdiag reads it through this function)
void he_sum(he_ct_t *ct_sum, const he_ct_t *ct, const he_evk_t *rk) {
  gemv_impl(ct_sum, [](unsigned r, unsigned) { return r == 0 ? (gpq_zc)1.0 : (gpq_zc)0.0; }, ct, rk, 1, 0, nullptr);
}
// he_idx, :105-113: A[idx][idx] = 1
void he_idx(he_ct_t *ct_idx, const he_ct_t *ct, const unsigned int idx, const he_evk_t *rk) {
  gemv_impl(ct_idx, [idx](unsigned r, unsigned col) { return r == idx && col == idx ? (gpq_zc)1.0 : (gpq_zc)0.0; }, ct, rk, 2, idx, nullptr);
}
// 1: he_gemv / he_sum / he_idx encode the diagonals of a matrix they have no plan for on the device (gemv_plan_on_device); 0 (default): the
// host program's he_ecd does, as ever
void gpq_mpi_shim_set_device_ecd(int on) {
  SHIM_CALL();
  g_device_ecd = on != 0;
}
// Entries of he_gemv's plan cache (default 4, least recently used out); 0 frees every plan and makes every call encode, convert and upload
// its diagonals and run gpq_he_gemv, as before the cache existed.
void gpq_shim_gemv_plan_cache(unsigned entries) {
  SHIM_CALL();
  g_gemv_plan_slots = entries;
  gemv_plans_drop(entries);
}
