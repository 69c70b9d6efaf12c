// gemv_multi.hpp -- he_gemv for SEVERAL fixed matrices on the same ciphertexts (include/gpqhe_hip.h, "he_gemv for several matrices"): the plan
// set and the call.  Part of bridge.hip's translation unit, after gemv_plan.hpp (it uses that file's plan_usable, ranges_overlap and
// inner_finish); the kernel is gemv_mac_multi in ntt_kernels.hpp, launched by engine.hip's gpq_gemv_mac_multi.
//
// What the plans of a set share depends only on the ciphertext: the hoisted baby rotations, their rns_decompose + forward transform, and
// the reads of those transforms inside every giant step.  All of it runs once, over the union of the plans' live baby rotations and the
// largest `dim`; everything behind the inner sums (inverse transform, reconstruction, giant rotation, wrapping sum, he_rs) runs per plan
// exactly as gpq_he_gemv_planned runs it.  Nothing new to prove: a residue of a rotation does not depend on how many limbs lie next to it,
// and the sums leave gemv_mac_multi as canonical residues of the same terms, so output t is gpq_he_gemv_planned's for plans[t] word for word.
#pragma once

struct gpq_gemv_multi {
  gpq_ctx *ctx = nullptr;
  unsigned count = 0, groups = 0, slots = 0, n1 = 0, n2 = 0, logql = 0, dim = 0;   // dim: the largest among the plans
  std::vector<const gpq_gemv_plan *> plans;   // borrowed
  std::vector<unsigned> baby;                 // union of the plans' live baby rotations, ascending
  // per (giant step i, plan group g) at [i * groups + g]: where its entries start in d_entries (in entries) and how many there are
  std::vector<unsigned> first, nentries;
  gpq_dev<unsigned> d_entries;                // [entry][1 + NP]: union slot, then per plan of the group its diagonal or GEMV_NOT_LIVE
  size_t bytes = 0;
};

namespace {
constexpr unsigned kGemvMultiMax = 16, kGemvMultiNP = GPQ_GEMV_MULTI_NP;

struct MultiLayout { size_t rb, hat, acc, p, g, ws, total; };
int multi_layout(gpq_ctx *c, const gpq_gemv_multi *ms, unsigned W, unsigned dimB, unsigned dimP, unsigned m, MultiLayout *l) {
  const size_t nb = ms->baby.size(), big = (size_t)m * W * c->n * 8, slab = (size_t)m * ms->dim * c->n * 8;
  l->rb = 2 * align64(nb * big);                       // the union's baby rotations, c0 | c1
  l->hat = align64(2 * nb * slab);                     // ... decomposed and transformed over the largest dim
  l->acc = kGemvMultiNP * align64(2 * slab);           // one giant step's sums of one plan group
  l->p = 2 * align64(big);                             // ... of one plan, as words
  l->g = 2 * align64(big);                             // one giant rotation
  const size_t wn = nb ? gpq_he_rot_hoisted_workspace_bytes(c, W, dimB, dimP, (unsigned)nb, m) : 0, w1 = gpq_he_rot_hoisted_workspace_bytes(c, W, dimB, dimP, 1, m);
  if ((nb && !wn) || !w1) return GPQ_ERR_INVALID;      // (the rotation plan's message is in gpq_last_error)
  l->ws = align64(wn > w1 ? wn : w1);
  l->total = l->rb + l->hat + l->acc + l->p + l->g + l->ws;
  return GPQ_OK;
}
}  // namespace

extern "C" unsigned gpq_gemv_multi_width(void) { return kGemvMultiNP; }

extern "C" void gpq_gemv_multi_destroy(gpq_gemv_multi *ms) {
  if (!ms) return;
  DeviceScope on_device(ms->ctx->device);
  delete ms;
}

extern "C" int gpq_gemv_multi_info(const gpq_gemv_multi *ms, unsigned *count, unsigned *baby, unsigned *dim, size_t *bytes) {
  if (!ms) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_multi_info: null set");
  if (count) *count = ms->count;
  if (baby) *baby = (unsigned)ms->baby.size();
  if (dim) *dim = ms->dim;
  if (bytes) *bytes = ms->bytes;
  return GPQ_OK;
}

extern "C" int gpq_gemv_multi_rotations(const gpq_gemv_multi *ms, unsigned char *needed) {
  if (!ms || !needed) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_multi_rotations: null argument");
  memset(needed, 0, ms->slots);
  for (const gpq_gemv_plan *p : ms->plans) {
    for (unsigned j : p->baby) needed[j] = 1;
    for (unsigned i = 0; i < p->n2; ++i) if (p->nterms[i]) needed[i * p->n1] = 1;
  }
  return GPQ_OK;
}

extern "C" int gpq_gemv_multi_create(gpq_ctx *c, gpq_gemv_multi **out, const gpq_gemv_plan *const *plans, unsigned count, void *stream) {
  if (!c || !out || !plans) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_multi_create: null argument");
  if (count < 1 || count > kGemvMultiMax) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_multi_create: %u plans (1..%u)", count, kGemvMultiMax);
  int rc;
  for (unsigned t = 0; t < count; ++t) {
    if ((rc = plan_usable(c, plans[t], "gpq_gemv_multi_create"))) return rc;
    if (plans[t]->slots != plans[0]->slots || plans[t]->logql != plans[0]->logql)
      return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_multi_create: plan %u has %u slots at q = 2^%u, plan 0 has %u at 2^%u: one set, one shape", t,
                      plans[t]->slots, plans[t]->logql, plans[0]->slots, plans[0]->logql);
  }
  if (gpq_capturing((hipStream_t)stream))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_multi_create allocates and copies its tables: not inside a stream capture");
  std::unique_ptr<gpq_gemv_multi, void (*)(gpq_gemv_multi *)> ms(new (std::nothrow) gpq_gemv_multi(), gpq_gemv_multi_destroy);
  if (!ms) return gpq_fail(GPQ_ERR_NOMEM, "out of host memory");
  const gpq_gemv_plan *p0 = plans[0];
  ms->ctx = c; ms->count = count; ms->groups = (count + kGemvMultiNP - 1) / kGemvMultiNP;
  ms->slots = p0->slots; ms->n1 = p0->n1; ms->n2 = p0->n2; ms->logql = p0->logql;
  ms->plans.assign(plans, plans + count);
  std::vector<unsigned char> in_union(ms->n1, 0);
  for (const gpq_gemv_plan *p : ms->plans) {
    if (p->dim > ms->dim) ms->dim = p->dim;
    for (unsigned j : p->baby) in_union[j] = 1;
  }
  for (unsigned j = 0; j < ms->n1; ++j) if (in_union[j]) ms->baby.push_back(j);
  // per giant step and plan group: the union slots that some plan of the group reads, with every plan's diagonal there
  const unsigned stride = 1 + kGemvMultiNP;
  std::vector<unsigned> entries;
  ms->first.assign((size_t)ms->n2 * ms->groups, 0);
  ms->nentries.assign((size_t)ms->n2 * ms->groups, 0);
  for (unsigned i = 0; i < ms->n2; ++i)
    for (unsigned g = 0; g < ms->groups; ++g) {
      const size_t at = (size_t)i * ms->groups + g;
      ms->first[at] = (unsigned)(entries.size() / stride);
      for (unsigned u = 0; u < ms->baby.size(); ++u) {
        const unsigned k = i * ms->n1 + ms->baby[u];
        unsigned e[1 + kGemvMultiNP];
        bool any = false;
        e[0] = u;
        for (unsigned t = 0; t < kGemvMultiNP; ++t) {
          const unsigned pl = g * kGemvMultiNP + t;
          const bool live = pl < count && ms->plans[pl]->live_diag[k];
          e[1 + t] = live ? k : GEMV_NOT_LIVE;
          any = any || live;
        }
        if (!any) continue;
        entries.insert(entries.end(), e, e + stride);
        ++ms->nentries[at];
      }
    }
  if (!entries.empty()) {
    DeviceScope on_device(c->device);
    ms->bytes = entries.size() * sizeof(unsigned);
    HIP_TRY(ms->d_entries.alloc(ms->bytes));
    HIP_TRY(hipMemcpy(ms->d_entries, entries.data(), ms->bytes, hipMemcpyHostToDevice));
  }
  *out = ms.release();
  return GPQ_OK;
}

extern "C" size_t gpq_he_gemv_multi_workspace_bytes(gpq_ctx *c, const gpq_gemv_multi *ms, unsigned W, unsigned dimB, unsigned dimP, unsigned batch) {
  if (!c || !ms || !batch || !W) return 0;
  MultiLayout l;
  return multi_layout(c, ms, W, dimB, dimP, batch < c->set.chunk ? batch : c->set.chunk, &l) == GPQ_OK ? l.total : 0;
}

extern "C" int gpq_he_gemv_multi(gpq_ctx *c, uint64_t *const *out_c0, uint64_t *const *out_c1, const uint64_t *c0, const uint64_t *c1,
                                 const gpq_gemv_multi *ms, const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logDelta,
                                 unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_he_gemv_multi");
  if (rc) return rc;
  if (!ms) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: null set");
  if (ms->ctx != c) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: the set belongs to another context");
  const unsigned logql = ms->logql, n1 = ms->n1, count = ms->count;
  if (!out_c0 || !out_c1 || !c0 || !c1 || !rk0 || !rk1 || !workspace || logDelta >= logql || W < (logql + 63) / 64 || W > 32)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: bad arguments (W words must hold q = 2^%u, Delta below q)", logql);
  const size_t n = c->n, bigpoly = (size_t)W * n, words = batch * bigpoly;
  std::vector<const uint64_t *> slabs{c0, c1};                            // the inputs, then every output: no two may overlap
  for (unsigned t = 0; t < count; ++t) {
    if (!out_c0[t] || !out_c1[t]) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: output %u is NULL", t);
    slabs.push_back(out_c0[t]); slabs.push_back(out_c1[t]);
  }
  for (size_t a = 2; a < slabs.size(); ++a)
    for (size_t b = 0; b < a; ++b)
      if (ranges_overlap(slabs[a], words, slabs[b], words))
        return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: the outputs alias each other or an input");
  const unsigned nb = (unsigned)ms->baby.size();
  std::vector<const uint64_t *> bk0(nb), bk1(nb);
  for (unsigned r = 0; r < nb; ++r) {
    bk0[r] = rk0[ms->baby[r]]; bk1[r] = rk1[ms->baby[r]];
    if (!bk0[r] || !bk1[r]) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: key %u is NULL (a live baby rotation of the set)", ms->baby[r]);
  }
  for (const gpq_gemv_plan *p : ms->plans)
    for (unsigned i = 0; i < p->n2; ++i)
      if (p->nterms[i] && (!rk0[i * n1] || !rk1[i * n1])) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: key %u is NULL (a live giant rotation of the set)", i * n1);
  hipStream_t s = (hipStream_t)stream;
  const unsigned m = batch < c->set.chunk ? batch : c->set.chunk;
  MultiLayout l;
  if (multi_layout(c, ms, W, dimB, dimP, m, &l)) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: unsupported shape");
  char *w = (char *)workspace;
  uint64_t *RB0 = (uint64_t *)w, *RB1 = (uint64_t *)(w + l.rb / 2); w += l.rb;
  uint64_t *hat = (uint64_t *)w; w += l.hat;
  char *acc = w; w += l.acc;
  uint64_t *P0 = (uint64_t *)w, *P1 = (uint64_t *)(w + l.p / 2); w += l.p;
  uint64_t *G0 = (uint64_t *)w, *G1 = (uint64_t *)(w + l.g / 2); w += l.g;
  void *ws = w;
  const unsigned stride = 1 + kGemvMultiNP;
  std::vector<unsigned char> first(count);
  for (unsigned k0 = 0; k0 < batch; k0 += m) {
    const unsigned polys = batch - k0 < m ? batch - k0 : m;
    const size_t o = k0 * bigpoly, rslab = (size_t)polys * ms->dim * n;
    for (unsigned t = 0; t < count; ++t)
      if (ms->plans[t]->baby.empty()) {                                    // the zero matrix
        HIP_TRY(hipMemsetAsync(out_c0[t] + o, 0, polys * bigpoly * 8, s));
        HIP_TRY(hipMemsetAsync(out_c1[t] + o, 0, polys * bigpoly * 8, s));
      }
    if (!nb) continue;
    uint64_t *hat0 = hat, *hat1 = hat + nb * rslab;
    if ((rc = gpq_he_rot_hoisted(c, RB0, RB1, c0 + o, c1 + o, ms->baby.data(), bk0.data(), bk1.data(), nb, W, logql, dimB, dimP, polys, ws, stream))) return rc;   // src/he-algo.c:63-68
    {
      StageRange stage("gpq_he_gemv_multi: rns_decompose + forward transform of the baby rotations (once per group, for every plan)");
      if ((rc = launch_decompose(c, hat0, RB0, W, 0, ms->dim, nb * polys, s))) return rc;
      if ((rc = launch_decompose(c, hat1, RB1, W, 0, ms->dim, nb * polys, s))) return rc;
      if ((rc = gpq_hoist_forward(c, hat, ms->dim, 2 * nb * polys, s))) return rc;
    }
    std::fill(first.begin(), first.end(), 1);
    for (unsigned i = 0; i < ms->n2; ++i)
      for (unsigned g = 0; g < ms->groups; ++g) {
        const size_t at = (size_t)i * ms->groups + g;
        if (!ms->nentries[at]) continue;                                   // no plan of the group has a live diagonal in this step
        StageRange stage("gpq_he_gemv_multi: one giant step of one plan group (inner sums, then per plan the rotation)");
        gpq_gemv_multi_arg arg[kGemvMultiNP];
        for (unsigned t = 0; t < kGemvMultiNP; ++t) {
          const unsigned pl = g * kGemvMultiNP + t;
          const gpq_gemv_plan *p = pl < count ? ms->plans[pl] : nullptr;
          uint64_t *a0 = (uint64_t *)(acc + t * (l.acc / kGemvMultiNP));
          if (p && p->nterms[i]) arg[t] = {p->d_hat, a0, a0 + (size_t)polys * p->dim * n, p->dim};
          else arg[t] = {nullptr, nullptr, nullptr, 0};
        }
        if ((rc = gpq_gemv_mac_multi(c, arg, hat0, hat1, ms->d_entries + (size_t)ms->first[at] * stride, ms->nentries[at], ms->dim, polys, s))) return rc;   // :70-78
        for (unsigned t = 0; t < kGemvMultiNP; ++t) {
          if (!arg[t].dim) continue;
          const unsigned pl = g * kGemvMultiNP + t;
          uint64_t *o0 = out_c0[pl] + o, *o1 = out_c1[pl] + o;
          if ((rc = inner_finish(c, ms->plans[pl], P0, P1, arg[t].acc0, W, polys, stream))) return rc;
          const unsigned shift = i * n1;
          uint64_t *g0 = first[pl] ? o0 : G0, *g1 = first[pl] ? o1 : G1;                                                   // :80-84
          if ((rc = gpq_he_rot_hoisted(c, g0, g1, P0, P1, &shift, rk0 + shift, rk1 + shift, 1, W, logql, dimB, dimP, polys, ws, stream))) return rc;
          if (!first[pl] && ((rc = gpq_big_addsub(c, o0, o0, G0, W, polys, 0, stream)) || (rc = gpq_big_addsub(c, o1, o1, G1, W, polys, 0, stream)))) return rc;
          first[pl] = 0;
        }
      }
  }
  for (unsigned t = 0; t < count; ++t) {
    if ((rc = gpq_he_rs(c, out_c0[t], out_c1[t], W, 0, logql, batch, stream))) return rc;                                // the adds' mpi_smod
    if (logDelta && (rc = gpq_he_rs(c, out_c0[t], out_c1[t], W, logDelta, logql - logDelta, batch, stream))) return rc;   // :87, src/he-rescale.c:33-54
  }
  return launched("gpq_he_gemv_multi");
}
