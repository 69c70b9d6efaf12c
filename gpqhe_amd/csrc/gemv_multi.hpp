// gemv_multi.hpp -- he_gemv for SEVERAL fixed matrices on the same ciphertexts (include/gpqhe_hip.h, "he_gemv for several matrices"): the plan
// set and the call.  Part of bridge.hip's translation unit, after gemv_plan.hpp (it uses that file's plan_usable and its driver gemv_call);
// the kernel is gemv_mac_multi in ntt_kernels.hpp, launched by engine.hip's gpq_gemv_mac_multi.
//
// What the plans of a set share depends only on the ciphertext: the hoisted baby rotations, their rns_decompose + forward transform, and
// the reads of those transforms inside every giant step.  gemv_call runs the first two once, over the union of the plans' live baby
// rotations and the largest `dim`, and everything behind the inner sums (inverse transform, reconstruction, giant rotation, wrapping sum,
// he_rs) per plan: the code gpq_he_gemv_planned runs, not a copy of it.  This file adds the third: one gemv_mac_multi launch per giant step
// and group of NP plans, where the planned call launches gemv_mac.  So only the inner sums have anything to prove, and it is little: a
// residue of a rotation does not depend on how many limbs lie next to it, and the sums leave gemv_mac_multi as canonical residues of the
// same terms, so output t is gpq_he_gemv_planned's for plans[t] word for word.
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
  return gemv_call_workspace_bytes(c, ms->baby.size(), ms->dim, kGemvMultiNP, W, dimB, dimP, batch);
}

extern "C" int gpq_he_gemv_multi(gpq_ctx *c, uint64_t *const *out_c0, uint64_t *const *out_c1, const uint64_t *c0, const uint64_t *c1,
                                 const gpq_gemv_multi *ms, const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logDelta,
                                 unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_he_gemv_multi");
  if (rc) return rc;
  if (!ms) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: null set");
  if (ms->ctx != c) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv_multi: the set belongs to another context");
  // one gemv_mac_multi launch for the NP plans from `first` on: the set's entries of (giant step, plan group), written for exactly these plans
  auto inner_sums = [&](unsigned i, unsigned first, unsigned polys, const uint64_t *hat0, const uint64_t *hat1, uint64_t *const *acc) {
    gpq_gemv_multi_arg arg[kGemvMultiNP];
    for (unsigned t = 0; t < kGemvMultiNP; ++t) {
      const gpq_gemv_plan *p = acc[t] ? ms->plans[first + t] : nullptr;
      if (p) arg[t] = {p->d_hat, acc[t], acc[t] + (size_t)polys * p->dim * c->n, p->dim};
      else arg[t] = {nullptr, nullptr, nullptr, 0};
    }
    const size_t at = (size_t)i * ms->groups + first / kGemvMultiNP;
    return gpq_gemv_mac_multi(c, arg, hat0, hat1, ms->d_entries + (size_t)ms->first[at] * (1 + kGemvMultiNP), ms->nentries[at], ms->dim, polys, (hipStream_t)stream);
  };
  return gemv_call(c, GemvCall{"gpq_he_gemv_multi", ms->plans.data(), ms->count, &ms->baby, ms->dim, kGemvMultiNP}, inner_sums, out_c0, out_c1, c0, c1, rk0, rk1,
                   W, logDelta, dimB, dimP, batch, workspace, stream);
}
