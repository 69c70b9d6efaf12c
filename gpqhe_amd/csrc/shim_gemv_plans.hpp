// shim_gemv_plans.hpp -- the plan cache of he_gemv / he_sum / he_idx (shim_algo.hpp).  The reference's users of he_gemv apply a FIXED matrix
// again and again (he_sum, he_idx, he_nrm2, the linear maps of bootstrapping); a hit costs no he_ecd, no conversion and no upload of
// diagonals, and the call runs gpq_he_gemv_planned on the plan's transformed diagonals.  Keyed by everything the encoded diagonals depend
// on -- ring, slots, level and its modulus, Delta -- and an EXACT copy of the slots^2 matrix entries compared with memcmp (he_sum / he_idx:
// the kind and idx; no matrix is built).  Least recently used out; the plans belong to the engine context and are released before it.
#pragma once

namespace {

struct GemvPlanKey {
  unsigned kind = 0, idx = 0, n = 0, slots = 0, l = 0, logql = 0;   // kind 0: he_gemv (A), 1: he_sum, 2: he_idx (idx)
  double Delta = 0;
  std::vector<unsigned char> A;
  bool operator==(const GemvPlanKey &o) const {
    return kind == o.kind && idx == o.idx && n == o.n && slots == o.slots && l == o.l && logql == o.logql && !memcmp(&Delta, &o.Delta, sizeof Delta) &&
           A.size() == o.A.size() && (A.empty() || !memcmp(A.data(), o.A.data(), A.size()));
  }
};
struct GemvPlanEntry {
  GemvPlanKey key;
  gpq_gemv_plan *plan = nullptr;
  double nu = 0;                 // pt.nu of every diagonal (they agree, or the call takes the loop)
  unsigned bits = 0;             // what sized the big slabs of the call that made the plan: W = bits / 64 + 1
  unsigned long long used = 0;
};
std::vector<GemvPlanEntry> g_gemv_plans;
unsigned g_gemv_plan_slots = 4;
bool g_device_ecd = false;      // gpq_mpi_shim_set_device_ecd: a missing plan is built from the matrix on the device (shim_algo.hpp)
unsigned long long g_gemv_plan_tick = 0;

// gpq_shim_he_dec_dcd's decoder tables (a gpq_ecd_plan on the host's polyctx.ring.zetas), kept between calls; they belong to the engine
// context like the plans above and go with them
struct DcdPlan { gpq_ecd_plan *plan = nullptr; unsigned slots = 0, m = 0; const void *zetas = nullptr; } g_dcd_plan;

void gemv_plans_drop(size_t keep) {        // least recently used first
  if (!keep && g_dcd_plan.plan) {
    (void)gpq_stream_sync(nullptr);
    gpq_ecd_plan_destroy(g_dcd_plan.plan);
    g_dcd_plan = DcdPlan();
  }
  while (g_gemv_plans.size() > keep) {
    size_t old = 0;
    for (size_t i = 1; i < g_gemv_plans.size(); ++i) if (g_gemv_plans[i].used < g_gemv_plans[old].used) old = i;
    (void)gpq_stream_sync(nullptr);        // a call that used the plan may still be running
    gpq_gemv_plan_destroy(g_gemv_plans[old].plan);
    g_gemv_plans.erase(g_gemv_plans.begin() + (long)old);
  }
}
GemvPlanEntry *gemv_plan_find(const GemvPlanKey &k) {
  for (GemvPlanEntry &e : g_gemv_plans) if (e.key == k) { e.used = ++g_gemv_plan_tick; return &e; }
  return nullptr;
}
GemvPlanEntry *gemv_plan_insert(GemvPlanEntry e) {
  if (!g_gemv_plan_slots) return nullptr;
  gemv_plans_drop(g_gemv_plan_slots - 1);
  e.used = ++g_gemv_plan_tick;
  g_gemv_plans.push_back(std::move(e));
  return &g_gemv_plans.back();
}

}  // namespace
