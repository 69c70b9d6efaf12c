// gemv_plan.hpp -- he_gemv for a fixed matrix (include/gpqhe_hip.h, "he_gemv with a plan"): the plan object, one giant step's inner sum in
// the NTT domain (gpq_gemv_inner), the driver of a whole call over a list of plans (gemv_call) and the call with one plan
// (gpq_he_gemv_planned); gemv_multi.hpp runs the same driver with a set's plans.  Part of bridge.hip's translation unit (it uses that file's
// gemv_steps, gemv_add_giant, gemv_close and align64, and bridge_launch.hpp's launch_decompose, check and ranges_overlap); the kernel is
// gemv_mac in ntt_kernels.hpp, launched by engine.hip's gpq_gemv_mac.
//
// The inner sum is exact, not approximate: see the header for the identity, the bound behind gpq_gemv_acc_dim and the guard.  What runs per
// call: the live baby rotations as ONE gpq_he_rot_hoisted, their rns_decompose + complete forward transform over `dim` limbs once, and per
// live giant step and plan the inner sum (the entry point's launcher: gemv_mac here, gemv_mac_multi for a set) -> gpq_invntt ->
// gpq_rns_reconstruct (centred mod 2^logql) -> he_rot by i n1 -> wrapping sum.  The inverse low stages are NOT fused into the inner sum and
// its c1 goes to the giant rotation as words (reconstruct + decompose), not through bridge_crt_decompose: DESIGN.md says what that leaves
// on the table.
#pragma once

struct gpq_gemv_plan {
  gpq_ctx *ctx = nullptr;
  unsigned slots = 0, n1 = 0, n2 = 0, logql = 0, dimpt = 0, dim = 0, diag_bits = 0, live = 0;
  int exact = 0;
  gpq_dev<uint64_t> d_hat;              // [slots][dim][n], NTT domain, words in [0, p]
  size_t bytes = 0;
  // (rotation slot, diagonal) of the live terms of giant step i at [i * n1 ...): slot = j for gpq_gemv_inner (`full`), slot = the rank of j
  // among the live baby rotations for gpq_he_gemv_planned (`packed`)
  gpq_dev<uint2> d_full, d_packed;
  std::vector<unsigned> nterms;         // per giant step
  std::vector<unsigned> baby;           // live baby rotations, ascending
  std::vector<unsigned char> live_diag; // per diagonal
};

namespace {
unsigned ceil_log2(unsigned v) { unsigned b = 0; while ((1ull << b) < v) ++b; return b; }

int plan_usable(const gpq_ctx *c, const gpq_gemv_plan *p, const char *who) {
  if (!p) return gpq_fail(GPQ_ERR_INVALID, "%s: null plan", who);
  if (p->ctx != c) return gpq_fail(GPQ_ERR_INVALID, "%s: the plan belongs to another context", who);
  if (!p->exact)
    return gpq_fail(GPQ_ERR_INVALID, "%s: the plan is not exact (diagonals of %u bits at q = 2^%u: one product can wrap the %u-limb basis of he_mulpt, or %u limbs exceed the context's %u): use gpq_he_gemv",
                    who, p->diag_bits, p->logql, p->dimpt, p->dim, c->nprimes);
  return GPQ_OK;
}

// acc -> words: inverse transform of both sums (acc0 | acc1 contiguous), then one reconstruction per polynomial of the ciphertext
int inner_finish(gpq_ctx *c, const gpq_gemv_plan *p, uint64_t *out0, uint64_t *out1, uint64_t *acc, unsigned W, unsigned polys, void *stream) {
  const size_t slab = (size_t)polys * p->dim * c->n;
  int rc;
  if ((rc = gpq_invntt(c, acc, p->dim, 2 * polys, stream))) return rc;
  if ((rc = gpq_rns_reconstruct(c, out0, W, acc, p->dim, polys, p->logql, stream))) return rc;
  return gpq_rns_reconstruct(c, out1, W, acc + slab, p->dim, polys, p->logql, stream);
}
}  // namespace

extern "C" unsigned gpq_gemv_acc_dim(unsigned logql, unsigned diag_bits, unsigned logn, unsigned n1) {
  const unsigned long long need = (unsigned long long)logql - (logql ? 1 : 0) + diag_bits + logn + ceil_log2(n1 ? n1 : 1) + 1;   // L + 1 <= 59 d
  const unsigned long long d = (need + 58) / 59;
  return d ? (unsigned)d : 1u;
}

extern "C" void gpq_gemv_plan_destroy(gpq_gemv_plan *p) {
  if (!p) return;
  DeviceScope on_device(p->ctx->device);
  delete p;
}

extern "C" int gpq_gemv_plan_info(const gpq_gemv_plan *p, unsigned *dim, size_t *bytes, unsigned *live, int *exact) {
  if (!p) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_info: null plan");
  if (dim) *dim = p->dim;
  if (bytes) *bytes = p->bytes;
  if (live) *live = p->live;
  if (exact) *exact = p->exact;
  return GPQ_OK;
}

extern "C" unsigned gpq_gemv_plan_diag_bits(const gpq_gemv_plan *p) { return p ? p->diag_bits : 0; }

extern "C" int gpq_gemv_plan_rotations(const gpq_gemv_plan *p, unsigned char *needed) {
  if (!p || !needed) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_rotations: null argument");
  memset(needed, 0, p->slots);
  for (unsigned j : p->baby) needed[j] = 1;
  for (unsigned i = 0; i < p->n2; ++i) if (p->nterms[i]) needed[i * p->n1] = 1;
  return GPQ_OK;
}

extern "C" int gpq_gemv_plan_create(gpq_ctx *c, gpq_gemv_plan **out, const uint64_t *diag, unsigned slots, unsigned W, unsigned logql,
                                    unsigned dimpt, void *stream) {
  int rc = check(c, dimpt, slots, "gpq_gemv_plan_create");
  if (rc) return rc;
  if (!out || !diag || !logql || W < 1 || W > 32) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_create: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (gpq_capturing(s))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_create allocates and waits for the stream: not inside a stream capture");
  std::unique_ptr<gpq_gemv_plan, void (*)(gpq_gemv_plan *)> p(new (std::nothrow) gpq_gemv_plan(), gpq_gemv_plan_destroy);
  if (!p) return gpq_fail(GPQ_ERR_NOMEM, "out of host memory");
  p->ctx = c; p->slots = slots; p->logql = logql; p->dimpt = dimpt;
  gemv_steps(slots, &p->n1, &p->n2);
  // the largest coefficient of every diagonal, on the device
  std::vector<unsigned> bits(slots, 0);
  {
    gpq_dev<unsigned> d_bits;
    HIP_TRY(d_bits.alloc(slots * sizeof(unsigned)));
    hipError_t e = hipMemsetAsync(d_bits, 0, slots * sizeof(unsigned), s);
    for (unsigned k0 = 0; k0 < slots && e == hipSuccess; k0 += 65535) {
      const unsigned cnt = slots - k0 < 65535 ? slots - k0 : 65535u;
      MagnitudeArgs m{diag + (size_t)k0 * W * c->n, d_bits + k0, W, c->logn};
      hipLaunchKernelGGL(bridge_magnitude_bits, dim3((c->n + 255) / 256, cnt), dim3(256), 0, s, m);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bits.data(), d_bits, slots * sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "gpq_gemv_plan_create: measuring the diagonals: %s", hipGetErrorString(e));
  }
  p->live_diag.resize(slots);
  for (unsigned k = 0; k < slots; ++k) {
    p->live_diag[k] = bits[k] != 0;
    p->live += bits[k] != 0;
    if (bits[k] > p->diag_bits) p->diag_bits = bits[k];
  }
  const unsigned acc = gpq_gemv_acc_dim(logql, p->diag_bits, c->logn, p->n1);
  p->dim = acc > dimpt ? acc : dimpt;
  const bool product_exact = (unsigned long long)logql - 1 + p->diag_bits + c->logn + 1 <= 59ull * dimpt;
  p->exact = product_exact && p->dim <= c->nprimes;
  // the live terms of every giant step
  std::vector<unsigned> rank(p->n1, 0);
  for (unsigned j = 0; j < p->n1; ++j) {
    bool any = false;
    for (unsigned i = 0; i < p->n2; ++i) any = any || p->live_diag[i * p->n1 + j];
    if (any) { rank[j] = (unsigned)p->baby.size(); p->baby.push_back(j); }
  }
  std::vector<uint2> full((size_t)p->n1 * p->n2), packed(full.size());
  p->nterms.assign(p->n2, 0);
  for (unsigned i = 0; i < p->n2; ++i)
    for (unsigned j = 0; j < p->n1; ++j)
      if (p->live_diag[i * p->n1 + j]) {
        const size_t t = (size_t)i * p->n1 + p->nterms[i]++;
        full[t] = make_uint2(j, i * p->n1 + j);
        packed[t] = make_uint2(rank[j], i * p->n1 + j);
      }
  if (!p->exact) { *out = p.release(); return GPQ_OK; }            // holds nothing: the entry points refuse it
  DeviceScope on_device(c->device);
  HIP_TRY(p->d_full.alloc(full.size() * sizeof(uint2)));
  HIP_TRY(p->d_packed.alloc(full.size() * sizeof(uint2)));
  HIP_TRY(hipMemcpy(p->d_full, full.data(), full.size() * sizeof(uint2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_packed, packed.data(), full.size() * sizeof(uint2), hipMemcpyHostToDevice));
  const size_t poly = (size_t)p->dim * c->n;
  p->bytes = (size_t)slots * poly * 8;
  if (p->d_hat.alloc(p->bytes) != hipSuccess) {
    (void)hipGetLastError();
    return gpq_fail(GPQ_ERR_NOMEM, "gpq_gemv_plan_create: no room for %zu bytes of transformed diagonals", p->bytes);
  }
  {
    StageRange stage("gpq_gemv_plan_create: rns_decompose + forward transform of the diagonals");
    for (unsigned k0 = 0; k0 < slots; k0 += c->set.chunk) {               // (zero diagonals too: their words are never read, but stay defined)
      const unsigned cnt = gpq_group_size(c, slots - k0);
      if ((rc = launch_decompose(c, p->d_hat + k0 * poly, diag + (size_t)k0 * W * c->n, W, 0, p->dim, cnt, s))) return rc;
      if ((rc = gpq_hoist_forward(c, p->d_hat + k0 * poly, p->dim, cnt, s))) return rc;
    }
  }
  if ((rc = launched("gpq_gemv_plan_create"))) return rc;
  *out = p.release();
  return GPQ_OK;
}

extern "C" size_t gpq_gemv_inner_workspace_bytes(gpq_ctx *c, const gpq_gemv_plan *p, unsigned batch) {
  if (!c || !p || !batch) return 0;
  const unsigned m = gpq_group_size(c, batch);
  const size_t slab = (size_t)m * p->dim * c->n * 8;
  return align64(2 * p->n1 * slab) + align64(2 * slab);
}

extern "C" int gpq_gemv_inner(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *R0, const uint64_t *R1, const gpq_gemv_plan *p,
                              unsigned giant, unsigned W, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, 1, batch, "gpq_gemv_inner");
  if (rc || (rc = plan_usable(c, p, "gpq_gemv_inner"))) return rc;
  if (!out_c0 || !out_c1 || !R0 || !R1 || !workspace || giant >= p->n2 || W < (p->logql + 63) / 64 || W > 32)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_inner: bad arguments (giant step < %u, W words must hold q = 2^%u)", p->n2, p->logql);
  const size_t n = c->n, bigpoly = (size_t)W * n, out_words = batch * bigpoly, in_words = p->n1 * out_words;
  if (ranges_overlap(out_c0, out_words, out_c1, out_words) || ranges_overlap(out_c0, out_words, R0, in_words) || ranges_overlap(out_c0, out_words, R1, in_words) ||
      ranges_overlap(out_c1, out_words, R0, in_words) || ranges_overlap(out_c1, out_words, R1, in_words))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_inner: the outputs alias each other or an input");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nterms = p->nterms[giant];
  if (!nterms) {                                                        // every diagonal of the step is zero: an exact zero
    HIP_TRY(hipMemsetAsync(out_c0, 0, out_words * 8, s));
    HIP_TRY(hipMemsetAsync(out_c1, 0, out_words * 8, s));
    return GPQ_OK;
  }
  const unsigned m = gpq_group_size(c, batch);
  const size_t group_slab = (size_t)m * p->dim * n;
  uint64_t *hat = (uint64_t *)workspace, *acc = (uint64_t *)((char *)workspace + align64(2 * p->n1 * group_slab * 8));
  for (unsigned k0 = 0; k0 < batch; k0 += m) {
    const unsigned polys = batch - k0 < m ? batch - k0 : m;
    const size_t slab = (size_t)polys * p->dim * n;
    uint64_t *hat0 = hat, *hat1 = hat + p->n1 * slab;
    {
      StageRange stage("gpq_gemv_inner: rns_decompose + forward transform of the rotations");
      for (unsigned j = 0; j < p->n1; ++j) {
        const size_t src = ((size_t)j * batch + k0) * bigpoly;
        if (!p->live_diag[giant * p->n1 + j]) {                       // not read by gemv_mac; keeps the transform below on defined words
          HIP_TRY(hipMemsetAsync(hat0 + j * slab, 0, slab * 8, s));
          HIP_TRY(hipMemsetAsync(hat1 + j * slab, 0, slab * 8, s));
          continue;
        }
        if ((rc = launch_decompose(c, hat0 + j * slab, R0 + src, W, 0, p->dim, polys, s))) return rc;
        if ((rc = launch_decompose(c, hat1 + j * slab, R1 + src, W, 0, p->dim, polys, s))) return rc;
      }
      if ((rc = gpq_hoist_forward(c, hat, p->dim, 2 * p->n1 * polys, s))) return rc;
    }
    if ((rc = gpq_gemv_mac(c, acc, acc + slab, hat0, hat1, p->d_hat, p->d_full + (size_t)giant * p->n1, nterms, p->dim, polys, s))) return rc;
    if ((rc = inner_finish(c, p, out_c0 + k0 * bigpoly, out_c1 + k0 * bigpoly, acc, W, polys, stream))) return rc;
  }
  return launched("gpq_gemv_inner");
}

// ---------------------------------------------------------------------------
// The he_gemv call over a list of plans on the same ciphertexts: ONE plan for gpq_he_gemv_planned, a set's for gpq_he_gemv_multi
// (gemv_multi.hpp).  What depends on the ciphertext alone -- the hoisted baby rotations, their rns_decompose + forward transform -- runs
// once per launch group over the plans' live baby rotations and `dim` limbs; everything behind the inner sums runs per plan.  An entry
// point supplies only how one giant step's inner sums are launched.
// ---------------------------------------------------------------------------
namespace {
struct GemvCall {
  const char *who;                        // the entry point, for messages
  const gpq_gemv_plan *const *plans;      // usable, same slots and logql
  unsigned count;
  const std::vector<unsigned> *baby;      // the live baby rotations of all of them, ascending
  unsigned dim;                           // limbs of the transformed rotations: the largest among the plans
  unsigned nacc;                          // plans per launch of inner sums
};

// Workspace of one launch group of m ciphertexts, in this order
struct GemvCallLayout { size_t rb, hat, acc, p, g, ws, total; };
int gemv_call_layout(gpq_ctx *c, size_t nb, unsigned dim, unsigned nacc, unsigned W, unsigned dimB, unsigned dimP, unsigned m, GemvCallLayout *l) {
  const size_t big = (size_t)m * W * c->n * 8, slab = (size_t)m * dim * c->n * 8;
  l->rb = 2 * align64(nb * big);                       // the live baby rotations, c0 | c1
  l->hat = align64(2 * nb * slab);                     // ... decomposed and transformed
  l->acc = align64(2 * slab);                          // one giant step's sums of one plan: ONE of nacc regions
  l->p = 2 * align64(big);                             // ... as words
  l->g = 2 * align64(big);                             // one giant rotation
  const size_t wn = nb ? gpq_he_rot_hoisted_workspace_bytes(c, W, dimB, dimP, (unsigned)nb, m) : 0, w1 = gpq_he_rot_hoisted_workspace_bytes(c, W, dimB, dimP, 1, m);
  if ((nb && !wn) || !w1) return GPQ_ERR_INVALID;      // (the rotation plan's message is in gpq_last_error)
  l->ws = align64(wn > w1 ? wn : w1);
  l->total = l->rb + l->hat + nacc * l->acc + l->p + l->g + l->ws;
  return GPQ_OK;
}
struct GemvCallSlabs { uint64_t *RB0, *RB1, *hat; char *acc; uint64_t *P0, *P1, *G0, *G1; void *ws; };
GemvCallSlabs gemv_call_carve(const GemvCallLayout &l, unsigned nacc, void *workspace) {
  GemvCallSlabs b;
  char *w = (char *)workspace;
  b.RB0 = (uint64_t *)w; b.RB1 = (uint64_t *)(w + l.rb / 2); w += l.rb;
  b.hat = (uint64_t *)w; w += l.hat;
  b.acc = w; w += nacc * l.acc;
  b.P0 = (uint64_t *)w; b.P1 = (uint64_t *)(w + l.p / 2); w += l.p;
  b.G0 = (uint64_t *)w; b.G1 = (uint64_t *)(w + l.g / 2); w += l.g;
  b.ws = w;
  return b;
}
size_t gemv_call_workspace_bytes(gpq_ctx *c, size_t nb, unsigned dim, unsigned nacc, unsigned W, unsigned dimB, unsigned dimP, unsigned batch) {
  GemvCallLayout l;
  return gemv_call_layout(c, nb, dim, nacc, W, dimB, dimP, gpq_group_size(c, batch), &l) == GPQ_OK ? l.total : 0;
}

// inner_sums(i, first, polys, hat0, hat1, acc) launches giant step i's inner sums of plans first .. first + nacc - 1 on `polys` ciphertexts:
// acc[t] is NULL when plan first + t is past the list or has no live term in the step, else its sums go to acc[t] (c0) and
// acc[t] + polys * dim_t * n (c1) over the plan's own dim_t limbs.  Called only when some acc[t] is not NULL.
template <class InnerSums>
int gemv_call(gpq_ctx *c, const GemvCall &g, InnerSums &&inner_sums, uint64_t *const *out_c0, uint64_t *const *out_c1, const uint64_t *c0, const uint64_t *c1,
              const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logDelta, unsigned dimB, unsigned dimP, unsigned batch,
              void *workspace, void *stream) {
  const unsigned logql = g.plans[0]->logql, n1 = g.plans[0]->n1, n2 = g.plans[0]->n2, count = g.count, nacc = g.nacc, nb = (unsigned)g.baby->size();
  if (!out_c0 || !out_c1 || !c0 || !c1 || !rk0 || !rk1 || !workspace || logDelta >= logql || W < (logql + 63) / 64 || W > 32)
    return gpq_fail(GPQ_ERR_INVALID, "%s: bad arguments (W words must hold q = 2^%u, Delta below q)", g.who, logql);
  const size_t n = c->n, bigpoly = (size_t)W * n, words = batch * bigpoly;
  std::vector<const uint64_t *> slabs{c0, c1};                            // the inputs, then every output: no two may overlap
  for (unsigned t = 0; t < count; ++t) {
    if (!out_c0[t] || !out_c1[t]) return gpq_fail(GPQ_ERR_INVALID, "%s: output %u is NULL", g.who, t);
    slabs.push_back(out_c0[t]); slabs.push_back(out_c1[t]);
  }
  for (size_t a = 2; a < slabs.size(); ++a)
    for (size_t b = 0; b < a; ++b)
      if (ranges_overlap(slabs[a], words, slabs[b], words)) return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs alias each other or an input", g.who);
  std::vector<const uint64_t *> bk0(nb), bk1(nb);
  for (unsigned r = 0; r < nb; ++r) {
    const unsigned j = (*g.baby)[r];
    bk0[r] = rk0[j]; bk1[r] = rk1[j];
    if (!bk0[r] || !bk1[r]) return gpq_fail(GPQ_ERR_INVALID, "%s: key %u is NULL (a live baby rotation)", g.who, j);
  }
  for (unsigned t = 0; t < count; ++t)
    for (unsigned i = 0; i < n2; ++i)
      if (g.plans[t]->nterms[i] && (!rk0[i * n1] || !rk1[i * n1])) return gpq_fail(GPQ_ERR_INVALID, "%s: key %u is NULL (a live giant rotation)", g.who, i * n1);
  hipStream_t s = (hipStream_t)stream;
  const unsigned m = gpq_group_size(c, batch);
  GemvCallLayout l;
  if (gemv_call_layout(c, nb, g.dim, nacc, W, dimB, dimP, m, &l)) return gpq_fail(GPQ_ERR_INVALID, "%s: unsupported shape", g.who);
  const GemvCallSlabs b = gemv_call_carve(l, nacc, workspace);
  std::vector<unsigned char> first(count);
  std::vector<uint64_t *> acc(nacc);
  int rc;
  for (unsigned k0 = 0; k0 < batch; k0 += m) {
    const unsigned polys = batch - k0 < m ? batch - k0 : m;
    const size_t o = k0 * bigpoly, slab = (size_t)polys * g.dim * n;
    for (unsigned t = 0; t < count; ++t)
      if (g.plans[t]->baby.empty()) {                                      // the zero matrix
        HIP_TRY(hipMemsetAsync(out_c0[t] + o, 0, polys * bigpoly * 8, s));
        HIP_TRY(hipMemsetAsync(out_c1[t] + o, 0, polys * bigpoly * 8, s));
      }
    if (!nb) continue;
    uint64_t *hat0 = b.hat, *hat1 = b.hat + nb * slab;
    if ((rc = gpq_he_rot_hoisted(c, b.RB0, b.RB1, c0 + o, c1 + o, g.baby->data(), bk0.data(), bk1.data(), nb, W, logql, dimB, dimP, polys, b.ws, stream))) return rc;   // src/he-algo.c:63-68
    {
      StageRange stage("he_gemv: rns_decompose + forward transform of the baby rotations (once per group, for every plan)");
      if ((rc = launch_decompose(c, hat0, b.RB0, W, 0, g.dim, nb * polys, s))) return rc;
      if ((rc = launch_decompose(c, hat1, b.RB1, W, 0, g.dim, nb * polys, s))) return rc;
      if ((rc = gpq_hoist_forward(c, b.hat, g.dim, 2 * nb * polys, s))) return rc;
    }
    std::fill(first.begin(), first.end(), 1);
    for (unsigned i = 0; i < n2; ++i)
      for (unsigned t0 = 0; t0 < count; t0 += nacc) {
        bool any = false;
        for (unsigned t = 0; t < nacc; ++t) {
          const bool live = t0 + t < count && g.plans[t0 + t]->nterms[i];
          acc[t] = live ? (uint64_t *)(b.acc + t * l.acc) : nullptr;
          any = any || live;
        }
        if (!any) continue;                                                // he_swk of an exact zero is zero
        StageRange stage("he_gemv: one giant step of one launch of inner sums (the sums, then per plan the rotation)");
        if ((rc = inner_sums(i, t0, polys, hat0, hat1, acc.data()))) return rc;                                              // :70-78
        for (unsigned t = 0; t < nacc; ++t) {
          if (!acc[t]) continue;
          const unsigned pl = t0 + t;
          if ((rc = inner_finish(c, g.plans[pl], b.P0, b.P1, acc[t], W, polys, stream))) return rc;
          if ((rc = gemv_add_giant(c, out_c0[pl] + o, out_c1[pl] + o, b.P0, b.P1, b.G0, b.G1, first[pl], i * n1, rk0, rk1, W, logql, dimB, dimP, polys, b.ws, stream))) return rc;
          first[pl] = 0;
        }
      }
  }
  for (unsigned t = 0; t < count; ++t)
    if ((rc = gemv_close(c, out_c0[t], out_c1[t], W, logDelta, logql, batch, stream))) return rc;
  return launched(g.who);
}
}  // namespace

extern "C" size_t gpq_he_gemv_planned_workspace_bytes(gpq_ctx *c, const gpq_gemv_plan *p, unsigned W, unsigned dimB, unsigned dimP, unsigned batch) {
  if (!c || !p || !batch || !W) return 0;
  return gemv_call_workspace_bytes(c, p->baby.size(), p->dim, 1, W, dimB, dimP, batch);
}

extern "C" int gpq_he_gemv_planned(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const gpq_gemv_plan *p,
                                   const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logDelta, unsigned dimB,
                                   unsigned dimP, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_he_gemv_planned");
  if (rc || (rc = plan_usable(c, p, "gpq_he_gemv_planned"))) return rc;
  auto inner_sums = [&](unsigned i, unsigned, unsigned polys, const uint64_t *hat0, const uint64_t *hat1, uint64_t *const *acc) {
    return gpq_gemv_mac(c, acc[0], acc[0] + (size_t)polys * p->dim * c->n, hat0, hat1, p->d_hat, p->d_packed + (size_t)i * p->n1, p->nterms[i], p->dim, polys,
                        (hipStream_t)stream);
  };
  return gemv_call(c, GemvCall{"gpq_he_gemv_planned", &p, 1, &p->baby, p->dim, 1}, inner_sums, &out_c0, &out_c1, c0, c1, rk0, rk1, W, logDelta, dimB, dimP, batch,
                   workspace, stream);
}
