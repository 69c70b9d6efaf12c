// shim_decrypt.hpp -- he_dec and gpq_shim_he_dec_dcd of the MPI-typed surface: one body, two tails.  Part of mpi_shim.hip's translation unit
// (included inside its extern "C" block, after the staging, key and polynomial fragments).
#pragma once

// src/he-encrypt.c:105-125: m = c1 * sk + c0, centred mod q_l.  The reference multiplies through poly_mul and then adds and centres with
// 2n libgcrypt calls on the host; here the product never leaves the device before the sum is centred, and a chained ciphertext (and the
// secret key after its first use) is resident.
// One body for he_dec and gpq_shim_he_dec_dcd: operands, residency and the recheck are the same; only the tail differs.  pt != NULL: the
// plaintext comes down and becomes libgcrypt integers (he_dec).  z != NULL: he_dcd runs on the device result (gpq_he_dcd, the host's
// polyctx.ring.zetas as roots, nu = ct->nu) and 16 * hectx.slots bytes come down; returns false, with z untouched, when that path does not apply.
} // extern "C"
namespace {
bool dec_body(struct he_pt *pt, _Complex double *z, const struct he_ct *ct, const poly_mpi_t *sk) {
  need_hectx();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, l = ct->l;
  const std::vector<uint64_t> qw = words_of(hectx.q[l], "he_dec: q_l must be positive");
  const bool pow2 = is_pow2(qw);
  const unsigned nbq = G.mpi_get_nbits(hectx.q[l]), logql = nbq - 1, dim = nbq / 59 + 1;        // :113
  const poly_mpi_t *in[3] = {&ct->c1, sk, &ct->c0};
  poly_mpi_t *out[1] = {pt ? &pt->m : nullptr};
  const unsigned slots = hectx.slots;
  gpq_ecd_plan *dplan = nullptr;
  if (z) {
    if (!pow2 || logql == 0 || !polyctx.ring.zetas || !slots || (slots & (slots - 1)) || slots > n / 2 || slots > GPQ_ECD_MAX_SLOTS || !(ct->nu > 0) || !std::isfinite(ct->nu))
      return false;
    if (!g_dcd_plan.plan || g_dcd_plan.slots != slots || g_dcd_plan.m != polyctx.m || g_dcd_plan.zetas != (const void *)polyctx.ring.zetas) {
      if (g_dcd_plan.plan) { (void)gpq_stream_sync(nullptr); gpq_ecd_plan_destroy(g_dcd_plan.plan); g_dcd_plan = DcdPlan(); }
      if (gpq_ecd_plan_create_split(c, &g_dcd_plan.plan, slots, 0, (const double *)polyctx.ring.zetas, polyctx.m / 4) != GPQ_OK) die("he_dec_dcd: cannot build the decoder's tables");
      g_dcd_plan.slots = slots; g_dcd_plan.m = polyctx.m; g_dcd_plan.zetas = (const void *)polyctx.ring.zetas;
    }
    dplan = g_dcd_plan.plan;
  } else {
    pt->nu = ct->nu;                                                                             // :108
    if (logql == 0) { fill_minus_one(&pt->m, n); return true; }   // q_l = 1
  }
  const unsigned Wout = logql / 64 + 1;
  const size_t zbytes = (size_t)slots * 16;
  auto pass = [&](unsigned W, bool kept) -> bool {
    if (W > 32) die("he_dec: coefficients wider than 2047 bits");
    const size_t big = (size_t)W * n;
    DevBuf dz(big * 8), ws(gpq_poly_mul_general_workspace_bytes(c, dim, 1)), scratch(192 * 8);
    std::unique_ptr<DevBuf> dm, dzs;                          // z: the plaintext stays in a slab of the call's own, the doubles come down
    std::unique_ptr<HostBuf> hz;
    if (z) { dm.reset(new DevBuf(big * 8)); dzs.reset(new DevBuf(zbytes)); hz.reset(new HostBuf(zbytes)); }
    StagedCall call(n, W, 3, in, z ? 0 : 1);
    call.speculate = kept; call.report_misfits = true; call.Wdown = Wout < W ? Wout : W;
    const StagedCall::Verdict v = call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
      uint64_t *const dr = z ? dm->u64() : o[0];
      int rc = pow2 ? gpq_poly_mul(c, dr, x[0], x[1], W, dim, logql, 1, ws.p, nullptr)                                                 // :115
                    : gpq_poly_mul_general(c, dr, x[0], x[1], W, dim, qw.data(), (unsigned)qw.size(), 1, ws.p, nullptr);
      if (rc == GPQ_OK) rc = gpq_big_addsub(c, dr, dr, x[2], W, 1, 0, nullptr);                                                       // :117
      if (rc == GPQ_OK && hipMemsetAsync(dz.p, 0, big * 8, nullptr) != hipSuccess) die("device memset failed");                       // the centring kernels take a pair
      if (rc == GPQ_OK)                                                                                                                // :118
        rc = pow2 ? gpq_he_rs(c, dr, dz.u64(), W, 0, logql, 1, nullptr)
                  : gpq_he_rs_general(c, dr, dz.u64(), W, 1ull, qw.data(), (unsigned)qw.size(), 1, scratch.p, nullptr);
      if (rc != GPQ_OK) die("he_dec failed");
      if (!z) return;
      // the centred plaintext (sign-extended over all W words) is decoded where it lies
      if (gpq_he_dcd(c, dplan, (double *)dzs->p, dr, ct->nu, W, 1, nullptr) != GPQ_OK) die("he_dec_dcd: gpq_he_dcd failed");
      if (gpq_download(hz->p, dzs->p, zbytes, nullptr) != GPQ_OK) die("download failed");
    });
    if (v != StagedCall::Done) return false;
    if (!z) { call.deliver(out); return true; }
    if (call.sync() != GPQ_OK) die("he_dec_dcd: the device work failed");
    memcpy(z, hz->p, zbytes);
    return true;
  };
  width_ladder(in, 3, n, pow2, Wout, nbq, 1, pass);
  return true;
}
}  // namespace
extern "C" {

void he_dec(struct he_pt *pt, const struct he_ct *ct, const poly_mpi_t *sk) {
  SHIM_CALL();
  (void)dec_body(pt, nullptr, ct, sk);
}

// he_dec followed by he_dcd with the plaintext staying on the device (include/gpqhe_hip_compat.h)
int gpq_shim_he_dec_dcd(_Complex double *m, const struct he_ct *ct, const poly_mpi_t *sk) {
  SHIM_CALL();
  if (!m || !ct || !sk) die("gpq_shim_he_dec_dcd: null argument");
  return dec_body(nullptr, m, ct, sk) ? 1 : 0;
}
