// shim_encrypt.hpp -- he_enc_pk / he_enc_sk (src/he-encrypt.c:37-103) and he_keypair (src/he-kem.c:43-71) of the MPI-typed surface: one body.
// Part of mpi_shim.hip's translation unit (included inside its extern "C" block, after shim_decrypt.hpp).
#pragma once

// The randomness is the host program's.  Default: its own sample_zo / sample_error / sample_uniform / sample_sk (src/sample.c, weak
// references) are called in the reference's order and their polynomials converted once.  gpq_mpi_shim_set_device_samplers(1): the host's
// randombytes (weak) is called once per sampler call with the reference's byte counts -- n/4 (zo), n (error), n (nbits/8 + 1) (uniform) --
// and gpq_sample_zo / gpq_sample_error / gpq_sample_uniform expand the bytes on the device; sample_sk stays the host's.  Power-of-two q_L
// takes gpq_he_enc_pk / gpq_he_enc_sk; any other q_L the reference's sequence over the general entry points.  The key polynomials and the
// plaintext are resident operands like he_dec's, the written ciphertext / public key is remembered (one StagedCall, shim_call.hpp).
// gpq_mpi_shim_set_device_rng(1) on top of the device samplers: the same byte counts in the same order are reserved from the default stream
// of gpq_randombytes and generated in device memory by ONE gpq_randombytes_device per call; the samplers read slices of that buffer.
} // extern "C"
namespace {
bool g_device_samplers = false, g_device_rng = false;

struct TmpPoly {                                            // a polynomial for the host's samplers to fill
  poly_mpi_t p; unsigned n;
  explicit TmpPoly(unsigned n_) : n(n_) { p.coeffs = (gpq_MPI *)malloc(n * sizeof(gpq_MPI)); for (unsigned i = 0; i < n; ++i) p.coeffs[i] = G.mpi_new(0); }
  ~TmpPoly() { for (unsigned i = 0; i < n; ++i) G.mpi_release(p.coeffs[i]); free(p.coeffs); }
  TmpPoly(const TmpPoly &) = delete;
  TmpPoly &operator=(const TmpPoly &) = delete;
};
void forget_poly(const poly_mpi_t *p) {
  for (size_t i = 0; i < g_polys.size(); ++i) if (g_polys[i].coeffs == p->coeffs) { drop_poly_slot(i); return; }
}
// one small polynomial (zo: kind 0, error: kind 1) as an int8 small slab on the device
// (`drawn`: the bytes are already on the device, a slice of the call's gpq_randombytes_device)
void sample_small(gpq_ctx *c, const DevBuf &dst, int kind, unsigned n, bool device, const uint8_t *drawn = nullptr) {
  if (drawn) {
    const int rc = kind ? gpq_sample_error(c, (int8_t *)dst.p, drawn, 1, nullptr) : gpq_sample_zo(c, (int8_t *)dst.p, drawn, 1, nullptr);
    if (rc != GPQ_OK) die("he_enc: the device sampler failed");
    return;
  }
  if (device) {
    const size_t nbytes = kind ? n : n / 4;
    std::vector<uint8_t> h(nbytes);
    randombytes(h.data(), nbytes);
    DevBuf bytes(nbytes);
    if (gpq_upload(bytes.p, h.data(), nbytes, nullptr) != GPQ_OK || gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");   // (h goes out of scope)
    const int rc = kind ? gpq_sample_error(c, (int8_t *)dst.p, (const uint8_t *)bytes.p, 1, nullptr) : gpq_sample_zo(c, (int8_t *)dst.p, (const uint8_t *)bytes.p, 1, nullptr);
    if (rc != GPQ_OK) die("he_enc: the device sampler failed");
    return;
  }
  TmpPoly t(n);
  if (kind) sample_error(&t.p); else sample_zo(&t.p);
  if (max_bits(&t.p, n) > 7) die("he_enc: the host's sample_zo / sample_error gave a coefficient outside [-127, 127]");
  std::vector<uint64_t> w(n);
  to_slab(w.data(), &t.p, n, 1);
  std::vector<int8_t> h(n);
  for (unsigned i = 0; i < n; ++i) h[i] = (int8_t)(int64_t)w[i];
  if (gpq_upload(dst.p, h.data(), n, nullptr) != GPQ_OK || gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");
}
// sample_uniform(q) as a RAW big slab of W words on the device
void sample_raw(gpq_ctx *c, const DevBuf &dst, gpq_MPI q, unsigned n, unsigned W, bool device, const uint8_t *drawn = nullptr) {
  const unsigned nbits = G.mpi_get_nbits(q);
  if (drawn) {
    if (gpq_sample_uniform(c, dst.u64(), drawn, nbits, W, 1, nullptr) != GPQ_OK) die("he_enc: the device sampler failed");
    return;
  }
  if (device) {
    const size_t nbytes = (size_t)n * (nbits / 8 + 1);
    std::vector<uint8_t> h(nbytes);
    randombytes(h.data(), nbytes);
    DevBuf bytes(nbytes);
    if (gpq_upload(bytes.p, h.data(), nbytes, nullptr) != GPQ_OK || gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");
    if (gpq_sample_uniform(c, dst.u64(), (const uint8_t *)bytes.p, nbits, W, 1, nullptr) != GPQ_OK) die("he_enc: the device sampler failed");
    return;
  }
  TmpPoly t(n);
  sample_uniform(&t.p, q);
  if (max_bits(&t.p, n) >= 64 * W) die("he_enc: the host's sample_uniform gave a coefficient wider than the modulus allows");
  std::vector<uint64_t> h((size_t)W * n);
  to_slab(h.data(), &t.p, n, W);
  up(dst, h);
  if (gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");
}

// kind 0: he_enc_pk (keys = pk.p0, pk.p1), 1: he_enc_sk (keys = sk), 2: he_keypair's arithmetic (keys = sk, no plaintext)
void enc_body(int kind, poly_mpi_t *out0, poly_mpi_t *out1, const poly_mpi_t *key0, const poly_mpi_t *key1, const poly_mpi_t *m) {
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, L = hectx.L, dim = hectx.dim;
  gpq_MPI q = hectx.q[L];
  const std::vector<uint64_t> qw = words_of(q, "he_enc: q_L must be positive");
  const bool pow2 = is_pow2(qw);
  const unsigned nbq = G.mpi_get_nbits(q), logq = nbq - 1;
  if (logq == 0) die("he_enc: q_L = 1");
  if (polyctx.logn < 2) die("he_enc: sample_zo needs n >= 4");
  const bool drawn = g_device_samplers && g_device_rng, device = drawn || (g_device_samplers && randombytes != nullptr);
  if (!device && (!sample_error || (kind == 0 ? !sample_zo : !sample_uniform)))
    die("he_enc / he_keypair: the host program does not provide sample_zo / sample_error / sample_uniform (src/sample.c)");
  const unsigned Wmin = nbq / 64 + 1;                        // holds the raw sample (nbq bits) as a non-negative value
  if (Wmin > 32) die("he_enc: modulus wider than 2047 bits");
  // the samples, in the reference's order, once per call (a repeated device pass reuses them)
  DevBuf dv(n), de0(n), de1(n);
  // device rng: every byte of the call at once -- zo, error, error (n/4 + 2n) resp. error, uniform (n + n (nbq / 8 + 1))
  const size_t ndrawn = kind == 0 ? (size_t)n / 4 + 2 * (size_t)n : (size_t)n + (size_t)n * (nbq / 8 + 1);
  std::unique_ptr<DevBuf> db;                                                                                                      // only with the device generator
  if (drawn) {
    db.reset(new DevBuf(ndrawn));
    if (gpq_randombytes_device(c, (uint8_t *)db->p, ndrawn, nullptr) != GPQ_OK) die("he_enc: generating the random bytes on the device failed");
  }
  const uint8_t *at = drawn ? (const uint8_t *)db->p : nullptr;
  if (kind == 0) {                                                                                                                // src/he-encrypt.c:50-56
    sample_small(c, dv, 0, n, device, at);
    sample_small(c, de0, 1, n, device, drawn ? at + n / 4 : nullptr);
    sample_small(c, de1, 1, n, device, drawn ? at + n / 4 + n : nullptr);
  } else sample_small(c, de0, 1, n, device, at);                                                                                  // :88, src/he-kem.c:56
  const int count = kind == 0 ? 3 : kind == 1 ? 2 : 1;
  const poly_mpi_t *in[3] = {key0, kind == 0 ? key1 : m, kind == 0 ? m : nullptr};
  poly_mpi_t *out[2] = {out0, out1};
  auto pass = [&](unsigned W, bool kept, const DevBuf *da) -> bool {
    if (W > 32) die("he_enc: coefficients wider than 2047 bits");
    const size_t big = (size_t)W * n, slab = (size_t)dim * n * 8;
    DevBuf k0(slab), k1(slab), tb(big * 8), scratch(192 * 8),
        ws(pow2 ? gpq_he_enc_workspace_bytes(c, dim, 1, kind == 0) : gpq_poly_mul_general_workspace_bytes(c, dim, 1));
    StagedCall call(n, W, count, in, 2);
    call.speculate = kept; call.report_misfits = true;
    auto ok = [](int rc) { if (rc != GPQ_OK) die("he_enc: the device work failed"); };
    auto add_small = [&](uint64_t *dst, const DevBuf &small) {                          // dst += small, through a big slab
      ok(gpq_small_to_big(c, tb.u64(), (const int8_t *)small.p, W, 1, nullptr));
      ok(gpq_big_addsub(c, dst, dst, tb.u64(), W, 1, 0, nullptr));
    };
    return call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
      if (kind == 0) {
        const uint64_t *p0 = x[0], *p1 = x[1], *mm = x[2];
        if (pow2) {
          ok(gpq_evk_pack(c, k0.u64(), p0, W, dim, 1, nullptr));
          ok(gpq_evk_pack(c, k1.u64(), p1, W, dim, 1, nullptr));
          ok(gpq_he_enc_pk(c, o[0], o[1], mm, (const int8_t *)dv.p, (const int8_t *)de0.p, (const int8_t *)de1.p, k0.u64(), k1.u64(), W, logq, dim, 1, ws.p, nullptr));
        } else {                                                                        // src/he-encrypt.c:58-66 call by call
          ok(gpq_small_to_big(c, tb.u64(), (const int8_t *)dv.p, W, 1, nullptr));
          ok(gpq_poly_mul_general(c, o[0], p0, tb.u64(), W, dim, qw.data(), (unsigned)qw.size(), 1, ws.p, nullptr));
          ok(gpq_poly_mul_general(c, o[1], p1, tb.u64(), W, dim, qw.data(), (unsigned)qw.size(), 1, ws.p, nullptr));
          ok(gpq_big_addsub(c, o[0], o[0], mm, W, 1, 0, nullptr));
          add_small(o[0], de0);
          add_small(o[1], de1);
          ok(gpq_he_rs_general(c, o[0], o[1], W, 1ull, qw.data(), (unsigned)qw.size(), 1, scratch.p, nullptr));
        }
      } else {
        const uint64_t *s = x[0], *mm = kind == 1 ? x[1] : nullptr;
        if (pow2) {
          ok(gpq_evk_pack(c, k0.u64(), s, W, dim, 1, nullptr));
          ok(gpq_he_enc_sk(c, o[0], o[1], mm, da->u64(), (const int8_t *)de0.p, k0.u64(), W, logq, dim, 1, ws.p, nullptr));
        } else {                                                                        // :91-97 / src/he-kem.c:59-64 call by call
          ok(gpq_poly_mul_general(c, o[0], da->u64(), s, W, dim, qw.data(), (unsigned)qw.size(), 1, ws.p, nullptr));
          ok(gpq_big_addsub(c, o[0], o[0], nullptr, W, 1, 2, nullptr));
          if (mm) ok(gpq_big_addsub(c, o[0], o[0], mm, W, 1, 0, nullptr));
          add_small(o[0], de0);
          if (hipMemcpyAsync(o[1], da->p, big * 8, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) die("device copy failed");
          ok(gpq_he_rs_general(c, o[0], o[1], W, 1ull, qw.data(), (unsigned)qw.size(), 1, scratch.p, nullptr));
        }
      }
    }, out) == StagedCall::Done;
  };
  // the width: what holds q and every operand; the raw sample is made at that width once it is known
  auto run = [&](unsigned W, bool kept) -> bool {
    if (kind == 0) return pass(W, kept, nullptr);
    DevBuf da((size_t)W * n * 8);
    sample_raw(c, da, q, n, W, device, drawn ? at + n : nullptr);                                                 // src/he-encrypt.c:89, src/he-kem.c:58
    return pass(W, kept, &da);
  };
  unsigned bits = nbq;
  for (int i = 0; i < count; ++i) { const unsigned bi = max_bits(in[i], n); if (bi > bits) bits = bi; }
  const unsigned W = (bits + 1) / 64 + 1 > Wmin ? (bits + 1) / 64 + 1 : Wmin;
  if (!run(W, true)) die("he_enc: an operand changed width during the call");   // (operands with a trusted resident copy at this width are taken from it)
}
}  // namespace
extern "C" {

void he_enc_pk(struct he_ct *ct, const struct he_pt *pt, const struct he_pk *pk) {
  SHIM_CALL();
  need_hectx();
  ct->l = hectx.L;                                                                       // src/he-encrypt.c:40-42
  ct->nu = pt->nu >= hectx.Delta ? pt->nu : hectx.Delta;
  ct->B = hectx.bnd.Bclean;
  enc_body(0, &ct->c0, &ct->c1, &pk->p0, &pk->p1, &pt->m);
}

void he_enc_sk(struct he_ct *ct, const struct he_pt *pt, const poly_mpi_t *sk) {
  SHIM_CALL();
  need_hectx();
  ct->l = hectx.L;                                                                       // :78-80
  ct->nu = pt->nu >= hectx.Delta ? pt->nu : hectx.Delta;
  ct->B = hectx.bnd.Bclean;
  enc_body(1, &ct->c0, &ct->c1, sk, nullptr, &pt->m);
}

void he_keypair(he_pk_t *pk, poly_mpi_t *sk) {                                            // src/he-kem.c:43-71
  SHIM_CALL();
  need_hectx();
  if (!sample_sk) die("he_keypair: the host program does not provide sample_sk (src/sample.c)");
  printf("Generating sk and pk ... ");
  fflush(stdout);
  forget_poly(sk); forget_poly(&pk->p0); forget_poly(&pk->p1);                             // about to be rewritten: their device copies go first
  sample_sk(sk);                                                                          // :52
  enc_body(2, &pk->p0, &pk->p1, sk, nullptr, nullptr);
  printf("done.\n");
}

void gpq_mpi_shim_set_device_samplers(int on) { SHIM_CALL(); g_device_samplers = on != 0; }
void gpq_mpi_shim_set_device_rng(int on) { SHIM_CALL(); g_device_rng = on != 0; }
