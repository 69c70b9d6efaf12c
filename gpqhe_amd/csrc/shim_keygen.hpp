// shim_keygen.hpp -- he_genswk / he_genrlk / he_genck / he_genrk (src/he-kem.c:74-170) with the reference's signatures.  Included inside mpi_shim.hip's extern "C" block.
// Part of the MPI-typed surface: one translation unit (mpi_shim.hip includes these fragments in order); split by concern in round 4.
#pragma once

// ---- key generation, src/he-kem.c:74-170 -----------------------------------------------------------------------------
// he_genswk (static in the reference, :74-118) for `count` keys through gpq_he_genswk_batch.  The secret is converted and packed ONCE per
// he_gen*k call (an int8 small slab for the kernel's gather, gpq_evk_pack over the product's limbs); keys are made in groups of at most
// kKeygenGroup, so host memory stays bounded, with two downloads per group.  The samplers are the host program's, in the reference's order
// per key -- sample_error, then sample_uniform(P q_L) -- so a seeded RNG gives the reference's own keys; with
// gpq_mpi_shim_set_device_samplers(1) the host's randombytes is called instead, once per sampler call with the reference's byte counts
// (n, then n (nbits/8 + 1)), and gpq_sample_error / gpq_sample_uniform expand the group's byte buffer on the device, one launch per key
// slice: no sampled polynomial becomes libgcrypt integers.  With gpq_mpi_shim_set_device_rng(1) as well the group's byte buffer is not
// drawn from the host at all: ONE gpq_randombytes_device reserves the same bytes from the default stream and makes them on the device.
} // extern "C"
namespace {
constexpr unsigned kKeygenGroup = 32;                       // the engine's default launch group (gpq_set_chunk)

struct KeygenSecret {                                       // what every key of a call shares
  unsigned W = 0, Wsk = 0, dimmul = 0, logqL = 0, nbits = 0;
  bool small = false;                                       // every coefficient fits int8: the kernel gathers the hidden polynomial itself
  std::unique_ptr<DevBuf> big, ntt, i8;
};

void keygen_secret(KeygenSecret &k, const poly_mpi_t *sk) {
  need_hectx();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n;
  if (!is_pow2(words_of(hectx.q[hectx.L], "he_gen*k: q_L must be positive"))) die("he_gen*k: q_L must be a power of two on this path");
  k.logqL = G.mpi_get_nbits(hectx.q[hectx.L]) - 1;
  k.nbits = G.mpi_get_nbits(hectx.PqL);
  k.W = k.nbits / 64 + 1;
  if (!(k.dimmul = gpq_he_genswk_dimmul(c, hectx.dim, k.logqL))) die("he_gen*k: the modulus P q_L is outside what the engine supports");
  const unsigned bits = max_bits(sk, n);
  k.small = bits <= 7;
  k.Wsk = bits / 64 + 1;
  std::vector<uint64_t> hs((size_t)k.Wsk * n);
  to_slab(hs.data(), sk, n, k.Wsk);
  k.big.reset(new DevBuf(hs.size() * 8));
  k.ntt.reset(new DevBuf((size_t)k.dimmul * n * 8));
  up(*k.big, hs);
  if (gpq_evk_pack(c, k.ntt->u64(), k.big->u64(), k.Wsk, k.dimmul, 1, nullptr) != GPQ_OK) die("he_gen*k: packing the secret failed");
  if (k.small) {
    std::vector<int8_t> h8(n);
    for (unsigned i = 0; i < n; ++i) h8[i] = (int8_t)(int64_t)hs[i];
    k.i8.reset(new DevBuf(n));
    if (gpq_upload(k.i8->p, h8.data(), n, nullptr) != GPQ_OK) die("upload failed");
  }
  if (gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");                            // (the host vectors go out of scope)
}

// keys swk[0..count): the hidden polynomial of key j is the image of the secret under X -> X^galois[j] -- poly_conj (conj) or poly_rot by j --
// or (galois == nullptr, count == 1) the device big slab sp of Wsp words
void genswk_keys(he_evk_t *swk, unsigned count, const KeygenSecret &k, const uint64_t *galois, bool conj, const uint64_t *sp, unsigned Wsp) {
  const bool drawn = g_device_samplers && g_device_rng, device = drawn || (g_device_samplers && randombytes != nullptr);
  if (!device && (!sample_error || !sample_uniform)) die("he_gen*k: the host program does not provide sample_error / sample_uniform (src/sample.c)");
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, W = k.W, dimevk = hectx.dimevk, nb = k.nbits / 8 + 1;
  const size_t big = (size_t)W * n, evk = (size_t)dimevk * n;
  for (unsigned k0 = 0; k0 < count; k0 += kKeygenGroup) {
    const unsigned m = count - k0 < kKeygenGroup ? count - k0 : kKeygenGroup;
    for (unsigned j = 0; j < m; ++j) forget_key_at(swk[k0 + j].p0.coeffs, swk[k0 + j].p1.coeffs);   // about to be rewritten: their device copies go first
    DevBuf dp(m * big * 8), de((size_t)m * n), d0(m * evk * 8), d1(m * evk * 8),
        ws(gpq_he_genswk_batch_workspace_bytes(c, W, hectx.dim, k.logqL, dimevk, m));
    if (device) {
      std::vector<uint8_t> bytes(drawn ? 0 : (size_t)m * ((size_t)n + (size_t)n * nb));
      DevBuf db((size_t)m * ((size_t)n + (size_t)n * nb));
      if (drawn) {                                                                          // the same slices of one stream, made where they are read
        if (gpq_randombytes_device(c, (uint8_t *)db.p, (size_t)m * ((size_t)n + (size_t)n * nb), nullptr) != GPQ_OK) die("he_gen*k: generating the random bytes on the device failed");
      } else {
        for (unsigned j = 0; j < m; ++j) {
          uint8_t *at = bytes.data() + (size_t)j * ((size_t)n + (size_t)n * nb);
          randombytes(at, n);                                                               // sample_error, :87
          randombytes(at + n, (size_t)n * nb);                                              // sample_uniform(P q_L), :94
        }
        if (gpq_upload(db.p, bytes.data(), bytes.size(), nullptr) != GPQ_OK) die("upload failed");
      }
      for (unsigned j = 0; j < m; ++j) {
        const uint8_t *at = (const uint8_t *)db.p + (size_t)j * ((size_t)n + (size_t)n * nb);
        if (gpq_sample_error(c, (int8_t *)de.p + (size_t)j * n, at, 1, nullptr) != GPQ_OK ||
            gpq_sample_uniform(c, dp.u64() + j * big, at + n, k.nbits, W, 1, nullptr) != GPQ_OK) die("he_gen*k: the device sampler failed");
      }
      if (gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");                        // (`bytes` goes out of scope)
    } else {
      std::vector<uint64_t> hp(m * big), w(n);
      std::vector<int8_t> he((size_t)m * n);
      TmpPoly t(n);
      for (unsigned j = 0; j < m; ++j) {
        sample_error(&t.p);                                                                 // :87
        if (max_bits(&t.p, n) > 7) die("he_gen*k: the host's sample_error gave a coefficient outside [-127, 127]");
        to_slab(w.data(), &t.p, n, 1);
        for (unsigned i = 0; i < n; ++i) he[(size_t)j * n + i] = (int8_t)(int64_t)w[i];
        sample_uniform(&t.p, hectx.PqL);                                                    // :94
        if (max_bits(&t.p, n) >= 64 * W) die("he_gen*k: the host's sample_uniform gave a coefficient wider than the modulus allows");
        to_slab(hp.data() + j * big, &t.p, n, W);
      }
      up(dp, hp);
      if (gpq_upload(de.p, he.data(), he.size(), nullptr) != GPQ_OK || gpq_stream_sync(nullptr) != GPQ_OK) die("upload failed");
    }
    int rc;
    if (galois && k.small) {
      rc = gpq_he_genswk_batch(c, d0.u64(), d1.u64(), dp.u64(), (const int8_t *)de.p, k.ntt->u64(), (const int8_t *)k.i8->p, galois + k0, nullptr, 0, W,
                               hectx.dim, k.logqL, dimevk, m, ws.p, nullptr);
    } else if (galois) {                                    // a secret beyond int8: its images as big slabs, permuted on the device
      const size_t one = (size_t)k.Wsk * n;
      DevBuf dsp(m * one * 8);
      for (unsigned j = 0; j < m; ++j)
        if ((conj ? gpq_poly_conj(c, dsp.u64() + j * one, k.big->u64(), k.Wsk, 1, nullptr)
                  : gpq_poly_rot(c, dsp.u64() + j * one, k.big->u64(), k.Wsk, k0 + j, 1, nullptr)) != GPQ_OK) die("poly_rot / poly_conj failed");
      rc = gpq_he_genswk_batch(c, d0.u64(), d1.u64(), dp.u64(), (const int8_t *)de.p, k.ntt->u64(), nullptr, nullptr, dsp.u64(), k.Wsk, W, hectx.dim,
                               k.logqL, dimevk, m, ws.p, nullptr);
    } else {
      rc = gpq_he_genswk_batch(c, d0.u64(), d1.u64(), dp.u64(), (const int8_t *)de.p, k.ntt->u64(), nullptr, nullptr, sp, Wsp, W, hectx.dim, k.logqL,
                               dimevk, m, ws.p, nullptr);
    }
    if (rc != GPQ_OK) die("he_genswk failed");
    std::vector<uint64_t> h0(m * evk), h1(m * evk);
    if (gpq_download(h0.data(), d0.p, h0.size() * 8, nullptr) != GPQ_OK || gpq_download(h1.data(), d1.p, h1.size() * 8, nullptr) != GPQ_OK ||
        gpq_stream_sync(nullptr) != GPQ_OK) die("download failed");
    for (unsigned j = 0; j < m; ++j) {
      memcpy(swk[k0 + j].p0.coeffs, h0.data() + j * evk, evk * 8);
      memcpy(swk[k0 + j].p1.coeffs, h1.data() + j * evk, evk * 8);
    }
  }
}
}  // namespace
extern "C" {

void he_genrlk(he_evk_t *rlk, const poly_mpi_t *sk) {                                              // :120-137
  SHIM_CALL();
  KeygenSecret k;
  keygen_secret(k, sk);
  const unsigned n = polyctx.n;
  gpq_ctx *c = engine();
  printf("Generating rlk ... ");
  fflush(stdout);
  const unsigned nbq = G.mpi_get_nbits(hectx.q[hectx.L]), dim = nbq / 59 + 1;                      // :131
  const unsigned Ws = k.Wsk > nbq / 64 + 1 ? k.Wsk : nbq / 64 + 1;                                  // holds the secret and s^2 centred mod q_L
  const size_t big = (size_t)Ws * n;
  DevBuf a(big * 8), r(big * 8), ws(gpq_poly_mul_workspace_bytes(c, dim, 1));
  std::vector<uint64_t> hs(big);
  to_slab(hs.data(), sk, n, Ws);
  up(a, hs);
  if (gpq_poly_mul(c, r.u64(), a.u64(), a.u64(), Ws, dim, nbq - 1, 1, ws.p, nullptr) != GPQ_OK) die("he_genrlk: poly_mul failed");
  genswk_keys(rlk, 1, k, nullptr, false, r.u64(), Ws);                                                    // :132
  printf("done.\n");
}

void he_genck(he_evk_t *ck, const poly_mpi_t *sk) {                                                // :140-154
  SHIM_CALL();
  KeygenSecret k;
  keygen_secret(k, sk);
  printf("Generating ck ... ");
  fflush(stdout);
  const uint64_t g = 2ull * polyctx.n - 1;                                                         // poly_conj, src/poly.c:277-283
  genswk_keys(ck, 1, k, &g, true, nullptr, 0);
  printf("done.\n");
}

void he_genrk(he_evk_t *rk, const poly_mpi_t *sk) {                                                // :156-170
  SHIM_CALL();
  KeygenSecret k;
  keygen_secret(k, sk);
  printf("Generating rk ... ");
  fflush(stdout);
  std::vector<uint64_t> g(hectx.slots);
  uint64_t power = 1;
  for (unsigned rot = 0; rot < hectx.slots; ++rot, power *= 5) g[rot] = power;                     // poly_rot, src/poly.c:266-268
  genswk_keys(rk, hectx.slots, k, g.data(), false, nullptr, 0);
  printf("done.\n");
}

// wall milliseconds of the last he_mul(he_ct_t*, ...) call: [0] MPI -> slab conversions and uploads, [1] device kernels,
// [2] downloads and slab -> MPI conversions (includes waiting for [1]), [3] the whole call
void gpq_mpi_shim_last_timing(double ms[4]) { for (int i = 0; i < 4; ++i) ms[i] = g_last_ms[i]; }

// How many evaluation keys stay on the device between calls (default 64; he_rot over many rotation keys -- the gemv of
// src/he-algo.c:63-85 walks rk[0..slots) -- wants as many as it cycles through: 45 MiB each at n = 2^16, 45 limbs).
void gpq_mpi_shim_set_key_slots(unsigned slots) {
  SHIM_CALL();
  g_key_slots = slots ? slots : 1;
  while (g_keys.size() > g_key_slots) {                     // resident keys beyond the new limit go at once, least recently used first
    size_t victim = 0;
    for (size_t i = 1; i < g_keys.size(); ++i) if (g_keys[i].used < g_keys[victim].used) victim = i;
    drop_key_slot(victim);
  }
}
// 1 (default): a resident key is recognised by a fingerprint of every word, computed by the conversion threads beside the
// ciphertext conversions; 0: by ~1000 sampled words (for programs that never edit a key in place; gpq_mpi_shim_forget_keys covers the rest)
void gpq_mpi_shim_set_key_check(int full) { SHIM_CALL(); g_key_check_full = full != 0; }
unsigned gpq_mpi_shim_resident_keys(void) { SHIM_CALL(); return (unsigned)g_keys.size(); }
// 1 (default): libgcrypt integers are read and written limb by limb in place once the layout probe has passed (mpi_convert.hpp);
// 0: every coefficient goes through gcry_mpi_print / gcry_mpi_scan.  Returns whether the direct path is in use afterwards.
int gpq_mpi_shim_set_direct_mpi(int on) { SHIM_CALL(); need_gcrypt(); g_mpi_direct_wanted = on != 0; return mpi_direct() ? 1 : 0; }

// Drops the device copies of evaluation keys (he_mul / he_rot / he_conj keep up to gpq_mpi_shim_set_key_slots of them, recognised by the caller's pointers, the
// length and a fingerprint of every word -- of ~1000 sampled words after gpq_mpi_shim_set_key_check(0), and then a program that rewrites a
// key IN PLACE in a way the samples may miss must call this after the rewrite).  he_gen*k drop the slot of the key they write themselves.
void gpq_mpi_shim_forget_keys(void) {
  SHIM_CALL();
  (void)gpq_stream_sync(nullptr);
  for (KeySlot &k : g_keys) { (void)gpq_free(k.d0); (void)gpq_free(k.d1); }
  g_keys.clear();
}

// Resident polynomials (see PolySlot above): how many device copies of the caller's polynomials are kept between calls (default 32, 7 MiB each at
// n = 2^16 and 14 words; 0 = none: every call converts and uploads its operands before the device starts, as up to round 2).
void gpq_mpi_shim_set_poly_slots(unsigned slots) {
  SHIM_CALL();
  g_poly_slots = slots;
  while (g_polys.size() > g_poly_slots) {
    size_t victim = 0;
    for (size_t i = 1; i < g_polys.size(); ++i) if (g_polys[i].used < g_polys[victim].used) victim = i;
    drop_poly_slot(victim);
  }
}
// Host threads that convert between libgcrypt integers and slabs (default: the hardware threads, at most 16; up to 64).  Takes effect only
// before the first MPI-typed call of the process (the pool is started once); returns the number in use afterwards.
unsigned gpq_mpi_shim_set_conversion_threads(unsigned threads) { SHIM_CALL(); g_workers_wanted = threads; return workers().width(); }
unsigned gpq_mpi_shim_resident_polys(void) { SHIM_CALL(); return (unsigned)g_polys.size(); }
// operands served from a resident copy that the check confirmed / that the check found changed (uploaded again, device work repeated)
void gpq_mpi_shim_poly_stats(uint64_t *confirmed, uint64_t *stale) { SHIM_CALL(); if (confirmed) *confirmed = g_poly_hits; if (stale) *stale = g_poly_stale; }
// testing: while on, the MPI-typed calls convert and upload everything and remember nothing, without touching what is resident
void gpq_mpi_shim_poly_bypass(int on) { SHIM_CALL(); g_poly_bypass = on != 0; }
void gpq_mpi_shim_forget_polys(void) {
  SHIM_CALL();
  (void)gpq_stream_sync(nullptr);
  for (PolySlot &k : g_polys) (void)gpq_free(k.d);
  g_polys.clear();
}

// frees the device buffers the MPI-typed calls keep between calls, and the engine context
void gpq_mpi_shim_release(void) {
  SHIM_CALL();
  (void)gpq_stream_sync(nullptr);
  for (PolySlot &k : g_polys) (void)gpq_free(k.d);
  g_polys.clear();
  for (auto &kv : g_pool) for (void *q : kv.second) (void)gpq_free(q);
  g_pool.clear();
  for (auto &kv : g_pinned) for (void *q : kv.second) (void)hipHostFree(q);
  g_pinned.clear();
  for (KeySlot &k : g_keys) { (void)gpq_free(k.d0); (void)gpq_free(k.d1); }
  g_keys.clear();
  for (hipEvent_t e : g_events) (void)hipEventDestroy(e);
  g_events.clear();
  gemv_plans_drop(0);
  if (g_engine) { gpq_ctx_destroy(g_engine); g_engine = nullptr; }
}

void he_rs(struct he_ct *ct) { rescale_common(ct, true); }        // src/he-rescale.c:33-54
void he_rescale(struct he_ct *ct) { rescale_common(ct, true); }
void he_moddown(he_ct_t *ct) { rescale_common(ct, false); }       // src/he-rescale.c:56-70

