// mpi_shim.hip -- poly_mul / he_mul / he_rs / he_rescale / he_moddown with the reference's own
// MPI-typed signatures (src/poly.h:86-87, src/gpqhe.h:136-137,147), so that GPQHE objects which
// call them link against libgpqhe_hip.so unchanged.  The work itself is the device code behind
// gpq_poly_mul / gpq_he_mul / gpq_he_rs; this file only moves coefficients between libgcrypt MPIs
// and big slabs and mirrors the host-side bookkeeping (ct->l, nu, B).
//
// libgcrypt is reached through its runtime ABI only (dlsym on the library the host program has
// loaded, or libgcrypt.so.20): this image ships no <gcrypt.h>, and none is needed.
#include "../../include/gpqhe_hip.h"
#include "../../include/gpqhe_hip_compat.h"

#include <dlfcn.h>
#include <sys/random.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <set>
#include <thread>
#include <vector>

extern "C" struct poly_ctx polyctx __attribute__((weak));   // src/precomp.c:41
extern "C" struct he_ctx hectx __attribute__((weak));       // src/precomp.c:47
// the reference's samplers (src/sample.c; externs at src/he-kem.c:33-34): key generation draws from them in the reference's order
extern "C" void sample_error(poly_mpi_t *r) __attribute__((weak));
extern "C" void sample_uniform(poly_mpi_t *r, const gpq_MPI q) __attribute__((weak));
// ... and encryption / he_keypair (src/he-encrypt.c:33-35, src/he-kem.c:32): sample_zo, sample_sk; randombytes (src/rng.c) feeds the device
// samplers after gpq_mpi_shim_set_device_samplers(1)
extern "C" void sample_zo(poly_mpi_t *r) __attribute__((weak));
extern "C" void sample_sk(poly_mpi_t *r) __attribute__((weak));
extern "C" void randombytes(uint8_t *x, size_t xlen) __attribute__((weak));
// the reference's encoder (src/he-encode.c:107-111): he_gemv / he_sum / he_idx encode their diagonals with the host program's own
extern "C" void he_ecd(struct he_pt *pt, const _Complex double *m) __attribute__((weak));

#include "mpi_convert.hpp"
#include "algo_seq.hpp"         // the evaluators' sequences and their host bookkeeping (shim_evaluators.hpp)

// Every copy, kernel and event of the MPI-typed calls goes to the legacy null stream (stream argument nullptr), from the calling thread and
// from the conversion threads alike: that ONE stream is what orders a range's upload before the transposes and kernels that read it, and a
// pooled buffer's reuse behind its last reader.  With per-thread default streams nullptr would mean a different stream in every thread.
#if defined(HIP_API_PER_THREAD_DEFAULT_STREAM)
#error "mpi_shim.hip relies on the legacy (process-wide) null stream: build without -fgpu-default-stream=per-thread"
#endif

#include "shim_gemv_plans.hpp"
#include "shim_staging.hpp"
#include "shim_keys.hpp"
#include "shim_polys.hpp"
#include "shim_call.hpp"

namespace {

// The MPI-typed entry points share the staging buffers, the buffer pools, the key cache and the worker threads: one call at a
// time (the reference itself is single-threaded; a second host thread simply waits here).  Recursive: he_rescale -> he_rs etc.
std::recursive_mutex g_call_mu;
#define SHIM_CALL() std::lock_guard<std::recursive_mutex> shim_call_lock(g_call_mu)

}  // namespace

extern "C" {

// index of this node's prime in the chain: a node with `dim` limbs carries prime dim-1 (src/precomp.c:266-293)
static unsigned limb_of(gpq_ctx *c, const struct rns_ctx *rns, const char *who) {
  if (!rns || rns->dim < 1 || rns->dim > gpq_ctx_nprimes(c) || gpq_ctx_const(c, rns->dim - 1, 0) != rns->p) die(who);
  return rns->dim - 1;
}

// src/rns.c:37-48 -- one limb: ahat[i] = a[i] mod rns->p, non-negative
void rns_decompose(uint64_t ahat[], const gpq_MPI a[], const struct rns_ctx *rns) {
  SHIM_CALL();
  need_gcrypt();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, limb = limb_of(c, rns, "rns_decompose: the node is not one of the caller's prime chain");
  poly_mpi_t view{const_cast<gpq_MPI *>(a)};
  const unsigned W = max_bits(&view, n) / 64 + 1;
  if (W > 32) die("rns_decompose: coefficients wider than 2047 bits");
  std::vector<uint64_t> h((size_t)W * n);
  to_slab(h.data(), &view, n, W);
  DevBuf big(h.size() * 8), out((size_t)n * 8);
  up(big, h);
  if (gpq_rns_decompose_limbs(c, out.u64(), big.u64(), W, limb, 1, 1, nullptr) != GPQ_OK) die("rns_decompose failed");
  if (gpq_download(ahat, out.p, (size_t)n * 8, nullptr) != GPQ_OK || gpq_stream_sync(nullptr) != GPQ_OK) die("download failed");
}

static void set_from_words(MPI r, const uint64_t *w, unsigned W) {
  poly_mpi_t one{&r};
  from_slab(&one, w, 1, W);
}

// src/rns.c:60-75 -- coefficient i of a slab with rns->dim limbs, value in [0, P)
void rns_reconstruct(gpq_MPI a, const uint64_t ahat[], const unsigned int i, const struct rns_ctx *rns) {
  SHIM_CALL();
  need_gcrypt();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n;
  (void)limb_of(c, rns, "rns_reconstruct: the node is not one of the caller's prime chain");
  if (i >= n) die("rns_reconstruct: coefficient index out of range");
  const unsigned dim = rns->dim, W = gpq_ctx_pbits(c, dim) / 64 + 2;
  std::vector<uint64_t> col(dim), w(W);
  for (unsigned d = 0; d < dim; ++d) col[d] = ahat[(size_t)d * n + i];
  if (gpq_rns_reconstruct_one(c, w.data(), W, col.data(), dim) != GPQ_OK) die("rns_reconstruct failed");
  set_from_words(a, w.data(), W);
}

// src/poly.c:109-120 -- every coefficient: reconstruct, centre mod P, centre mod q
void poly_rns2mpi(poly_mpi_t *r, const poly_rns_t *rhat, const struct rns_ctx *rns, const gpq_MPI q) {
  SHIM_CALL();
  need_gcrypt();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n;
  (void)limb_of(c, rns, "poly_rns2mpi: the node is not one of the caller's prime chain");
  const unsigned dim = rns->dim;
  const std::vector<uint64_t> qw = words_of(q, "poly_rns2mpi: the modulus must be positive");
  const unsigned nbq = G.mpi_get_nbits(q), W = nbq / 64 + 1;
  if (qw.size() > 48) die("poly_rns2mpi: modulus wider than 48 words");
  DevBuf slab((size_t)dim * n * 8), big((size_t)W * n * 8), scratch(gpq_poly_mul_general_workspace_bytes(c, dim, 1));
  if (gpq_upload(slab.p, rhat->coeffs, (size_t)dim * n * 8, nullptr) != GPQ_OK) die("upload failed");
  const int rc = is_pow2(qw) ? gpq_rns_reconstruct(c, big.u64(), W, slab.u64(), dim, 1, nbq - 1, nullptr)
                             : gpq_rns_reconstruct_general(c, big.u64(), W, slab.u64(), dim, 1, qw.data(), (unsigned)qw.size(), scratch.p, nullptr);
  if (rc != GPQ_OK) die("poly_rns2mpi failed");
  std::vector<uint64_t> h((size_t)W * n);
  down(h, big);
  from_slab(r, h.data(), n, W);
}

// src/poly.c:84-107
void poly_mul(poly_mpi_t *r, const poly_mpi_t *a, const poly_mpi_t *b, const unsigned int dim, const gpq_MPI q) {
  SHIM_CALL();
  need_gcrypt();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n;
  const std::vector<uint64_t> qw = words_of(q, "poly_mul: the modulus must be positive");
  const unsigned nbq = G.mpi_get_nbits(q);
  const poly_mpi_t *in[2] = {a, b};
  poly_mpi_t *out[1] = {r};
  const bool pow2 = is_pow2(qw);
  const int count = a->coeffs == b->coeffs ? 1 : 2;
  // one pass at W words per coefficient; with `kept`, from the resident copies of both operands (false: one of them has outgrown its copy)
  auto pass = [&](unsigned W, bool kept) -> bool {
    if (W > 32) die("poly_mul: coefficients wider than 2047 bits");
    DevBuf ws(gpq_poly_mul_general_workspace_bytes(c, dim, 1));
    StagedCall call(n, W, count, in, 1);
    call.speculate = kept; call.report_misfits = true;
    return call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
      const uint64_t *xa = x[0], *xb = count == 1 ? xa : x[1];
      const int rc = pow2 ? gpq_poly_mul(c, o[0], xa, xb, W, dim, nbq - 1, 1, ws.p, nullptr)
                          : gpq_poly_mul_general(c, o[0], xa, xb, W, dim, qw.data(), (unsigned)qw.size(), 1, ws.p, nullptr);
      if (rc != GPQ_OK) die("poly_mul failed");   // q = P*q_L in he_genswk (src/he-kem.c:95) takes the general path
    }, out) == StagedCall::Done;
  };
  // (he_dec multiplies a chained ciphertext's c1 with the same secret key every time)
  width_ladder(in, count, n, true, nbq / 64 + 1, nbq, 0, pass);
}

#include "shim_decrypt.hpp"
#include "shim_encrypt.hpp"

// src/he-mult.c:88-156
void he_mul(he_ct_t *ct, const he_ct_t *ct1, const he_ct_t *ct2, const he_evk_t *rlk) {
  SHIM_CALL();
  need_hectx();
  if (ct1->l != ct2->l) die("he_mul: operands at different levels");   // assert at src/he-mult.c:90
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, l = ct1->l;
  const double nu = ct1->nu * ct2->nu;                                                        // :93
  // :94-95 read ct1->nu / ct2->nu AFTER :93 has stored the product in ct->nu: where ct is one of the operands (he_mul(&ct, &ct, &ct),
  // src/he-algo.c:151) the reference builds B from the NEW nu -- measured against the executed reference (tests/c/mpi_host.c, mode ref)
  const double nu1 = ct == ct1 ? nu : ct1->nu, nu2 = ct == ct2 ? nu : ct2->nu;
  const double B = nu1 * ct2->B + nu2 * ct1->B + ct1->B * ct2->B + hectx.bnd.Bmult[l];         // :94-95
  const std::vector<uint64_t> qw = words_of(hectx.q[l], "he_mul: q_l must be positive");
  const bool pow2 = is_pow2(qw);
  const unsigned nbq = G.mpi_get_nbits(hectx.q[l]), logql = nbq - 1, nbPqL = G.mpi_get_nbits(hectx.PqL);
  const unsigned dimA = (nbq * 2 + polyctx.logn) / 59 + 1;                                     // :99
  const unsigned dimB = (nbq + nbPqL + polyctx.logn) / 59 + 1;                                 // :51
  const unsigned dimP = hectx.dim;                                                             // hectx.P, src/precomp.c:401-404
  if (gpq_ctx_pbits(c, dimP) != G.mpi_get_nbits(hectx.P)) die("he_mul: hectx.P is not the product of the first hectx.dim primes");
  const unsigned W = logql / 64 + 1;
  const poly_mpi_t *in[4] = {&ct1->c0, &ct1->c1, &ct2->c0, &ct2->c1};
  poly_mpi_t *out[2] = {&ct->c0, &ct->c1};
  DevBuf ws(pow2 ? gpq_he_mul_workspace_bytes(c, W, dimA, dimB, dimP, 1) : gpq_he_general_workspace_bytes(c, W, dimA, dimB, dimP, 1));
  // he_mul(&ct, &ct, &ct, rlk), src/he-algo.c:151: one ciphertext on both sides -- convert and upload it once, square on the device
  const bool square = ct1->c0.coeffs == ct2->c0.coeffs && ct1->c1.coeffs == ct2->c1.coeffs;
  StagedCall call(n, W, square ? 2 : 4, in, 2);
  const double t0 = wall_ms();
  CallKey key(rlk, dimB, n);                         // operands and key are checked against the caller's memory while the device works
  key.ride(call);
  call.prepare();
  key.settle();
  if (!g_tick[0]) { (void)hipEventCreate(&g_tick[0]); (void)hipEventCreate(&g_tick[1]); }
  (void)hipEventRecord(g_tick[0], nullptr);
  const double t1 = wall_ms();
  call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
    const uint64_t *const a0 = x[0], *const a1 = x[1], *const e0 = square ? a0 : x[2], *const e1 = square ? a1 : x[3];
    const int rc = pow2 ? gpq_he_mul(c, o[0], o[1], a0, a1, e0, e1, key.k0, key.k1, W, logql, dimA, dimB, dimP, 1, ws.p, nullptr)
                        : gpq_he_mul_general(c, o[0], o[1], a0, a1, e0, e1, key.k0, key.k1, W, qw.data(),
                                             (unsigned)qw.size(), dimA, dimB, dimP, 1, ws.p, nullptr);
    if (rc != GPQ_OK) die("he_mul failed");
    (void)hipEventRecord(g_tick[1], nullptr);
  }, out);
  const double t2 = call.queued_ms, t3 = wall_ms();
  float dev_ms = 0;
  (void)hipEventElapsedTime(&dev_ms, g_tick[0], g_tick[1]);
  g_last_ms[0] = t1 - t0; g_last_ms[1] = dev_ms; g_last_ms[2] = t3 - t2; g_last_ms[3] = t3 - t0;
  ct->l = l; ct->nu = nu; ct->B = B;                                                           // :92-95
}

static void rescale_common(he_ct_t *ct, bool divide) {
  SHIM_CALL();
  need_hectx();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n;
  if (ct->l == 0) die("he_rs / he_moddown: already at level 0");
  const unsigned lnew = ct->l - 1;                                                             // src/he-rescale.c:36, :59
  const std::vector<uint64_t> qw = words_of(hectx.q[lnew], "he_rs: q_l must be positive");
  const std::vector<uint64_t> dw = words_of(hectx.p, "he_rs: Delta must be positive");
  if (dw.size() != 1) die("he_rs: Delta wider than 64 bits");          // hectx_init takes a uint64_t, src/gpqhe.h:100
  const bool pow2 = is_pow2(qw) && (!divide || is_pow2(dw));
  const unsigned logql = G.mpi_get_nbits(hectx.q[lnew]) - 1;
  const unsigned s = divide ? G.mpi_get_nbits(hectx.p) - 1 : 0;
  const poly_mpi_t *in[2] = {&ct->c0, &ct->c1};
  poly_mpi_t *out[2] = {&ct->c0, &ct->c1};
  if (logql == 0) {                                          // q_0 = 1
    fill_minus_one(out[0], n); fill_minus_one(out[1], n);
    ct->l = lnew;
    if (divide) { ct->nu /= hectx.Delta; ct->B = ct->B / hectx.Delta + hectx.bnd.Brs; }
    return;
  }
  const unsigned Wout = logql / 64 + 1;                    // the results are centred mod q_lnew: they fit the width he_mul uses at that level
  // One pass at W words per coefficient; with `kept`, from the resident copies of both polynomials (returns false if one of them
  // turned out wider than its copy: the caller measures the integers and runs again)
  auto pass = [&](unsigned W, bool kept) -> bool {
    DevBuf scratch(192 * 8);
    StagedCall call(n, W, 2, in, 2, true);
    call.speculate = kept; call.report_misfits = true; call.Wdown = Wout < W ? Wout : W;
    return call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
      for (int i = 0; i < 2; ++i)                            // gpq_he_rs works in place: a resident copy is copied, not lent
        if (x[i] != o[i] && hipMemcpyAsync(o[i], x[i], (size_t)W * n * 8, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) die("device copy failed");
      const int rc = pow2 ? gpq_he_rs(c, o[0], o[1], W, s, logql, 1, nullptr)                                          // :45-48 / :64-65
                          : gpq_he_rs_general(c, o[0], o[1], W, divide ? dw[0] : 1ull, qw.data(), (unsigned)qw.size(), 1, scratch.p, nullptr);
      if (rc != GPQ_OK) die("he_rs failed");
    }, out) == StagedCall::Done;
  };
  width_ladder(in, 2, n, true, Wout, logql + 1, 0, pass);
  ct->l = lnew;
  if (divide) { ct->nu /= hectx.Delta; ct->B = ct->B / hectx.Delta + hectx.bnd.Brs; }             // :37-38
}

// ---- constant plaintexts ---------------------------------------------------------------------------------------------------------
// he_const_pt (src/he-encode.c:119-125) writes m[0] and m[n/2] of a plaintext that is 0 elsewhere, and the reference's algorithms
// (he_inv, he_sqrt, he_sigmoid, he_log, he_exp_taylor, he_cmp*, he_coeff2slot) multiply and add such plaintexts between all their he_mul
// calls.  For q_l = 2^k the product and the sums with a + b x^(n/2) are closed forms on the ciphertext's words alone (constpt_kernels.hpp):
// the plaintext is then no operand -- neither converted nor uploaded nor kept resident -- and the call is one launch.  Same words as the
// dense path (he_mulpt: for centred inputs, which the kernel checks); gpq_mpi_shim_set_const_pt(0) keeps every plaintext dense.
static bool g_const_pt_on = true;
static unsigned long g_const_taken = 0, g_const_fell_back = 0;
void gpq_mpi_shim_set_const_pt(int on) { SHIM_CALL(); g_const_pt_on = on != 0; }
void gpq_mpi_shim_const_pt_stats(unsigned long *taken, unsigned long *fell_back) {
  SHIM_CALL();
  if (taken) *taken = g_const_taken;
  if (fell_back) *fell_back = g_const_fell_back;
}

static bool mpi_is_zero(MPI m, bool direct) {
  const MpiView *v = (const MpiView *)m;
  if (direct && !(v->flags & 4)) {
    for (int j = 0; j < v->nlimbs; ++j) if (v->d[j]) return false;
    return true;
  }
  return G.mpi_cmp_ui(m, 0) == 0;
}
// A candidate in O(1): m[1] is zero and m[0], m[n/2] have at most 63 bits.  A dense plaintext leaves here, at its first look.
static bool const_pt_candidate(const poly_mpi_t *m, unsigned n, int64_t *a, int64_t *b) {
  if (n < 4 || !mpi_is_zero(m->coeffs[1], mpi_direct())) return false;
  int64_t v[2];
  for (int k = 0; k < 2; ++k) {
    MPI x = m->coeffs[k ? n / 2 : 0];
    const unsigned nb = G.mpi_get_nbits(x);
    if (nb > 63) return false;
    uint64_t mag = 0;
    if (nb) {
      unsigned char buf[8];
      size_t nw = 0;
      if (G.mpi_print(FMT_USG, buf, sizeof buf, &nw, x)) die("gcry_mpi_print failed");
      for (size_t i = 0; i < nw; ++i) mag = mag << 8 | buf[i];
    }
    v[k] = G.mpi_is_neg(x) ? -(int64_t)mag : (int64_t)mag;
  }
  *a = v[0]; *b = v[1];
  return true;
}
// The rest of the scan -- is every other coefficient zero? -- cut into the conversion threads' ranges; a range stops at the first non-zero
// coefficient anyone found.  The tasks ride with the conversions of the call (StagedCall's `side` tasks): when
// every operand is resident the device already works on the candidate's closed form while the host scans, as it does for the operands.
struct ConstScan {
  const poly_mpi_t *m;
  unsigned n, parts;
  bool direct;
  std::atomic<bool> dense{false};
  std::function<void(unsigned)> job;
  ConstScan(const poly_mpi_t *m_, unsigned n_) : m(m_), n(n_), parts(convert_threads(n_)), direct(mpi_direct()) {
    job = [this](unsigned t) {
      const unsigned per = (n + parts - 1) / parts, lo = t * per, hi = lo + per < n ? lo + per : n, h = n / 2;
      for (unsigned i = lo; i < hi && !dense.load(std::memory_order_relaxed); ++i)
        if (i != 0 && i != h && !mpi_is_zero(m->coeffs[i], direct)) dense.store(true, std::memory_order_relaxed);
    };
  }
};
static bool all_operands_resident(const poly_mpi_t *const in[], int count, unsigned n, unsigned W) {
  if (!poly_cache_on(n)) return false;
  for (int i = 0; i < count; ++i) {
    const PolySlot *s = resident_poly(in[i], n, W);
    if (!s || !s->trusted) return false;
  }
  return true;
}

// he_mulpt by a + b x^(n/2), q_l = 2^logql, on the ciphertext's two polynomials alone.  The caller's integers may be anything, and the closed
// form is he_mulpt's words for centred ones only: the kernel counts the others, the count comes back with the first bytes of the download,
// and a non-zero count leaves `dest` untouched (it may be `src`) and returns 0 -- the caller runs the dense path.  -1: the plaintext has
// another non-zero coefficient after all (nothing was written either); 1: done.
static int mulpt_const(gpq_ctx *c, struct he_ct *dest, const struct he_ct *src, const struct he_pt *pt, int64_t ca, int64_t cb, unsigned n, unsigned logql, unsigned dim) {
  static hipEvent_t counted = nullptr;
  if (!counted && hipEventCreateWithFlags(&counted, hipEventDisableTiming) != hipSuccess) die("hipEventCreate failed");
  const unsigned W = (logql + 1) / 64 + 1;
  HostBuf count(8);
  DevBuf bad(8);
  const poly_mpi_t *in[2] = {&src->c0, &src->c1};
  poly_mpi_t *out[2] = {&dest->c0, &dest->c1};
  ConstScan scan(&pt->m, n);
  StagedCall call(n, W, 2, in, 2);
  call.side_parts = scan.parts; call.side = &scan.job; call.abort = &scan.dense;
  call.side_later = all_operands_resident(in, 2, n, W);      // the scan rides with the check of the resident copies
  const StagedCall::Verdict v = call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
    if (hipMemsetAsync(bad.p, 0, 4, nullptr) != hipSuccess) die("device memset failed");
    if (gpq_he_mulpt_const(c, o[0], o[1], x[0], x[1], ca, cb, W, logql, dim, 0, 1, (unsigned *)bad.p, nullptr) != GPQ_OK) die("he_mulpt failed");
    if (hipMemcpyAsync(count.p, bad.p, 4, hipMemcpyDeviceToHost, nullptr) != hipSuccess || hipEventRecord(counted, nullptr) != hipSuccess) die("download failed");
  });
  if (v == StagedCall::Aborted) return -1;
  if (hipEventSynchronize(counted) != hipSuccess) die("download failed");
  if (*(volatile unsigned *)count.p) return 0;
  call.deliver(out);
  return 1;
}

// src/he-mult.c:159-196
void he_mulpt(struct he_ct *dest, const struct he_ct *src, const struct he_pt *pt) {
  SHIM_CALL();
  need_hectx();
  gpq_ctx *c = engine();
  const unsigned n = polyctx.n, l = src->l;
  const double nu = src->nu * pt->nu, B = src->B * pt->nu;                                      // :163-164
  const std::vector<uint64_t> qw = words_of(hectx.q[l], "he_mulpt: q_l must be positive");
  const bool pow2 = is_pow2(qw);
  const unsigned logql = G.mpi_get_nbits(hectx.q[l]) - 1;
  const unsigned dim = (unsigned)((logql + 1 + log2(pt->nu) + polyctx.logn) / 59u + 1);        // :169, evaluated in double as there
  int64_t ca, cb;
  if (g_const_pt_on && pow2 && logql >= 1 && const_pt_candidate(&pt->m, n, &ca, &cb) && gpq_he_mulpt_const_fits(c, ca, cb, logql, dim)) {
    const int took = mulpt_const(c, dest, src, pt, ca, cb, n, logql, dim);
    if (took >= 0) ++g_const_taken;
    if (took > 0) {
      dest->l = l; dest->nu = nu; dest->B = B;                                                  // :162-164
      return;
    }
    if (took == 0) ++g_const_fell_back;
  }
  unsigned bits = max_bits(&pt->m, n);
  if (logql + 1 > bits) bits = logql + 1;
  const unsigned W = bits / 64 + 1;
  DevBuf ws(gpq_he_mulpt_workspace_bytes(c, dim, 1) + gpq_poly_mul_general_workspace_bytes(c, dim, 1));
  const poly_mpi_t *in[3] = {&src->c0, &src->c1, &pt->m};
  poly_mpi_t *out[2] = {&dest->c0, &dest->c1};
  StagedCall call(n, W, 3, in, 2);
  call.run([&](const uint64_t *const x[], uint64_t *const o[]) {
    const int rc = pow2 ? gpq_he_mulpt(c, o[0], o[1], x[0], x[1], x[2], W, logql, dim, 1, ws.p, nullptr)
                        : gpq_he_mulpt_general(c, o[0], o[1], x[0], x[1], x[2], W, qw.data(), (unsigned)qw.size(), dim, 1, ws.p, nullptr);
    if (rc != GPQ_OK) die("he_mulpt failed");
  }, out);
  dest->l = l; dest->nu = nu; dest->B = B;                                                      // :162-164
}

#include "shim_additive.hpp"
#include "shim_keygen.hpp"
#include "shim_algo.hpp"
#include "shim_evaluators.hpp"

}  // extern "C"

#include "shim_chain.hpp"
