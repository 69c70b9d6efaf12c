// enc.hip -- samplers and encryption on the device (include/gpqhe_hip.h): the Gaussian pair table, gpq_sample_zo / gpq_sample_error /
// gpq_sample_uniform / gpq_small_to_big (kernels: enc_kernels.hpp), and gpq_he_enc_pk / gpq_he_enc_sk, which are gpq_keyswitch resp.
// gpq_he_dec's product sequence followed by gpq_rns_reconstruct and enc_tail_k.
#include <hip/hip_runtime.h>
#include "../../include/gpqhe_hip.h"
#include "engine_internal.hpp"
#include "enc_kernels.hpp"

#include <cmath>
#include <vector>

using namespace gpq;

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr unsigned kMaxGridY = 65535;
constexpr size_t kMaxGridX = 0x7fffffff;                   // blocks of one launch: a larger count is refused, never truncated

int on_device(const gpq_ctx *c, const char *who) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "%s: null context", who);
  int dev = -1;
  if (hipGetDevice(&dev) == hipSuccess && dev != c->device)
    return gpq_fail(GPQ_ERR_INVALID, "%s: the context lives on device %d but the calling thread's current device is %d (gpq_set_device(gpq_ctx_device(ctx)) first)", who, c->device, dev);
  return GPQ_OK;
}
int launched(const char *who) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GPQ_OK : gpq_fail(GPQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}
bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const char *x = (const char *)a, *y = (const char *)b;
  return a && b && x < y + nb && y < x + na;
}
// the table on the device, built and uploaded at first use (synchronous, like every other constant of the cache: outside a stream capture)
int error_table(gpq_ctx *c, const uint16_t **out) {
  if (!c->cache) return gpq_fail(GPQ_ERR_INVALID, "gpq_sample_error: the context has no table cache");
  if (!c->cache->d_error_table) {
    std::vector<int8_t> T(2 * 65536);
    int rc = gpq_sample_error_table(T.data());
    if (rc) return rc;
    if ((rc = c->cache->d_error_table.upload(c, T))) return rc;
  }
  *out = c->cache->d_error_table;
  return GPQ_OK;
}
int small_to_rns(gpq_ctx *c, uint64_t *slab, const int8_t *small, unsigned dim, unsigned batch, hipStream_t s) {
  ProfScope prof(c, GPQ_K_ENC, s);
  SmallToRnsArgs a{small, slab, c->d_tabs, dim, c->logn};
  hipLaunchKernelGGL(small_to_rns_k, dim3((c->n + 255) / 256, batch), dim3(256), 0, s, a);
  return launched("small_to_rns_k");
}
int enc_tail(gpq_ctx *c, uint64_t *out, const uint64_t *x, const uint64_t *m, const int8_t *e, unsigned W, unsigned logq, bool negate, unsigned batch,
             hipStream_t s) {
  ProfScope prof(c, GPQ_K_ENC, s);
  EncTailArgs a{out, x, m, e, W, c->logn, logq, negate ? 1u : 0u};
  hipLaunchKernelGGL(enc_tail_k, dim3((c->n + 255) / 256, batch), dim3(256), 0, s, a);
  return launched("enc_tail_k");
}
// what gpq_he_enc_pk / gpq_he_enc_sk refuse alike
int enc_check(const gpq_ctx *c, unsigned W, unsigned logq, unsigned dim, unsigned batch, const char *who) {
  int rc = on_device(c, who);
  if (rc) return rc;
  if (dim < 1 || dim > c->nprimes) return gpq_fail(GPQ_ERR_INVALID, "%s: dim=%u outside 1..%u", who, dim, c->nprimes);
  if (batch < 1 || batch > kMaxGridY) return gpq_fail(GPQ_ERR_INVALID, "%s: batch = %u outside 1..%u", who, batch, kMaxGridY);
  if (!logq) return gpq_fail(GPQ_ERR_INVALID, "%s: q must be 2^logq with logq > 0", who);
  if (W < 1 || W > 32 || 64ull * W <= logq) return gpq_fail(GPQ_ERR_INVALID, "%s: W = %u words: 1..32 and 64 W > logq = %u", who, W, logq);
  return GPQ_OK;
}
}  // namespace

// T[b0][b1] of src/sample.c:64-71 for every byte pair; (0, 0) where b1 = 0 (log 0 = -inf: the conversion is undefined in C, the
// reference on x86-64 stores 0).  The argument of floor stays 5e-5 away from every integer, so the entries do not depend on the libm.
extern "C" int gpq_sample_error_table(int8_t *table) {
  if (!table) return gpq_fail(GPQ_ERR_INVALID, "gpq_sample_error_table: null table");
  const double PI = 3.141592653589793238462643383279502884, SIGMA = 3.1915382432114616;   // src/params.h:52, :55
  for (unsigned b0 = 0; b0 < 256; ++b0) {
    const double theta = 2 * PI * ((double)b0 / 256);
    const double cs = std::cos(theta), sn = std::sin(theta);
    table[2 * (b0 * 256)] = table[2 * (b0 * 256) + 1] = 0;
    for (unsigned b1 = 1; b1 < 256; ++b1) {
      const double rr = std::sqrt(-2 * std::log((double)b1 / 256)) * SIGMA;
      table[2 * (b0 * 256 + b1)] = (int8_t)(int16_t)std::floor(rr * cs + 0.5);
      table[2 * (b0 * 256 + b1) + 1] = (int8_t)(int16_t)std::floor(rr * sn + 0.5);
    }
  }
  return GPQ_OK;
}

extern "C" int gpq_sample_zo(gpq_ctx *c, int8_t *out, const uint8_t *bytes_dev, unsigned count, void *stream) {
  const char *who = "gpq_sample_zo";
  int rc = on_device(c, who);
  if (rc) return rc;
  if (!out || !bytes_dev || !count) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument or count = 0", who);
  if (c->logn < 2) return gpq_fail(GPQ_ERR_INVALID, "%s: n/4 bytes per polynomial need logn >= 2", who);
  const size_t nbytes = (size_t)count * (c->n / 4);
  if (overlap(out, 4 * nbytes, bytes_dev, nbytes)) return gpq_fail(GPQ_ERR_INVALID, "%s: the output overlaps the input", who);
  const size_t threads = ((uintptr_t)out & 15) ? nbytes : nbytes / 4 + nbytes % 4;
  if ((threads + 255) / 256 > kMaxGridX) return gpq_fail(GPQ_ERR_INVALID, "%s: count = %u is more than one launch covers", who, count);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(c, GPQ_K_SAMPLE, s);
  SampleZoArgs a{bytes_dev, out, nbytes};
  hipLaunchKernelGGL(sample_zo_k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return launched(who);
}

extern "C" int gpq_sample_error(gpq_ctx *c, int8_t *out, const uint8_t *bytes_dev, unsigned count, void *stream) {
  const char *who = "gpq_sample_error";
  int rc = on_device(c, who);
  if (rc) return rc;
  if (!out || !bytes_dev || !count) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument or count = 0", who);
  if (c->logn < 1) return gpq_fail(GPQ_ERR_INVALID, "%s: coefficients come in pairs: logn >= 1", who);
  const size_t nbytes = (size_t)count * c->n;
  if (overlap(out, nbytes, bytes_dev, nbytes)) return gpq_fail(GPQ_ERR_INVALID, "%s: the output overlaps the input", who);
  const uint16_t *table = nullptr;
  if ((rc = error_table(c, &table))) return rc;
  const size_t threads = ((uintptr_t)out & 15) ? nbytes / 2 : nbytes / 16 + (nbytes % 16) / 2;
  if ((threads + 255) / 256 > kMaxGridX) return gpq_fail(GPQ_ERR_INVALID, "%s: count = %u is more than one launch covers", who, count);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(c, GPQ_K_SAMPLE, s);
  SampleErrorArgs a{bytes_dev, out, table, nbytes};
  hipLaunchKernelGGL(sample_error_k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return launched(who);
}

extern "C" int gpq_sample_uniform(gpq_ctx *c, uint64_t *big, const uint8_t *bytes_dev, unsigned nbits, unsigned W, unsigned count, void *stream) {
  const char *who = "gpq_sample_uniform";
  int rc = on_device(c, who);
  if (rc) return rc;
  if (!big || !bytes_dev || !count) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument or count = 0", who);
  if (!nbits) return gpq_fail(GPQ_ERR_INVALID, "%s: nbits = 0", who);
  if (W < 1 || W > 32 || 64ull * W <= nbits) return gpq_fail(GPQ_ERR_INVALID, "%s: W = %u words: 1..32 and 64 W > nbits = %u", who, W, nbits);
  const unsigned nb = nbits / 8 + 1;                                                   // src/sample.c:137
  const size_t ncoef = (size_t)count << c->logn;
  if (overlap(big, ncoef * W * 8, bytes_dev, ncoef * nb)) return gpq_fail(GPQ_ERR_INVALID, "%s: the output overlaps the input", who);
  if ((ncoef + kUniformTile - 1) / kUniformTile > kMaxGridX) return gpq_fail(GPQ_ERR_INVALID, "%s: count = %u is more than one launch covers", who, count);
  unsigned stride = (nb + 7) & ~7u;
  if (!((stride / 8) & 1)) stride += 8;
  SampleUniformArgs a{bytes_dev, big, ncoef, nbits, nb, W, c->logn, stride, nb > 1 ? (unsigned)((0x100000000ull + nb - 1) / nb) : 0u};
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(c, GPQ_K_SAMPLE, s);
  hipLaunchKernelGGL(sample_uniform_k, dim3((unsigned)((ncoef + kUniformTile - 1) / kUniformTile)), dim3(256), (size_t)kUniformTile * stride, s, a);
  return launched(who);
}

extern "C" int gpq_small_to_big(gpq_ctx *c, uint64_t *big, const int8_t *small, unsigned W, unsigned count, void *stream) {
  const char *who = "gpq_small_to_big";
  int rc = on_device(c, who);
  if (rc) return rc;
  if (!big || !small || !count || count > kMaxGridY) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument, or count = %u outside 1..%u", who, count, kMaxGridY);
  if (W < 1 || W > 32) return gpq_fail(GPQ_ERR_INVALID, "%s: W = %u outside 1..32", who, W);
  const size_t ncoef = (size_t)count << c->logn;
  if (overlap(big, ncoef * W * 8, small, ncoef)) return gpq_fail(GPQ_ERR_INVALID, "%s: the output overlaps the input", who);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(c, GPQ_K_ENC, s);
  SmallToBigArgs a{small, big, W, c->logn};
  hipLaunchKernelGGL(small_to_big_k, dim3((c->n + 255) / 256, count), dim3(256), 0, s, a);
  return launched(who);
}

extern "C" size_t gpq_he_enc_workspace_bytes(const gpq_ctx *c, unsigned dim, unsigned batch, int pk) {
  if (!c || !dim || !batch) return 0;
  const size_t slab = (size_t)batch * ((size_t)dim << c->logn) * 8;
  return pk ? 3 * slab + gpq_keyswitch_workspace_bytes(c, dim, batch) : slab;      // v's limbs, c0hat, c1hat, the key switch's own | a's limbs
}

// he_enc_pk, src/he-encrypt.c:37-73, q = 2^logq: v is transformed once for both products -- gpq_keyswitch with x = v's limbs and the key pair
extern "C" int gpq_he_enc_pk(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *m, const int8_t *v, const int8_t *e0, const int8_t *e1,
                             const uint64_t *pk0_ntt, const uint64_t *pk1_ntt, unsigned W, unsigned logq, unsigned dim, unsigned batch,
                             void *workspace, void *stream) {
  const char *who = "gpq_he_enc_pk";
  int rc = enc_check(c, W, logq, dim, batch, who);
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !v || !e0 || !e1 || !pk0_ntt || !pk1_ntt || !workspace) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument", who);
  const size_t big = (size_t)batch * W * c->n * 8, small = (size_t)batch * c->n, key = ((size_t)dim << c->logn) * 8;
  for (uint64_t *o : {out_c0, out_c1})
    if (overlap(o, big, m, big) || overlap(o, big, v, small) || overlap(o, big, e0, small) || overlap(o, big, e1, small) || overlap(o, big, pk0_ntt, key) ||
        overlap(o, big, pk1_ntt, key))
      return gpq_fail(GPQ_ERR_INVALID, "%s: an output overlaps an input", who);
  if (overlap(out_c0, big, out_c1, big)) return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs overlap", who);
  const size_t wsb = gpq_he_enc_workspace_bytes(c, dim, batch, 1);
  for (const void *o : {(const void *)out_c0, (const void *)out_c1, (const void *)m})
    if (overlap(workspace, wsb, o, big)) return gpq_fail(GPQ_ERR_INVALID, "%s: the workspace overlaps an output or the plaintext", who);
  StageRange stage(who);
  hipStream_t s = (hipStream_t)stream;
  const size_t slab = (size_t)batch * ((size_t)dim << c->logn);
  uint64_t *vhat = (uint64_t *)workspace, *c0hat = vhat + slab, *c1hat = c0hat + slab;
  if ((rc = small_to_rns(c, vhat, v, dim, batch, s))) return rc;                                                  // rns_decompose(v), src/poly.c:94
  if ((rc = gpq_keyswitch(c, c0hat, c1hat, vhat, pk0_ntt, pk1_ntt, dim, batch, c1hat + slab, stream))) return rc;   // :58-59 up to poly_rns2mpi
  if ((rc = gpq_rns_reconstruct(c, out_c0, W, c0hat, dim, batch, logq, stream))) return rc;
  if ((rc = gpq_rns_reconstruct(c, out_c1, W, c1hat, dim, batch, logq, stream))) return rc;
  if ((rc = enc_tail(c, out_c0, out_c0, m, e0, W, logq, false, batch, s))) return rc;                              // :61-62, :64
  return enc_tail(c, out_c1, out_c1, nullptr, e1, W, logq, false, batch, s);                                       // :63, :65
}

// he_enc_sk, src/he-encrypt.c:75-103, and with m == NULL he_keypair's pk.p0 / pk.p1, src/he-kem.c:59-65: the RAW sample `a` is multiplied
// (:91) and centred afterwards (:97) -- gpq_he_dec's product sequence on it
extern "C" int gpq_he_enc_sk(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *m, const uint64_t *a, const int8_t *e,
                             const uint64_t *sk_ntt, unsigned W, unsigned logq, unsigned dim, unsigned batch, void *workspace, void *stream) {
  const char *who = "gpq_he_enc_sk";
  int rc = enc_check(c, W, logq, dim, batch, who);
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !a || !e || !sk_ntt || !workspace) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument", who);
  if (64ull * W <= logq + 1) return gpq_fail(GPQ_ERR_INVALID, "%s: the raw sample has logq + 1 = %u bits and must stay non-negative in %u words (64 W > logq + 1)", who, logq + 1, W);
  const size_t big = (size_t)batch * W * c->n * 8, small = (size_t)batch * c->n, key = ((size_t)dim << c->logn) * 8;
  for (uint64_t *o : {out_c0, out_c1})
    if (overlap(o, big, m, big) || overlap(o, big, a, big) || overlap(o, big, e, small) || overlap(o, big, sk_ntt, key))
      return gpq_fail(GPQ_ERR_INVALID, "%s: an output overlaps an input", who);
  if (overlap(out_c0, big, out_c1, big)) return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs overlap", who);
  const size_t wsb = gpq_he_enc_workspace_bytes(c, dim, batch, 0);
  for (const void *o : {(const void *)out_c0, (const void *)out_c1, (const void *)m, (const void *)a})
    if (overlap(workspace, wsb, o, big)) return gpq_fail(GPQ_ERR_INVALID, "%s: the workspace overlaps an output, the plaintext or the sample", who);
  StageRange stage(who);
  hipStream_t s = (hipStream_t)stream;
  uint64_t *x = (uint64_t *)workspace;
  if ((rc = gpq_rns_decompose(c, x, a, W, dim, batch, stream))) return rc;                 // src/poly.c:96-103 with the key's limbs already transformed
  if ((rc = gpq_ntt(c, x, dim, batch, stream))) return rc;
  if ((rc = gpq_rns_mul_shared(c, x, x, sk_ntt, dim, batch, s))) return rc;
  if ((rc = gpq_invntt(c, x, dim, batch, stream))) return rc;
  if ((rc = gpq_rns_reconstruct(c, out_c0, W, x, dim, batch, logq, stream))) return rc;
  if ((rc = enc_tail(c, out_c0, out_c0, m, e, W, logq, true, batch, s))) return rc;        // src/he-encrypt.c:93-96
  return enc_tail(c, out_c1, a, nullptr, nullptr, W, logq, false, batch, s);               // :97
}
