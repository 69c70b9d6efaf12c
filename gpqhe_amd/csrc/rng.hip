// rng.hip -- the reference's deterministic randombytes addressed by position (include/gpqhe_hip.h, "random bytes on the device"):
// gpq_surf_bytes (kernel: rng_kernels.hpp) and gpq_surf_bytes_host, the stream objects gpq_rng_*, and the process-wide default stream
// behind gpq_randombytes (include/gpqhe_hip_compat.h).  Nothing here invents entropy: a stream is a function of the caller's seed.
#include <hip/hip_runtime.h>
#include "../../include/gpqhe_hip.h"
#include "../../include/gpqhe_hip_compat.h"
#include "engine_internal.hpp"
#include "rng_kernels.hpp"

#include <cstring>
#include <mutex>
#include <new>

using namespace gpq;

struct gpq_rng {
  SurfSeed seed;
  U128 pos{0, 0};
  mutable std::mutex mu;                                   // tell is a const call
};

namespace {
// the reference's seed, src/rng.c:36-38 (the digits of pi: public test data, not entropy)
constexpr uint32_t kReferenceSeed[32] = {3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6, 2, 6, 4, 3, 3, 8, 3, 2, 7, 9, 5};
constexpr size_t kSplitDefault = (size_t)1 << 30;          // bytes of one launch: 2^18 workgroups of 4 KiB
size_t g_split = kSplitDefault;                           // a test hook (gpq_debug_rng_split): plain, unsynchronised -- set it while no call is in flight

void seed_of(SurfSeed &s, const uint32_t seed[32]) { memcpy(s.w, seed ? seed : kReferenceSeed, sizeof s.w); }
// pos + len <= 2^128: the slice exists
bool slice_fits(U128 pos, size_t len) {
  const U128 e = u128_add(pos, len);
  const bool carry = e.hi < pos.hi || (e.hi == pos.hi && e.lo < pos.lo);
  return !carry || (e.lo == 0 && e.hi == 0);
}
void host_bytes(uint8_t *x, size_t len, const SurfSeed &s, U128 pos) {
  U128 idx{(pos.lo >> 3) | (pos.hi << 61), pos.hi >> 3};
  unsigned r = (unsigned)(pos.lo & 7);
  while (len) {
    const uint64_t w = surf_block_at(s, idx);
    for (; r < 8 && len; ++r, --len) *x++ = (uint8_t)(w >> (8 * r));
    r = 0;
    idx = u128_add(idx, 1);
  }
}
int check_device(const gpq_ctx *c, const char *who) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "%s: null context", who);
  int dev = -1;
  if (hipGetDevice(&dev) == hipSuccess && dev != c->device)
    return gpq_fail(GPQ_ERR_INVALID, "%s: the context lives on device %d but the calling thread's current device is %d (gpq_set_device(gpq_ctx_device(ctx)) first)", who, c->device, dev);
  return GPQ_OK;
}
// the launches of one slice; everything was checked by the caller
int device_bytes(gpq_ctx *c, uint8_t *dst, size_t len, const SurfSeed &seed, U128 pos, hipStream_t s, const char *who) {
  while (len) {
    const size_t part = len < g_split ? len : g_split;
    SurfStreamArgs a;
    a.head = (uint32_t)((uintptr_t)dst & 15);
    a.base = dst - a.head;
    a.end = (uint64_t)a.head + part;
    a.start = U128{pos.lo - a.head, pos.hi - (pos.lo < a.head)};                  // mod 2^128
    a.seed = seed;
    const uint64_t blocks = (a.end + 4095) / 4096;
    {
      ProfScope prof(c, GPQ_K_RNG, s);
      hipLaunchKernelGGL(surf_stream_k, dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    dst += part; len -= part; pos = u128_add(pos, part);
  }
  return GPQ_OK;
}

gpq_rng &default_rng() {
  static gpq_rng *r = [] { gpq_rng *p = new gpq_rng; seed_of(p->seed, nullptr); return p; }();   // never destroyed: usable from any exit path
  return *r;
}
}  // namespace

extern "C" int gpq_surf_bytes_host(uint8_t *x, size_t len, const uint32_t seed[32], uint64_t pos_lo, uint64_t pos_hi) {
  const char *who = "gpq_surf_bytes_host";
  if (!x || !len) return gpq_fail(GPQ_ERR_INVALID, "%s: null pointer or len = 0", who);
  if (!slice_fits(U128{pos_lo, pos_hi}, len)) return gpq_fail(GPQ_ERR_INVALID, "%s: pos + len is beyond 2^128", who);
  SurfSeed s;
  seed_of(s, seed);
  host_bytes(x, len, s, U128{pos_lo, pos_hi});
  return GPQ_OK;
}

extern "C" int gpq_surf_bytes(gpq_ctx *c, uint8_t *bytes_dev, size_t len, const uint32_t seed[32], uint64_t pos_lo, uint64_t pos_hi, void *stream) {
  const char *who = "gpq_surf_bytes";
  int rc = check_device(c, who);
  if (rc) return rc;
  if (!bytes_dev || !len) return gpq_fail(GPQ_ERR_INVALID, "%s: null pointer or len = 0", who);
  if (!slice_fits(U128{pos_lo, pos_hi}, len)) return gpq_fail(GPQ_ERR_INVALID, "%s: pos + len is beyond 2^128", who);
  SurfSeed s;
  seed_of(s, seed);
  return device_bytes(c, bytes_dev, len, s, U128{pos_lo, pos_hi}, (hipStream_t)stream, who);
}

extern "C" int gpq_debug_rng_split(size_t bytes) {
  if (bytes % 16) return gpq_fail(GPQ_ERR_INVALID, "gpq_debug_rng_split: %zu bytes is no multiple of 16", bytes);
  g_split = bytes ? bytes : kSplitDefault;
  return GPQ_OK;
}

extern "C" int gpq_rng_create(gpq_rng **rng, const uint32_t seed[32]) {
  if (!rng) return gpq_fail(GPQ_ERR_INVALID, "gpq_rng_create: null pointer");
  gpq_rng *r = new (std::nothrow) gpq_rng;
  if (!r) return gpq_fail(GPQ_ERR_NOMEM, "gpq_rng_create: out of memory");
  seed_of(r->seed, seed);
  *rng = r;
  return GPQ_OK;
}
extern "C" void gpq_rng_destroy(gpq_rng *rng) { delete rng; }

extern "C" int gpq_rng_seek(gpq_rng *rng, uint64_t pos_lo, uint64_t pos_hi) {
  if (!rng) return gpq_fail(GPQ_ERR_INVALID, "gpq_rng_seek: null stream");
  std::lock_guard<std::mutex> lock(rng->mu);
  rng->pos = U128{pos_lo, pos_hi};
  return GPQ_OK;
}
extern "C" int gpq_rng_tell(const gpq_rng *rng, uint64_t pos[2]) {
  if (!rng || !pos) return gpq_fail(GPQ_ERR_INVALID, "gpq_rng_tell: null pointer");
  std::lock_guard<std::mutex> lock(rng->mu);
  pos[0] = rng->pos.lo; pos[1] = rng->pos.hi;
  return GPQ_OK;
}
extern "C" int gpq_rng_host_bytes(gpq_rng *rng, uint8_t *x, size_t len) {
  const char *who = "gpq_rng_host_bytes";
  if (!rng || !x || !len) return gpq_fail(GPQ_ERR_INVALID, "%s: null pointer or len = 0", who);
  std::lock_guard<std::mutex> lock(rng->mu);
  if (!slice_fits(rng->pos, len)) return gpq_fail(GPQ_ERR_INVALID, "%s: pos + len is beyond 2^128", who);
  host_bytes(x, len, rng->seed, rng->pos);
  rng->pos = u128_add(rng->pos, len);
  return GPQ_OK;
}
extern "C" int gpq_rng_device_bytes(gpq_ctx *c, gpq_rng *rng, uint8_t *bytes_dev, size_t len, void *stream) {
  const char *who = "gpq_rng_device_bytes";
  int rc = check_device(c, who);
  if (rc) return rc;
  if (!rng || !bytes_dev || !len) return gpq_fail(GPQ_ERR_INVALID, "%s: null pointer or len = 0", who);
  std::lock_guard<std::mutex> lock(rng->mu);
  if (!slice_fits(rng->pos, len)) return gpq_fail(GPQ_ERR_INVALID, "%s: pos + len is beyond 2^128", who);
  if ((rc = device_bytes(c, bytes_dev, len, rng->seed, rng->pos, (hipStream_t)stream, who))) return rc;
  rng->pos = u128_add(rng->pos, len);                                             // a reserved slice is spent once its launches are queued
  return GPQ_OK;
}

// ---- the process-wide default stream (include/gpqhe_hip_compat.h) ---------------------------------------------------------------------
extern "C" void gpq_randombytes(uint8_t *x, size_t xlen) {
  if (!x || !xlen) return;                                                        // src/rng.c:67: nothing to do
  gpq_rng &r = default_rng();
  std::lock_guard<std::mutex> lock(r.mu);
  host_bytes(x, xlen, r.seed, r.pos);                                             // a 128-bit position does not run out in practice: it wraps like the counter
  r.pos = u128_add(r.pos, xlen);
}
extern "C" int gpq_randombytes_seek(uint64_t pos_lo, uint64_t pos_hi) { return gpq_rng_seek(&default_rng(), pos_lo, pos_hi); }
extern "C" int gpq_randombytes_tell(uint64_t pos[2]) { return gpq_rng_tell(&default_rng(), pos); }
extern "C" int gpq_randombytes_seed(const uint32_t seed[32]) {
  gpq_rng &r = default_rng();
  std::lock_guard<std::mutex> lock(r.mu);
  seed_of(r.seed, seed);
  r.pos = U128{0, 0};
  return GPQ_OK;
}
extern "C" int gpq_randombytes_device(gpq_ctx *c, uint8_t *bytes_dev, size_t len, void *stream) {
  return gpq_rng_device_bytes(c, &default_rng(), bytes_dev, len, stream);
}
