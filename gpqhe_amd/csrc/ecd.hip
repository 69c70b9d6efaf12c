// ecd.hip -- the encoder on the device (include/gpqhe_hip.h, "he_ecd"): the root table, the per-slot-count plan, gpq_he_ecd /
// gpq_he_ecd_diagonals (kernel: ecd_kernels.hpp) and gpq_gemv_plan_create_from_matrix, which encodes a matrix's diagonals into a one-word
// slab and hands it to gpq_gemv_plan_create; and the decoder, gpq_he_dcd (kernel: dcd_kernels.hpp), on the same plan.
#include <hip/hip_runtime.h>
#include "../../include/gpqhe_hip.h"
#include "engine_internal.hpp"
#include "ecd_kernels.hpp"
#include "dcd_kernels.hpp"

#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <vector>

using namespace gpq;

static_assert(GPQ_ECD_MAX_BLOCK_SLOTS == kEcdMaxSlots && GPQ_ECD_MAX_SLOTS == (kEcdMaxSlots << kEcdMaxSplit), "include/gpqhe_hip.h states the kernels' limits");

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct gpq_ecd_plan {
  gpq_ctx *ctx = nullptr;
  unsigned slots = 0, logslots = 0;
  unsigned logblock = 0;           // B = 2^logblock slots per workgroup; < logslots: the two-pass kernels (gpq_ecd_plan_set_block)
  gpq_dev<double2> d_roots;        // T[0 .. 4 slots]
  gpq_dev<uint32_t> d_pow5;        // 5^j mod 4 slots
  gpq_dev<uint32_t> d_bad;         // gpq_gemv_plan_create_from_matrix's own counter ...
  uint32_t *h_bad = nullptr;       // ... and the page-locked word it is read through
};

namespace {
bool pow2(unsigned v) { return v && !(v & (v - 1)); }
unsigned log2u(unsigned v) { unsigned b = 0; while ((1u << b) < v) ++b; return b; }
bool block_fits(unsigned slots, unsigned block) {             // gpq_ecd_plan_set_block's rule for a non-zero block
  return pow2(block) && block >= 2 && block <= slots && block <= gpq::kEcdMaxSlots && slots / block <= (1u << gpq::kEcdMaxSplit);
}
void gemv_split(unsigned slots, unsigned *n1) {               // src/he-algo.c:51-54
  unsigned a = (unsigned)std::sqrt((double)slots);
  if (slots != a * a) a = (unsigned)std::sqrt((double)(2 * slots));
  *n1 = a;
}

int encode(gpq_ctx *c, const gpq_ecd_plan *p, uint64_t *out, const double *src, unsigned logDelta, unsigned W, unsigned count, unsigned n1,
           uint32_t *bad, void *stream, const char *who) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "%s: null context", who);
  if (!p || p->ctx != c) return gpq_fail(GPQ_ERR_INVALID, "%s: no plan, or a plan of another context", who);
  if (!out || !src || !count) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument or empty batch", who);
  if (W < 1 || W > 32) return gpq_fail(GPQ_ERR_INVALID, "%s: W = %u outside 1..32", who, W);
  if (logDelta > 63) return gpq_fail(GPQ_ERR_INVALID, "%s: Delta = 2^%u is not a 64-bit Delta (src/gpqhe.h:100)", who, logDelta);
  int dev = -1;
  if (hipGetDevice(&dev) == hipSuccess && dev != c->device)
    return gpq_fail(GPQ_ERR_INVALID, "%s: the context lives on device %d but the calling thread's current device is %d (gpq_set_device(gpq_ctx_device(ctx)) first)", who, c->device, dev);
  EcdArgs a{src, out, p->d_roots, p->d_pow5, bad, std::ldexp(1.0, (int)logDelta), 1.0 / p->slots, p->slots, p->logslots, c->logn, W, n1,
            p->logblock, nullptr, nullptr};
  hipStream_t s = (hipStream_t)stream;
  if (p->logblock < p->logslots) {
    // slots = 2^k B: columns, blocks, slab (ecd_kernels.hpp); 32 slots bytes of hand-off memory per vector, the context's
    if ((uintptr_t)out & 15) return gpq_fail(GPQ_ERR_INVALID, "%s: out must be 16-byte aligned for a plan of more than one block", who);
    const size_t per = (size_t)p->slots * 16, need = 2 * per * count;
    if (need > c->d_ecd_hand.bytes)
      if (int rc = c->d_ecd_hand.grow(c, s, need, false, "the first gpq_he_ecd of a larger batch of more than one block allocates its hand-off memory: run it once outside stream capture")) return rc;
    a.hand = (double2 *)c->d_ecd_hand.p;
    a.ints = (long long *)((char *)c->d_ecd_hand.p + per * count);
    const unsigned B = 1u << p->logblock, blocks = p->slots >> p->logblock, col_tiles = (B + kEcdColThreads - 1) / kEcdColThreads;
    const unsigned slab_tiles = (c->n / 2 + kEcdSlabThreads - 1) / kEcdSlabThreads;
    ProfScope prof(c, GPQ_K_ECD, s);
    switch (p->logslots - p->logblock) {
      case 1: hipLaunchKernelGGL(he_ecd_cols<1>, dim3(count, col_tiles), dim3(kEcdColThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL(he_ecd_cols<2>, dim3(count, col_tiles), dim3(kEcdColThreads), 0, s, a); break;
      default: hipLaunchKernelGGL(he_ecd_cols<3>, dim3(count, col_tiles), dim3(kEcdColThreads), 0, s, a); break;
    }
    if (int rc = gpq_launch_lds<&he_ecd_block>((int)(kEcdMaxSlots * 16), dim3(count, blocks), dim3(B / 2 >= kEcdMaxThreads ? kEcdMaxThreads : 256u), (size_t)B * 16, s, a)) return rc;
    hipLaunchKernelGGL(he_ecd_slab, dim3(count, slab_tiles), dim3(kEcdSlabThreads), 0, s, a);
  } else {
    const size_t lds = (size_t)p->slots * 16;                              // above 64 KB for many slots: gpq_launch_lds
    const unsigned threads = (p->slots / 2 >= kEcdMaxThreads || ((size_t)W << c->logn) >= 8192) ? kEcdMaxThreads : 256u;
    ProfScope prof(c, GPQ_K_ECD, s);
    if (int rc = gpq_launch_lds<&he_ecd_lds>((int)(kEcdMaxSlots * 16), dim3(count), dim3(threads), lds, s, a)) return rc;
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GPQ_OK : gpq_fail(GPQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}
}  // namespace

extern "C" int gpq_ecd_roots(double *table, unsigned slots) {
  if (!table || !pow2(slots) || slots > (1u << 28)) return gpq_fail(GPQ_ERR_INVALID, "gpq_ecd_roots: slots = %u must be a power of two", slots);
  const unsigned m4 = 4 * slots;
  for (unsigned t = 0; t < m4; ++t) {
    const double theta = 2 * 3.141592653589793238462643383279502884 * t / m4;     // src/precomp.c:307, src/params.h:52
    double sn, cs;
    sincos(theta, &sn, &cs);                                                       // what gcc -O2 makes of :308
    table[2 * t] = cs; table[2 * t + 1] = sn;
  }
  table[2 * m4] = table[0]; table[2 * m4 + 1] = table[1];                           // :310
  return GPQ_OK;
}

extern "C" void gpq_ecd_plan_destroy(gpq_ecd_plan *p) {
  if (!p) return;
  DeviceScope on_device(p->ctx->device);
  if (p->h_bad) (void)hipHostFree(p->h_bad);
  delete p;
}

// one body for gpq_ecd_plan_create (most = what one workgroup holds) and gpq_ecd_plan_create_split (most = kEcdMaxSlots << kEcdMaxSplit)
static int plan_create(gpq_ctx *c, gpq_ecd_plan **out, unsigned slots, const double *roots, unsigned roots_slots, unsigned most, const char *who) {
  if (!c || !out) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument", who);
  if (!pow2(slots) || slots > c->n / 2)
    return gpq_fail(GPQ_ERR_INVALID, "%s: slots = %u must be a power of two up to n/2 = %u", who, slots, c->n / 2);
  if (slots > most)
    return gpq_fail(GPQ_ERR_INVALID, "%s: %u slots exceed the %u that %u workgroup(s) hold in LDS", who, slots, most, most / kEcdMaxSlots);
  if (roots && (!pow2(roots_slots) || roots_slots < slots))
    return gpq_fail(GPQ_ERR_INVALID, "%s: the root table is for %u slots: a power of two >= %u is needed", who, roots_slots, slots);
  const unsigned m4 = 4 * slots;
  std::vector<double> T(2 * (size_t)(m4 + 1));
  if (roots) {
    const size_t stride = roots_slots / slots;
    for (unsigned t = 0; t <= m4; ++t) { T[2 * t] = roots[2 * t * stride]; T[2 * t + 1] = roots[2 * t * stride + 1]; }
  } else {
    int rc = gpq_ecd_roots(T.data(), slots);
    if (rc) return rc;
  }
  std::vector<uint32_t> pow5(slots / 2 ? slots / 2 : 1);
  uint32_t g = 1;
  for (uint32_t &v : pow5) { v = g; g = (uint32_t)((5ull * g) % m4); }
  std::unique_ptr<gpq_ecd_plan, void (*)(gpq_ecd_plan *)> p(new (std::nothrow) gpq_ecd_plan(), gpq_ecd_plan_destroy);
  if (!p) return gpq_fail(GPQ_ERR_NOMEM, "%s: out of host memory", who);
  p->ctx = c; p->slots = slots; p->logslots = log2u(slots);
  p->logblock = log2u(slots < kEcdMaxSlots ? slots : kEcdMaxSlots);
  DeviceScope on_device(c->device);
  HIP_TRY(p->d_roots.alloc(T.size() * sizeof(double)));
  HIP_TRY(p->d_pow5.alloc(pow5.size() * sizeof(uint32_t)));
  HIP_TRY(p->d_bad.alloc(sizeof(uint32_t)));
  HIP_TRY(hipHostMalloc((void **)&p->h_bad, sizeof(uint32_t), hipHostMallocDefault));
  HIP_TRY(hipMemcpy(p->d_roots, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_pow5, pow5.data(), pow5.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  *out = p.release();
  return GPQ_OK;
}

extern "C" int gpq_ecd_plan_create(gpq_ctx *c, gpq_ecd_plan **out, unsigned slots, const double *roots, unsigned roots_slots) {
  return plan_create(c, out, slots, roots, roots_slots, kEcdMaxSlots, "gpq_ecd_plan_create");
}

extern "C" int gpq_ecd_plan_create_split(gpq_ctx *c, gpq_ecd_plan **out, unsigned slots, unsigned block_slots, const double *roots, unsigned roots_slots) {
  if (block_slots && pow2(slots) && !block_fits(slots, block_slots))           // before anything is allocated
    return gpq_fail(GPQ_ERR_INVALID, "gpq_ecd_plan_create_split: %u is no power of two in 2..min(slots, %u) with at most %u blocks in %u slots", block_slots, kEcdMaxSlots, 1u << kEcdMaxSplit, slots);
  gpq_ecd_plan *p = nullptr;
  int rc = plan_create(c, &p, slots, roots, roots_slots, kEcdMaxSlots << kEcdMaxSplit, "gpq_ecd_plan_create_split");
  if (rc != GPQ_OK) return rc;
  if (block_slots) p->logblock = log2u(block_slots);
  *out = p;
  return GPQ_OK;
}

extern "C" int gpq_ecd_plan_set_block(gpq_ecd_plan *p, unsigned block_slots) {
  if (!p) return gpq_fail(GPQ_ERR_INVALID, "gpq_ecd_plan_set_block: no plan");
  const unsigned most = p->slots < kEcdMaxSlots ? p->slots : kEcdMaxSlots;
  if (!block_slots) { p->logblock = log2u(most); return GPQ_OK; }
  if (!block_fits(p->slots, block_slots))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_ecd_plan_set_block: %u is no power of two in 2..%u with at most %u blocks in %u slots", block_slots, most, 1u << kEcdMaxSplit, p->slots);
  p->logblock = log2u(block_slots);
  return GPQ_OK;
}

extern "C" int gpq_he_ecd(gpq_ctx *c, const gpq_ecd_plan *p, uint64_t *out, const double *z_dev, unsigned logDelta, unsigned W, unsigned count,
                          uint32_t *bad_dev, void *stream) {
  return encode(c, p, out, z_dev, logDelta, W, count, 0, bad_dev, stream, "gpq_he_ecd");
}

extern "C" int gpq_he_ecd_diagonals(gpq_ctx *c, const gpq_ecd_plan *p, uint64_t *out, const double *A_dev, unsigned logDelta, unsigned W,
                                    uint32_t *bad_dev, void *stream) {
  unsigned n1 = 1;
  if (p && p->slots > kEcdMaxSlots) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_ecd_diagonals: a %u x %u matrix (a plan above %u slots) is not taken", p->slots, p->slots, kEcdMaxSlots);
  if (p) gemv_split(p->slots, &n1);
  return encode(c, p, out, A_dev, logDelta, W, p ? p->slots : 1, n1, bad_dev, stream, "gpq_he_ecd_diagonals");
}

// he_dcd, src/he-encode.c:66-74 and :114-117: `count` plaintext big slabs -> [count][slots] (re, im) pairs
extern "C" int gpq_he_dcd(gpq_ctx *c, const gpq_ecd_plan *p, double *z_dev, const uint64_t *in, double nu, unsigned W, unsigned count, void *stream) {
  const char *who = "gpq_he_dcd";
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "%s: null context", who);
  if (!p || p->ctx != c) return gpq_fail(GPQ_ERR_INVALID, "%s: no plan, or a plan of another context", who);
  if (!z_dev || !in || !count) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument or empty batch", who);
  if (W < 1 || W > 32) return gpq_fail(GPQ_ERR_INVALID, "%s: W = %u outside 1..32", who, W);
  if (!std::isfinite(nu) || !(nu > 0)) return gpq_fail(GPQ_ERR_INVALID, "%s: nu = %g must be a finite double above 0", who, nu);
  int dev = -1;
  if (hipGetDevice(&dev) == hipSuccess && dev != c->device)
    return gpq_fail(GPQ_ERR_INVALID, "%s: the context lives on device %d but the calling thread's current device is %d (gpq_set_device(gpq_ctx_device(ctx)) first)", who, c->device, dev);
  DcdArgs a{in, z_dev, p->d_roots, p->d_pow5, nu, p->slots, p->logslots, c->logn, W, p->logblock};
  hipStream_t s = (hipStream_t)stream;
  if (p->logblock < p->logslots) {
    // slots = 2^k B: blocks into z_dev, then columns in place on it (dcd_kernels.hpp): no scratch
    if ((uintptr_t)z_dev & 15) return gpq_fail(GPQ_ERR_INVALID, "%s: z_dev must be 16-byte aligned", who);
    const unsigned B = 1u << p->logblock, blocks = p->slots >> p->logblock, col_tiles = (B + kEcdColThreads - 1) / kEcdColThreads;
    ProfScope prof(c, GPQ_K_DCD, s);
    if (int rc = gpq_launch_lds<&he_dcd_block>((int)(kEcdMaxSlots * 16), dim3(count, blocks), dim3(B >= kEcdMaxThreads ? kEcdMaxThreads : 256u), (size_t)B * 16, s, a)) return rc;
    switch (p->logslots - p->logblock) {
      case 1: hipLaunchKernelGGL(he_dcd_cols<1>, dim3(count, col_tiles), dim3(kEcdColThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL(he_dcd_cols<2>, dim3(count, col_tiles), dim3(kEcdColThreads), 0, s, a); break;
      default: hipLaunchKernelGGL(he_dcd_cols<3>, dim3(count, col_tiles), dim3(kEcdColThreads), 0, s, a); break;
    }
  } else {
    const size_t lds = (size_t)p->slots * 16;                              // (the attribute is per kernel function: he_ecd_lds having it does not serve)
    const unsigned threads = p->slots >= kEcdMaxThreads ? kEcdMaxThreads : 256u;     // 2 slots conversions, slots / 2 butterflies per stage
    ProfScope prof(c, GPQ_K_DCD, s);
    if (int rc = gpq_launch_lds<&he_dcd_lds>((int)(kEcdMaxSlots * 16), dim3(count), dim3(threads), lds, s, a)) return rc;
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GPQ_OK : gpq_fail(GPQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

extern "C" int gpq_gemv_plan_create_from_matrix(gpq_ctx *c, gpq_gemv_plan **out, const gpq_ecd_plan *p, const double *A_dev, unsigned logDelta,
                                                unsigned logql, unsigned dimpt, void *stream) {
  if (!c || !out || !p || p->ctx != c || !A_dev) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_create_from_matrix: null argument, or a plan of another context");
  if (p->slots > kEcdMaxSlots) return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_create_from_matrix: a %u x %u matrix (a plan above %u slots) is not taken", p->slots, p->slots, kEcdMaxSlots);
  hipStream_t s = (hipStream_t)stream;
  if (gpq_capturing(s))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_create_from_matrix allocates and waits for the stream: not inside a stream capture");
  // one word per coefficient: every encodable value fits (|v| < 2^63), 8 n bytes per diagonal
  gpq_dev<uint64_t> slab;                                     // (its hipFree waits for the transforms that read it)
  const size_t bytes = (size_t)p->slots * c->n * 8;
  if (slab.alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return gpq_fail(GPQ_ERR_NOMEM, "gpq_gemv_plan_create_from_matrix: no room for %zu bytes of encoded diagonals", bytes);
  }
  *p->h_bad = 0;
  HIP_TRY(hipMemsetAsync(p->d_bad, 0, sizeof(uint32_t), s));
  int rc = gpq_he_ecd_diagonals(c, p, slab, A_dev, logDelta, 1, p->d_bad, stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(p->h_bad, p->d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));   // arrives with gpq_gemv_plan_create's own wait
  gpq_gemv_plan *made = nullptr;
  if ((rc = gpq_gemv_plan_create(c, &made, slab, p->slots, 1, logql, dimpt, stream))) return rc;
  if (*p->h_bad) {
    gpq_gemv_plan_destroy(made);
    return gpq_fail(GPQ_ERR_INVALID, "gpq_gemv_plan_create_from_matrix: %u coefficients of the encoded diagonals are not finite or reach 2^63", *p->h_bad);
  }
  *out = made;
  return GPQ_OK;
}
