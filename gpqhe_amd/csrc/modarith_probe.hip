// modarith_probe.hip -- libgpqhe_modprobe.so: every inline device primitive of modarith.hpp (and gs_last / TwTraits / ref_fqmul of
// ntt_kernels.hpp, horner59 of bridge_kernels.hpp) callable on its own, one call per lane, for tests/test_modarith_device_gpu.py.
// The primitives are the product's: this file includes the headers and copies nothing.  One op per distinct instantiation the
// product compiles.  No domain checks here: the test owns the domains (tests/modarith_cases.py) and never leaves them.
// A library of its own so that libgpqhe_hip.so's export list stays what include/gpqhe_hip.h says.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "modarith.hpp"
#include "tables.hpp"
#include "ntt_kernels.hpp"
#include "bridge_kernels.hpp"

using namespace gpq;

namespace {

// OP(identifier, name as the test's table spells it, results written (1 or 2), statements)
// In scope: x, y (operands), w0, w1 (the multiplier w, or the pair X, Y), ws / ww (the pair as TwS / TwW), tab (a LimbTab whose
// last-stage constants are ninv = w0, winv1_ninv = w1 and whose split constants are both the pair), k; results go to r0, r1.
#define GPQ_PROBE_OPS(OP)                                                                                          \
  OP(raw_f, "mulmod_raw_t<false>", 1, r0 = mulmod_raw_t<false>(x, w0, k))                                          \
  OP(raw_t, "mulmod_raw_t<true>", 1, r0 = mulmod_raw_t<true>(x, w0, k))                                            \
  OP(split_s, "mulmod_split<TwS>", 1, r0 = mulmod_split(x, ws, k))                                                 \
  OP(split_w, "mulmod_split<TwW>", 1, r0 = mulmod_split(x, ww, k))                                                 \
  OP(ct_7, "ct_bfly(uint64_t)", 2, ct_bfly(x, y, w0, k); r0 = x; r1 = y)                                           \
  OP(ct_s, "ct_bfly(TwS)", 2, ct_bfly(x, y, ws, k); r0 = x; r1 = y)                                                \
  OP(ct_w1, "ct_bfly_wide<true>", 2, ct_bfly_wide<true>(x, y, ww, k); r0 = x; r1 = y)                              \
  OP(ct_w0, "ct_bfly_wide<false>", 2, ct_bfly_wide<false>(x, y, ww, k); r0 = x; r1 = y)                            \
  OP(gs_7, "gs_bfly(uint64_t)", 2, gs_bfly(x, y, w0, k); r0 = x; r1 = y)                                           \
  OP(gs_s, "gs_bfly_split<TwS>", 2, gs_bfly_split(x, y, ws, k); r0 = x; r1 = y)                                    \
  OP(gs_w1, "gs_bfly_wide<true>", 2, gs_bfly_wide<true>(x, y, ww, k); r0 = x; r1 = y)                              \
  OP(gs_w0, "gs_bfly_wide<false>", 2, gs_bfly_wide<false>(x, y, ww, k); r0 = x; r1 = y)                            \
  OP(last_7, "gs_last(LastK<uint64_t>)", 2, gs_last(x, y, LastK<uint64_t>(tab), k); r0 = x; r1 = y)                \
  OP(last_s, "gs_last(LastK<TwS>)", 2, gs_last(x, y, LastK<TwS>(tab), k); r0 = x; r1 = y)                          \
  OP(last_w, "gs_last(LastK<TwW>)", 2, gs_last(x, y, LastK<TwW>(tab), k); r0 = x; r1 = y)                          \
  OP(csub1, "csub1", 1, r0 = csub1(x, k))                                                                          \
  OP(csub2, "csub2", 1, r0 = csub2(x, k))                                                                          \
  OP(csub3, "csub3", 1, r0 = csub3(x, k))                                                                          \
  OP(csub4, "csub4", 1, r0 = csub4(x, k))                                                                          \
  OP(canon4, "canon4", 1, r0 = canon4(x, k))                                                                       \
  OP(canon8, "canon8", 1, r0 = canon8(x, k))                                                                       \
  OP(canon_fold, "canon_fold", 1, r0 = canon_fold(x, k.p, k.c))                                                    \
  OP(mul_canon, "mulmod_canon", 1, r0 = mulmod_canon(x, w0, k))                                                    \
  OP(mul_canon_lazy, "mulmod_canon_lazy", 1, r0 = mulmod_canon_lazy(x, w0, k))                                     \
  OP(add_canon, "addmod_canon", 1, r0 = addmod_canon(x, y, k))                                                     \
  OP(ref_fqmul, "ref_fqmul", 1, r0 = ref_fqmul(x, w0, k))                                                          \
  OP(horner59, "horner59", 1, r0 = horner59(x, y, k))                                                              \
  OP(t7_canon_fwd, "TwTraits<uint64_t>::canon_fwd", 1, r0 = TwTraits<uint64_t>::canon_fwd(x, k))                   \
  OP(t7_canon_inv, "TwTraits<uint64_t>::canon_inv", 1, r0 = TwTraits<uint64_t>::canon_inv(x, k))                   \
  OP(t7_inv_from8, "TwTraits<uint64_t>::inv_from8", 1, r0 = TwTraits<uint64_t>::inv_from8(x, k))                   \
  OP(t7_left, "TwTraits<uint64_t>::left", 1, r0 = TwTraits<uint64_t>::left(x, k))                                  \
  OP(t7_right, "TwTraits<uint64_t>::right", 1, r0 = TwTraits<uint64_t>::right(x, k))                               \
  OP(ts_canon_fwd, "TwTraits<TwS>::canon_fwd", 1, r0 = TwTraits<TwS>::canon_fwd(x, k))                             \
  OP(ts_canon_inv, "TwTraits<TwS>::canon_inv", 1, r0 = TwTraits<TwS>::canon_inv(x, k))                             \
  OP(ts_inv_from4, "TwTraits<TwS>::inv_from4", 1, r0 = TwTraits<TwS>::inv_from4(x, k))                             \
  OP(ts_inv_from8, "TwTraits<TwS>::inv_from8", 1, r0 = TwTraits<TwS>::inv_from8(x, k))                             \
  OP(ts_left, "TwTraits<TwS>::left", 1, r0 = TwTraits<TwS>::left(x, k))                                            \
  OP(tw_canon_fwd, "TwTraits<TwW>::canon_fwd", 1, r0 = TwTraits<TwW>::canon_fwd(x, k))                             \
  OP(tw_canon_inv, "TwTraits<TwW>::canon_inv", 1, r0 = TwTraits<TwW>::canon_inv(x, k))                             \
  OP(tw_inv_from8, "TwTraits<TwW>::inv_from8", 1, r0 = TwTraits<TwW>::inv_from8(x, k))                             \
  OP(tw_left, "TwTraits<TwW>::left", 1, r0 = TwTraits<TwW>::left(x, k))

enum {
#define GPQ_PROBE_ENUM(id, name, results, ...) PROBE_##id,
  GPQ_PROBE_OPS(GPQ_PROBE_ENUM)
#undef GPQ_PROBE_ENUM
  PROBE_NOPS
};

const char *const kOpNames[] = {
#define GPQ_PROBE_NAME(id, name, results, ...) name,
    GPQ_PROBE_OPS(GPQ_PROBE_NAME)
#undef GPQ_PROBE_NAME
};

// op is uniform across the launch; a lane handles one operand tuple.
__global__ __launch_bounds__(256) void modprobe_kernel(int op, PrimeK k0, const uint64_t *__restrict__ xs, const uint64_t *__restrict__ ys,
                                                       const uint64_t *__restrict__ w0s, const uint64_t *__restrict__ w1s,
                                                       uint64_t *__restrict__ out0, uint64_t *__restrict__ out1, size_t count) {
  const PrimeK k = pin_consts(k0);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint64_t x = xs[i], y = ys[i];
  const uint64_t w0 = w0s[i], w1 = w1s[i];
  TwS ws; ws.x = w0; ws.y = w1;
  TwW ww; ww.x = w0; ww.y = w1;
  LimbTab tab;
  tab.k = k; tab.ninv = w0; tab.winv1_ninv = w1; tab.ninv_s = ws; tab.winv1_ninv_s = ws;
  uint64_t r0 = 0, r1 = 0;
  switch (op) {
#define GPQ_PROBE_CASE(id, name, results, ...) \
  case PROBE_##id: { __VA_ARGS__; out0[i] = r0; if (results == 2) out1[i] = r1; } break;
    GPQ_PROBE_OPS(GPQ_PROBE_CASE)
#undef GPQ_PROBE_CASE
  default: break;
  }
}

// The conditional subtraction under lane masks that the one-call-per-lane kernel above never produces (csub_by's masked form narrows and
// restores the wave's lane mask itself): any workgroup size, so that a wave can start partly off; lanes at or past count return early;
// lanes with on[i] == 0 stay outside the divergent branch that subtracts.  out0 is written inside the branch, out1 behind it by every
// lane that did not return: a mask restored too wide or left too narrow shows as a word written, or not written, where the caller's
// fill says otherwise.  mul = 1 .. 4 picks csub1 .. csub4.
__global__ __launch_bounds__(256) void modprobe_csub_lanes_kernel(int mul, PrimeK k0, const uint64_t *__restrict__ xs, const unsigned char *__restrict__ on,
                                                                  uint64_t *__restrict__ out0, uint64_t *__restrict__ out1, size_t count) {
  const PrimeK k = pin_consts(k0);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint64_t x = xs[i];
  if (on[i]) {
    x = mul == 1 ? csub1(x, k) : mul == 2 ? csub2(x, k) : mul == 3 ? csub3(x, k) : csub4(x, k);
    out0[i] = x;
  }
  out1[i] = x;
}

}  // namespace

extern "C" {

int gpq_modprobe_nops(void) { return PROBE_NOPS; }

const char *gpq_modprobe_op_name(int op) { return op >= 0 && op < PROBE_NOPS ? kOpNames[op] : nullptr; }

// Runs op on count operand tuples with the constants of p (make_prime_k, as the context's tables).  x .. w1 and out0, out1 are host
// arrays of count words; y, w0, w1 and out1 may be null where the op does not use them (they then read as zero).  Allocates, uploads,
// launches, synchronises, downloads and frees; returns the HIP error code of the first call that failed, or 0.
int gpq_modprobe_run(int op, uint64_t p, const uint64_t *x, const uint64_t *y, const uint64_t *w0,
                                                            const uint64_t *w1, uint64_t *out0, uint64_t *out1, size_t count) {
  if (op < 0 || op >= PROBE_NOPS || !x || !out0 || p <= (1ull << 59) || p - (1ull << 59) >= GPQ_FOLD_CMAX) return (int)hipErrorInvalidValue;
  if (!count) return 0;
  const size_t bytes = count * sizeof(uint64_t);
  const uint64_t *src[4] = {x, y, w0, w1};
  uint64_t *dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int j = 0; j < 6 && e == hipSuccess; ++j) e = hipMalloc((void **)&dev[j], bytes);
  for (int j = 0; j < 4 && e == hipSuccess; ++j)
    e = src[j] ? hipMemcpy(dev[j], src[j], bytes, hipMemcpyHostToDevice) : hipMemset(dev[j], 0, bytes);
  for (int j = 4; j < 6 && e == hipSuccess; ++j) e = hipMemset(dev[j], 0, bytes);
  if (e == hipSuccess) {
    const unsigned threads = 256;
    const size_t blocks = (count + threads - 1) / threads;
    if (blocks > 0x7fffffffull) e = hipErrorInvalidValue;
    else {
      hipLaunchKernelGGL(modprobe_kernel, dim3((unsigned)blocks), dim3(threads), 0, 0, op, make_prime_k(p), dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], count);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out0, dev[4], bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out1) e = hipMemcpy(out1, dev[5], bytes, hipMemcpyDeviceToHost);
  for (int j = 0; j < 6; ++j)
    if (dev[j]) (void)hipFree(dev[j]);
  return (int)e;
}

// csub<mul> on blocks x threads lanes (threads <= 256, any value: 96 gives a second wave that starts half off), of which lanes
// >= count return early and lanes with on[i] == 0 skip the subtraction.  x, on, out0 and out1 are host arrays of blocks * threads
// entries; out0 and out1 are uploaded as given and downloaded again, so the caller sees which words the kernel wrote.
int gpq_modprobe_run_csub_lanes(int mul, uint64_t p, const uint64_t *x, const unsigned char *on, uint64_t *out0, uint64_t *out1, size_t count,
                                unsigned threads, unsigned blocks) {
  if (mul < 1 || mul > 4 || !x || !on || !out0 || !out1 || p <= (1ull << 59) || p - (1ull << 59) >= GPQ_FOLD_CMAX) return (int)hipErrorInvalidValue;
  if (!threads || threads > 256 || !blocks || blocks > 65535 || count > (size_t)threads * blocks) return (int)hipErrorInvalidValue;
  const size_t cap = (size_t)threads * blocks, bytes = cap * sizeof(uint64_t);
  uint64_t *dx = nullptr, *d0 = nullptr, *d1 = nullptr;
  unsigned char *don = nullptr;
  hipError_t e = hipMalloc((void **)&dx, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&d0, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&d1, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&don, cap);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d0, out0, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d1, out1, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(don, on, cap, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(modprobe_csub_lanes_kernel, dim3(blocks), dim3(threads), 0, 0, mul, make_prime_k(p), dx, don, d0, d1, count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out0, d0, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out1, d1, bytes, hipMemcpyDeviceToHost);
  if (dx) (void)hipFree(dx);
  if (d0) (void)hipFree(d0);
  if (d1) (void)hipFree(d1);
  if (don) (void)hipFree(don);
  return (int)e;
}

}  // extern "C"
