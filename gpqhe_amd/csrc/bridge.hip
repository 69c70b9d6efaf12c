// bridge.hip -- host side of the MPI <-> RNS bridge: the C ABI entry points (gpq_rns_decompose / _reconstruct, gpq_poly_mul, gpq_he_rs, gpq_he_mul,
// gpq_he_swk, gpq_he_rot_hoisted, gpq_he_gemv, ...) and the bridge's switches.  ONE translation unit -- every kernel template keeps one instantiation,
// one device function address (the dynamic-LDS attribute is per address) -- whose host code lies in the fragments included below.
#include "../../include/gpqhe_hip.h"
#include "engine_internal.hpp"
#include "bridge_kernels.hpp"
#include "bridge_mfma.hpp"
#include "bridge_stream.hpp"
#include "genswk_kernels.hpp"
#include "constpt_kernels.hpp"
#include "algo_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

using namespace gpq;

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)


#include "bridge_tables.hpp"   // host big integers; the constant tables (CRT constants per prefix of the prime chain: rns_init, src/precomp.c:266-293)
#include "bridge_launch.hpp"   // one launcher per kernel family
#include "bridge_tail.hpp"     // the relinearisation tail: tail_prescale_mode, relin_tail and its four flows

extern "C" int gpq_set_bridge_mfma(gpq_ctx *c, int on) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_set_bridge_mfma: null context");
  c->set.bridge_mfma = on != 0;
  return GPQ_OK;
}

extern "C" unsigned gpq_big_words(unsigned bits) { return (bits + 63) / 64; }

extern "C" uint64_t gpq_ctx_phat_invmp(gpq_ctx *c, unsigned dim, unsigned d) {
  gpq_bridge_basis *b;
  if (get_basis(c, 0, dim, &b) != GPQ_OK || d >= dim) return 0;
  return b->h_phat_inv[d];
}
extern "C" unsigned gpq_ctx_pbits(gpq_ctx *c, unsigned dim) {
  gpq_bridge_basis *b;
  return get_basis(c, 0, dim, &b) == GPQ_OK ? b->pbits : 0;
}

extern "C" int gpq_rns_decompose(gpq_ctx *c, uint64_t *slab, const uint64_t *big, unsigned W, unsigned dim, unsigned batch, void *stream) {
  int rc = check(c, dim, batch, "gpq_rns_decompose");
  if (rc) return rc;
  if (!slab || !big || W < 1) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_decompose: bad arguments");
  if ((rc = launch_decompose(c, slab, big, W, 0, dim, batch, (hipStream_t)stream))) return rc;
  return launched("gpq_rns_decompose");
}

extern "C" int gpq_rns_reconstruct(gpq_ctx *c, uint64_t *big, unsigned Wout, const uint64_t *slab, unsigned dim, unsigned batch,
                                   unsigned logq, void *stream) {
  int rc = check(c, dim, batch, "gpq_rns_reconstruct");
  if (rc) return rc;
  if (!slab || !big || Wout < 1) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_reconstruct: bad arguments");
  gpq_bridge_basis *b;
  if ((rc = get_basis(c, 0, dim, &b))) return rc;
  if (logq && Wout < (logq + 63) / 64) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_reconstruct: %u words cannot hold a value mod 2^%u", Wout, logq);
  if (!logq && Wout * 64 < b->pbits + 1) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_reconstruct: %u words cannot hold a value mod P (%u bits)", Wout, b->pbits);
  if ((rc = launch_reconstruct(c, b, big, Wout, slab, dim, 0, batch, logq, true, nullptr, (hipStream_t)stream))) return rc;
  return launched("gpq_rns_reconstruct");
}

// rns_reconstruct for ONE coefficient (src/rns.c:60-75 is per coefficient): host residues in, host words out, value in [0, P).
extern "C" int gpq_rns_reconstruct_one(gpq_ctx *c, uint64_t *words, unsigned Wout, const uint64_t *residues, unsigned dim) {
  int rc = check(c, dim, 1, "gpq_rns_reconstruct_one");
  if (rc) return rc;
  if (!words || !residues) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_reconstruct_one: null argument");
  gpq_bridge_basis *b;
  if ((rc = get_basis(c, 0, dim, &b))) return rc;
  if (Wout * 64 < b->pbits + 1) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_reconstruct_one: %u words cannot hold a value mod P (%u bits)", Wout, b->pbits);
  for (unsigned d = 0; d < dim; ++d)
    if (residues[d] >= c->p[d]) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_reconstruct_one: residue %u is not reduced", d);
  DeviceScope on_device(c->device);
  gpq_dev<uint64_t> dev;
  HIP_TRY(dev.alloc((size_t)(dim + Wout) * 8));
  hipError_t e = hipMemcpy(dev, residues, (size_t)dim * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = launch_reconstruct(c, b, dev + dim, Wout, dev, dim, 0, 1, 0, false, nullptr, nullptr, 0);
    if (rc == GPQ_OK) rc = launched("gpq_rns_reconstruct_one");
    if (rc == GPQ_OK) e = hipMemcpy(words, dev + dim, (size_t)Wout * 8, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "gpq_rns_reconstruct_one: %s", hipGetErrorString(e));
  return rc;
}

// rns_decompose for the limbs first .. first+count-1 only (src/rns.c:37-48 is per limb): slab[k][d][i], d < count.
extern "C" int gpq_rns_decompose_limbs(gpq_ctx *c, uint64_t *slab, const uint64_t *big, unsigned W, unsigned first, unsigned count,
                                       unsigned batch, void *stream) {
  int rc = check(c, count, batch, "gpq_rns_decompose_limbs");
  if (rc) return rc;
  if (!slab || !big || W < 1 || first + count > c->nprimes) return gpq_fail(GPQ_ERR_INVALID, "gpq_rns_decompose_limbs: bad arguments");
  if ((rc = launch_decompose(c, slab, big, W, first, count, batch, (hipStream_t)stream))) return rc;
  return launched("gpq_rns_decompose_limbs");
}

extern "C" size_t gpq_poly_mul_workspace_bytes(const gpq_ctx *c, unsigned dim, unsigned batch) {
  return 3ull * batch * ((size_t)dim << c->logn) * 8;
}

// poly_mul, src/poly.c:84-107, for q = 2^logq: decompose a and b to `dim` limbs, ntt, pointwise
// multiply, invntt, poly_rns2mpi.  r, a, b are big slabs of W words.
extern "C" int gpq_poly_mul(gpq_ctx *c, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned dim, unsigned logq,
                            unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dim, batch, "gpq_poly_mul");
  if (rc) return rc;
  if (!r || !a || !b || !workspace || !logq) return gpq_fail(GPQ_ERR_INVALID, "gpq_poly_mul: bad arguments (q must be 2^logq, logq > 0)");
  const size_t poly = (size_t)dim << c->logn;
  uint64_t *sa = (uint64_t *)workspace, *sb = sa + batch * poly, *sr = sb + batch * poly;
  if ((rc = gpq_rns_decompose(c, sa, a, W, dim, batch, stream))) return rc;
  if ((rc = gpq_rns_decompose(c, sb, b, W, dim, batch, stream))) return rc;
  if ((rc = gpq_poly_mul_rns(c, sr, sa, sb, dim, batch, stream))) return rc;
  return gpq_rns_reconstruct(c, r, W, sr, dim, batch, logq, stream);
}

// he_rs, src/he-rescale.c:33-54, for Delta = 2^logDelta and q_l = 2^logql: both polynomials of
// `batch` ciphertexts in place.  The level/nu/B bookkeeping of :36-38 stays with the caller.
extern "C" int gpq_he_rs(gpq_ctx *c, uint64_t *c0, uint64_t *c1, unsigned W, unsigned logDelta, unsigned logql, unsigned batch, void *stream) {
  if (!c || !c0 || !c1 || W < 1 || batch < 1 || logql < 1 || logql > 64 * W)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_rs: bad arguments");
  const dim3 grid((c->n + 255) / 256, batch), block(256);
  for (uint64_t *p : {c0, c1}) {
    RescaleArgs a{p, W, c->logn, logDelta, logql};
    ProfScope prof(c, GPQ_K_RESCALE, (hipStream_t)stream);
    hipLaunchKernelGGL(bridge_rescale, grid, block, 0, (hipStream_t)stream, a);
  }
  return launched("gpq_he_rs");
}
extern "C" int gpq_he_rescale(gpq_ctx *c, uint64_t *c0, uint64_t *c1, unsigned W, unsigned logDelta, unsigned logql, unsigned batch, void *stream) {
  return gpq_he_rs(c, c0, c1, W, logDelta, logql, batch, stream);
}

// ---------------------------------------------------------------------------
// he_mul / he_swk at the big-slab level (q_l = 2^logql)
// ---------------------------------------------------------------------------
namespace {

inline size_t align64(size_t b) { return (b + 63) & ~(size_t)63; }

// Workspace layouts of gpq_he_mul and gpq_he_swk for launch groups of m ciphertexts: byte offsets of the regions in the order they lie in,
// every size rounded to 64 bytes.  One definition for the *_workspace_bytes functions and for the entry points that carve the buffer.
struct HeMulPlan { size_t sA, wsT, sB, wsK, dbig, tail, total; };
int he_mul_plan(gpq_ctx *c, unsigned W, unsigned dimA, unsigned dimB, unsigned dimP, unsigned m, HeMulPlan *h) {
  TailPlan tp;
  int rc = tail_plan(c, W, dimP, dimB, 2 * m, &tp);                 // c0 and c1 of a launch group go through the tail together
  if (rc) return rc;
  const size_t n = c->n;
  h->sA = 0;
  h->wsT = h->sA + align64((size_t)m * 7 * dimA * n * 8);                  // sA: 4 decomposed inputs + d0hat,d1hat,d2hat
  h->sB = h->wsT + align64(gpq_tensor_workspace_bytes(c, dimA, m));
  h->wsK = h->sB + align64((size_t)m * 3 * dimB * n * 8);                  // sB: decomposed d2, c0hat, c1hat
  h->dbig = h->wsK + align64(gpq_keyswitch_workspace_bytes(c, dimB, m));
  h->tail = h->dbig + align64((size_t)m * 3 * W * n * 8);                  // dbig: d0, d1, d2
  h->total = h->tail + align64(tp.bytes);
  return GPQ_OK;
}
struct HeSwkPlan { size_t sB, wsK, tail, total; };
int he_swk_plan(gpq_ctx *c, unsigned W, unsigned dimB, unsigned dimP, unsigned m, HeSwkPlan *h) {
  TailPlan tp;
  int rc = tail_plan(c, W, dimP, dimB, 2 * m, &tp);
  if (rc) return rc;
  h->sB = 0;
  h->wsK = h->sB + align64((size_t)m * 3 * dimB * c->n * 8);               // sB: decomposed d1, c0hat, c1hat
  h->tail = h->wsK + align64(gpq_keyswitch_workspace_bytes(c, dimB, m));
  h->total = h->tail + align64(tp.bytes);
  return GPQ_OK;
}

}  // namespace

// dims the reference derives from the modulus chain: hectx.dim src/precomp.c:401, he_mul's
// tensor dim src/he-mult.c:99, he_relin/he_swk's dim src/he-mult.c:51, dimevk src/precomp.c:407.
extern "C" int gpq_he_dims(gpq_ctx *c, unsigned logqL, unsigned logql, unsigned *dimP, unsigned *dimA, unsigned *dimB, unsigned *dimevk) {
  if (!c || !logqL || !logql || logql > logqL) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_dims: bad arguments");
  const unsigned logn = c->logn;
  const unsigned dp = (logqL + 1 + logn) / 59 + 1;
  gpq_bridge_basis *bp;
  int rc = get_basis(c, 0, dp, &bp);
  if (rc) return rc;
  const unsigned nbPqL = bp->pbits + logqL;
  if (dimP) *dimP = dp;
  if (dimA) *dimA = (2 * (logql + 1) + logn) / 59 + 1;
  if (dimB) *dimB = ((logql + 1) + nbPqL + logn) / 59 + 1;
  if (dimevk) *dimevk = ((logqL + 1) + nbPqL + logn) / 59 + 1;
  return GPQ_OK;
}

extern "C" size_t gpq_he_mul_workspace_bytes(gpq_ctx *c, unsigned W, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch) {
  HeMulPlan h;
  return he_mul_plan(c, W, dimA, dimB, dimP, gpq_group_size(c, batch), &h) == GPQ_OK ? h.total : 0;
}

// he_mul, src/he-mult.c:88-156 (decl src/gpqhe.h:147), on big slabs of W words, q_l = 2^logql.
// ct = ct1 * ct2 relinearised with rlk (NTT-domain slabs of at least dimB limbs).  The l / nu / B
// bookkeeping of :92-95 stays with the caller.
// rs = 0: he_mul; rs = log2(Delta): he_mul followed by he_rs (src/he-rescale.c:33-54) with q_(l-1) = 2^(logql - rs), the rescale applied by the tail
// kernel on the way out where that kernel runs (1 <= rs <= 63), by the rescale kernel on the group's outputs otherwise.
static int he_mul_impl(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
                       const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
                       unsigned logql, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream, unsigned rs);
extern "C" int gpq_he_mul(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
                          const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
                          unsigned logql, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream) {
  return he_mul_impl(c, out_c0, out_c1, ct1c0, ct1c1, ct2c0, ct2c1, rlk0, rlk1, W, logql, dimA, dimB, dimP, batch, workspace, stream, 0);
}
extern "C" int gpq_he_mul_rs(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
                             const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
                             unsigned logql, unsigned dimA, unsigned dimB, unsigned dimP, unsigned logDelta, unsigned batch, void *workspace, void *stream) {
  if (!logDelta || logDelta >= logql) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_mul_rs: 0 < logDelta < logql");
  return he_mul_impl(c, out_c0, out_c1, ct1c0, ct1c1, ct2c0, ct2c1, rlk0, rlk1, W, logql, dimA, dimB, dimP, batch, workspace, stream, logDelta);
}
static int he_mul_impl(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
                       const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
                       unsigned logql, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream, unsigned rs) {
  const char *who = rs ? "gpq_he_mul_rs" : "gpq_he_mul";          // errors and launch checks name the entry point the caller used
  int rc = check(c, dimA, batch, who);
  if (rc || (rc = check(c, dimB, batch, who))) return rc;
  if (!out_c0 || !out_c1 || !ct1c0 || !ct1c1 || !ct2c0 || !ct2c1 || !rlk0 || !rlk1 || !workspace || !logql || W < (logql + 63) / 64)
    return gpq_fail(GPQ_ERR_INVALID, "%s: bad arguments", who);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = c->n, bigpoly = (size_t)W * n;
  const unsigned m = gpq_group_size(c, batch);
  HeMulPlan plan;
  if ((rc = he_mul_plan(c, W, dimA, dimB, dimP, m, &plan))) return rc;
  char *w = (char *)workspace;
  uint64_t *sA = (uint64_t *)(w + plan.sA), *sB = (uint64_t *)(w + plan.sB), *dbig = (uint64_t *)(w + plan.dbig);
  void *wsT = w + plan.wsT, *wsK = w + plan.wsK, *wsTail = w + plan.tail;
  gpq_bridge_basis *bA;
  if ((rc = get_basis(c, 0, dimA, &bA))) return rc;
  auto peer = [&](const PeerLane &lane, unsigned k0, unsigned polys) {       // every other launch group: the same call on the peer, for this group's slice
    const size_t o = k0 * bigpoly;
    return he_mul_impl(lane.c, out_c0 + o, out_c1 + o, ct1c0 + o, ct1c1 + o, ct2c0 + o, ct2c1 + o, rlk0, rlk1, W, logql, dimA, dimB, dimP,
                       polys, lane.ws, lane.s, rs);
  };
  auto own = [&](unsigned k0, unsigned polys) {
    int rc;
    const size_t pa = (size_t)polys * dimA * n, pb = (size_t)polys * dimB * n;
    uint64_t *h[4] = {sA, sA + pa, sA + 2 * pa, sA + 3 * pa};
    uint64_t *d0h = sA + 4 * pa, *d1h = sA + 5 * pa, *d2h = sA + 6 * pa;
    const uint64_t *in[4] = {ct1c0, ct1c1, ct2c0, ct2c1};
    // he_mul(&ct, &ct, &ct, rlk) (src/he-algo.c:151, the squarings of he_exp / he_inv): both operands are the same slabs --
    // two decompositions and two forward transforms instead of four, same residues
    const bool square = ct1c0 == ct2c0 && ct1c1 == ct2c1;
    {
      StageRange stage(square ? "gpq_he_mul: rns_decompose x2 (squaring)" : "gpq_he_mul: rns_decompose x4");
      const unsigned nin = square ? 2 : 4;                                                   // :117-120, one launch: h[0..3] are adjacent
      BigSources src{{in[0] + k0 * bigpoly, in[1] + k0 * bigpoly, in[square ? 0 : 2] + k0 * bigpoly, in[square ? 1 : 3] + k0 * bigpoly}, polys};
      if ((rc = launch_decompose(c, h[0], src, W, 0, dimA, nin * polys, s, c->set.lazy_decompose && c->logn > 12))) return rc;
    }
    const bool pre = can_prescale(c);      // the inverse passes hand the CRT kernels limbs already multiplied by (P/p_d)^-1
    const LimbTab *tabsA = nullptr, *tabsP = nullptr;
    int tail_mode = 0;
    if (pre && ((rc = get_scaled_tabs(c, bA, &tabsA)) || (rc = tail_prescale_mode(c, dimP, dimB, &tabsP, &tail_mode)))) return rc;
    apply_scaled_wide_limit(c, tabsA);
    apply_scaled_wide_limit(c, tabsP);
    if ((rc = gpq_he_mul_tensor_scaled(c, d0h, d1h, d2h, h[0], h[1], square ? h[0] : h[2], square ? h[1] : h[3], dimA, polys, wsT, stream, tabsA))) return rc;  // :121-136
    uint64_t *d0 = dbig, *d1 = dbig + polys * bigpoly, *d2 = dbig + 2 * polys * bigpoly;
    uint64_t *d2hat = sB, *c0hat = sB + pb, *c1hat = sB + 2 * pb;
    // With the one-product tail and bridge_stream.hpp, d0, d1, d2 (:139-141) never exist as words: d2hat goes CRT -> rns_decompose (:59) in
    // one kernel, d0hat | d1hat enter the tail as limbs.  Otherwise: poly_rns2mpi of the three adjacent slabs in one launch, rns_decompose of d2.
    const bool limbs_addend = pre && tail_mode == 3 && c->set.stream_bridge;
    bool fused = false;
    if (limbs_addend) {
      StageRange stage("gpq_he_mul: poly_rns2mpi d2 -> he_relin rns_decompose (one kernel)");
      if ((rc = crt_decompose_stream(c, bA, d2hat, d2h, d2, W, dimA, dimB, logql, polys, s, &fused))) return rc;
    }
    if (!fused) {
      {
        StageRange stage("gpq_he_mul: poly_rns2mpi d0,d1,d2 (CRT)");
        ReconExtra rx;
        rx.prescaled = pre;
        if (limbs_addend) rc = launch_reconstruct(c, bA, d2, W, d2h, dimA, 0, polys, logql, true, nullptr, s, -1, rx);
        else rc = launch_reconstruct(c, bA, d0, W, d0h, dimA, 0, 3 * polys, logql, true, nullptr, s, -1, rx);
        if (rc) return rc;
      }
      StageRange stage("gpq_he_mul: he_relin rns_decompose d2");
      if ((rc = launch_decompose(c, d2hat, d2, W, 0, dimB, polys, s, c->set.lazy_decompose && c->logn > 12))) return rc;          // :59
    }
    // he_relin, :40-85
    if ((rc = gpq_keyswitch_scaled(c, c0hat, c1hat, d2hat, rlk0, rlk1, dimB, polys, wsK, stream, tabsP))) return rc;   // :60-64
    StageRange stage("gpq_he_mul: he_relin tail (CRT, exact division by P, + d)");
    // c0 and c1 as one batch of 2 x polys polynomials: c0hat | c1hat and d0 | d1 are adjacent, the outputs are the caller's two slabs
    const TailD dh{d0h, bA, dimA, d0};
    bool rescaled = false;
    rc = relin_tail(c, Two<uint64_t>{out_c0 + k0 * bigpoly, out_c1 + k0 * bigpoly, polys}, c0hat,
                    limbs_addend ? Two<const uint64_t>{nullptr, nullptr, polys} : Two<const uint64_t>{d0, d1, polys},
                    W, dimP, dimB, logql, 2 * polys, wsTail, s, tail_mode, limbs_addend ? &dh : nullptr,                      // :67-77
                    rs >= 1 && rs <= 63 ? rs : 0u, &rescaled);   // the tail kernel shifts inside one word; other Deltas take the rescale kernel below
    if (rc) return rc;
    if (rs && !rescaled && (rc = gpq_he_rs(c, out_c0 + k0 * bigpoly, out_c1 + k0 * bigpoly, W, rs, logql - rs, polys, stream))) return rc;   // src/he-rescale.c:33-54
    return (int)GPQ_OK;
  };
  if ((rc = gpq_launch_groups(c, s, batch, m, gpq_lane_key(1, W, dimA, dimB, dimP, m ^ (logql << 8)),
                              [&](gpq_ctx *q) { return gpq_he_mul_workspace_bytes(q, W, dimA, dimB, dimP, m); }, own, peer))) return rc;
  return launched(who);
}

// he_swk, src/he-automorphism.c:40-85: key-switch d1 with swk, c0 += d0, on big slabs, q_l = 2^logql.
// (poly_rot / poly_conj, src/poly.c:263-283, are coefficient permutations done by the caller.)
extern "C" int gpq_he_swk(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *d0, const uint64_t *d1,
                          const uint64_t *swk0, const uint64_t *swk1, unsigned W, unsigned logql, unsigned dimB, unsigned dimP,
                          unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_he_swk");
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !d0 || !d1 || !swk0 || !swk1 || !workspace || !logql || W < (logql + 63) / 64)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_swk: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = c->n, bigpoly = (size_t)W * n;
  const unsigned m = gpq_group_size(c, batch);
  HeSwkPlan plan;
  if ((rc = he_swk_plan(c, W, dimB, dimP, m, &plan))) return rc;
  char *w = (char *)workspace;
  uint64_t *sB = (uint64_t *)(w + plan.sB);
  void *wsK = w + plan.wsK, *wsTail = w + plan.tail;
  auto peer = [&](const PeerLane &lane, unsigned k0, unsigned polys) {       // (as in gpq_he_mul)
    const size_t o = k0 * bigpoly;
    return gpq_he_swk(lane.c, out_c0 + o, out_c1 + o, d0 + o, d1 + o, swk0, swk1, W, logql, dimB, dimP, polys, lane.ws, lane.s);
  };
  auto own = [&](unsigned k0, unsigned polys) {
    int rc;
    const size_t pb = (size_t)polys * dimB * n;
    uint64_t *d1hat = sB, *c0hat = sB + pb, *c1hat = sB + 2 * pb;
    if ((rc = launch_decompose(c, d1hat, d1 + k0 * bigpoly, W, 0, dimB, polys, s, c->set.lazy_decompose && c->logn > 12))) return rc;   // :60
    const LimbTab *tabsP = nullptr;
    int tail_mode = 0;
    if ((rc = tail_prescale_mode(c, dimP, dimB, &tabsP, &tail_mode))) return rc;
    apply_scaled_wide_limit(c, tabsP);
    if ((rc = gpq_keyswitch_scaled(c, c0hat, c1hat, d1hat, swk0, swk1, dimB, polys, wsK, stream, tabsP))) return rc;   // :61-65
    // c0 (+ d0) and c1 (no addend) as one batch of 2 x polys polynomials                                           // :68-75
    if ((rc = relin_tail(c, Two<uint64_t>{out_c0 + k0 * bigpoly, out_c1 + k0 * bigpoly, polys}, c0hat, Two<const uint64_t>{d0 + k0 * bigpoly, nullptr, polys},
                         W, dimP, dimB, logql, 2 * polys, wsTail, s, tail_mode))) return rc;
    return (int)GPQ_OK;
  };
  if ((rc = gpq_launch_groups(c, s, batch, m, gpq_lane_key(2, W, 0, dimB, dimP, m ^ (logql << 8)),
                              [&](gpq_ctx *q) { return gpq_he_swk_workspace_bytes(q, W, dimB, dimP, m); }, own, peer))) return rc;
  return launched("gpq_he_swk");
}
extern "C" size_t gpq_he_swk_workspace_bytes(gpq_ctx *c, unsigned W, unsigned dimB, unsigned dimP, unsigned batch) {
  HeSwkPlan h;
  return he_swk_plan(c, W, dimB, dimP, gpq_group_size(c, batch), &h) == GPQ_OK ? h.total : 0;
}

// ---------------------------------------------------------------------------
// Hoisted rotations: he_rot (src/he-automorphism.c:101-115) of one ciphertext by several amounts.  The reference decomposes and transforms
// poly_rot(c1, r) for every r (:59-61); here c1 is decomposed and transformed once per launch group and each rotation permutes that
// transform (NTT(poly_rot(a, r)) = NTT(a) o sigma, ntt_kernels.hpp: automorphism_src).  The residues are those of the reference; the
// words of a forward transform can differ only where the reference stores p for 0 (src/ntt.c:45-48), and the product with the key
// reduces both to the same word, so every word from the product on is the reference's.
// ---------------------------------------------------------------------------
namespace {
uint64_t rot_power(unsigned rot) {                  // 5^rot modulo 2^64, as src/poly.c:266-268's size_t computes it
  uint64_t r = 1, b = 5;
  for (unsigned e = rot; e; e >>= 1, b *= b) if (e & 1) r *= b;
  return r;
}
struct HoistPlan { size_t x, chat, ks, rot, tail, total; };
int hoist_plan(gpq_ctx *c, unsigned W, unsigned dimB, unsigned dimP, unsigned nrot, unsigned m, HoistPlan *h) {
  TailPlan tp;
  int rc = tail_plan(c, W, dimP, dimB, 2 * m, &tp);
  if (rc) return rc;
  const size_t n = c->n, slab = (size_t)m * dimB * n * 8, big = (size_t)m * W * n * 8;
  if (nrot == 1) {                                   // he_swk as it is: both rotated polynomials, then gpq_he_swk
    *h = HoistPlan{0, 0, 0, 2 * align64(big), 0, 0};
    h->total = h->rot + align64(gpq_he_swk_workspace_bytes(c, W, dimB, dimP, m));
    return GPQ_OK;
  }
  h->x = align64(slab);
  h->chat = align64(2 * slab);
  h->ks = c->logn > 12 ? 0 : align64(gpq_keyswitch_workspace_bytes(c, dimB, m));
  h->rot = align64(big);
  h->tail = align64(tp.bytes);
  h->total = h->x + h->chat + h->ks + h->rot + h->tail;
  return GPQ_OK;
}
}  // namespace

extern "C" size_t gpq_he_rot_hoisted_workspace_bytes(gpq_ctx *c, unsigned W, unsigned dimB, unsigned dimP, unsigned nrot, unsigned batch) {
  if (!c || !nrot || !batch) return 0;
  HoistPlan h;
  return hoist_plan(c, W, dimB, dimP, nrot, gpq_group_size(c, batch), &h) == GPQ_OK ? h.total : 0;
}

extern "C" int gpq_he_rot_hoisted(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1,
                                  const unsigned *rots, const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned nrot,
                                  unsigned W, unsigned logql, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_he_rot_hoisted");
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !c0 || !c1 || !rots || !rk0 || !rk1 || !nrot || !workspace || !logql || W < (logql + 63) / 64)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_rot_hoisted: bad arguments");
  for (unsigned r = 0; r < nrot; ++r)
    if (!rk0[r] || !rk1[r]) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_rot_hoisted: key %u is NULL", r);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = c->n, bigpoly = (size_t)W * n;
  {   // every rotation reads c0 / c1 again after earlier rotations wrote their outputs: no overlap anywhere among the four ranges
    const size_t in_words = (size_t)batch * bigpoly, out_words = (size_t)nrot * in_words;
    if (ranges_overlap(out_c0, out_words, out_c1, out_words) || ranges_overlap(out_c0, out_words, c0, in_words) || ranges_overlap(out_c0, out_words, c1, in_words) ||
        ranges_overlap(out_c1, out_words, c0, in_words) || ranges_overlap(out_c1, out_words, c1, in_words))
      return gpq_fail(GPQ_ERR_INVALID, "gpq_he_rot_hoisted: the outputs alias each other or an input");
  }
  const unsigned m = gpq_group_size(c, batch);
  HoistPlan hp;
  if ((rc = hoist_plan(c, W, dimB, dimP, nrot, m, &hp))) return rc;
  char *w = (char *)workspace;
  if (nrot == 1) {                                   // nothing to share: poly_rot x2 + gpq_he_swk, group by group
    uint64_t *d0 = (uint64_t *)w, *d1 = (uint64_t *)(w + hp.rot / 2);
    for (unsigned k0 = 0; k0 < batch; k0 += m) {
      const unsigned polys = batch - k0 < m ? batch - k0 : m;
      const size_t o = k0 * bigpoly;
      if ((rc = gpq_poly_rot(c, d0, c0 + o, W, rots[0], polys, stream)) || (rc = gpq_poly_rot(c, d1, c1 + o, W, rots[0], polys, stream))) return rc;
      if ((rc = gpq_he_swk(c, out_c0 + o, out_c1 + o, d0, d1, rk0[0], rk1[0], W, logql, dimB, dimP, polys, w + hp.rot, stream))) return rc;
    }
    return launched("gpq_he_rot_hoisted");
  }
  uint64_t *X = (uint64_t *)w; w += hp.x;
  uint64_t *chat = (uint64_t *)w; w += hp.chat;
  void *wsK = w; w += hp.ks;
  uint64_t *d0 = (uint64_t *)w; w += hp.rot;
  void *wsTail = w;
  const LimbTab *tabsP = nullptr;
  int tail_mode = 0;
  if ((rc = tail_prescale_mode(c, dimP, dimB, &tabsP, &tail_mode))) return rc;
  apply_scaled_wide_limit(c, tabsP);
  const uint64_t mask2n = 2 * (uint64_t)n - 1;
  for (unsigned k0 = 0; k0 < batch; k0 += m) {
    const unsigned polys = batch - k0 < m ? batch - k0 : m;
    const size_t pb = (size_t)polys * dimB * n;
    {
      StageRange stage("gpq_he_rot_hoisted: rns_decompose + forward transform of c1 (once per group)");
      if ((rc = launch_decompose(c, X, c1 + k0 * bigpoly, W, 0, dimB, polys, s))) return rc;                 // src/he-automorphism.c:60
      if ((rc = gpq_hoist_forward(c, X, dimB, polys, s))) return rc;                                       // :61
    }
    for (unsigned r = 0; r < nrot; ++r) {
      StageRange stage("gpq_he_rot_hoisted: one rotation (permuted key switch + tail)");
      const unsigned g = (unsigned)(rot_power(rots[r]) & mask2n);
      if ((rc = gpq_poly_rot(c, d0, c0 + k0 * bigpoly, W, rots[r], polys, stream))) return rc;            // :108 (c1's is in the index map)
      if ((rc = gpq_keyswitch_rotated(c, chat, chat + pb, X, rk0[r], rk1[r], dimB, polys, g, wsK, s, tabsP))) return rc;   // :61-65
      const size_t o = ((size_t)r * batch + k0) * bigpoly;
      if ((rc = relin_tail(c, Two<uint64_t>{out_c0 + o, out_c1 + o, polys}, chat, Two<const uint64_t>{d0, nullptr, polys},
                           W, dimP, dimB, logql, 2 * polys, wsTail, s, tail_mode))) return rc;                // :68-75
    }
  }
  return launched("gpq_he_rot_hoisted");
}

// ---------------------------------------------------------------------------
// he_gemv, src/he-algo.c:47-93, on big slabs: baby steps j < n1 as ONE hoisted call (rk[j]), per giant step i the products with the
// diagonals diag[i n1 + j] (one gpq_he_mulpt over n1 x batch ciphertexts), their sum, he_rot by i n1 (rk[i n1]), the sum of the giant
// steps and he_rs.  With q_l = 2^logql every he_add (mpi_addm + mpi_smod, src/he-add.c:41-44) is the wrapping two's-complement sum of
// the big slabs followed by one centring: the sum is exact modulo 2^(64 W) and hence modulo q_l, and centring is a function of the
// residue modulo q_l.  So the sums run unreduced and are centred once -- before he_rot (whose rns_decompose reads the signed value)
// and before he_rs (whose rounding division does).
// ---------------------------------------------------------------------------
namespace {
void gemv_steps(unsigned slots, unsigned *n1, unsigned *n2) {  // :51-54 (sqrt of an unsigned, truncated)
  unsigned a = (unsigned)std::sqrt((double)slots);
  if (slots != a * a) a = (unsigned)std::sqrt((double)(2 * slots));
  *n1 = a;
  *n2 = slots / a;
}
struct GemvPlan { size_t r, mpt, p, g, ws, total; };
void gemv_plan(gpq_ctx *c, unsigned W, unsigned slots, unsigned dimB, unsigned dimP, unsigned dimpt, unsigned batch, GemvPlan *g) {
  unsigned n1, n2;
  gemv_steps(slots, &n1, &n2);
  const size_t big = (size_t)batch * W * c->n * 8;
  g->r = 2 * align64(n1 * big);                       // baby rotations, c0 | c1
  g->mpt = align64(n1 * big);                         // the diagonals of one giant step, one per ciphertext
  g->p = 2 * align64(n1 * big);                       // their products
  g->g = 2 * align64(big);                            // one giant rotation
  const size_t wn = gpq_he_rot_hoisted_workspace_bytes(c, W, dimB, dimP, n1, batch), w1 = gpq_he_rot_hoisted_workspace_bytes(c, W, dimB, dimP, 1, batch),
               wm = gpq_he_mulpt_workspace_bytes(c, dimpt, n1 * batch);
  if (!wn || !w1) { g->ws = g->total = 0; return; }       // either rotation plan failed (its message is in gpq_last_error)
  const size_t ws = wn > w1 ? wn : w1;
  g->ws = align64(ws > wm ? ws : wm);
  g->total = g->r + g->mpt + g->p + g->g + g->ws;
}

// The two steps every he_gemv call shares, plan or no plan (gemv_plan.hpp's driver calls them per launch group and per plan).
// One giant step's centred sum P joins the output (:80-84): he_rot by `shift` straight into out the first time, into G and a wrapping sum afterwards.
int gemv_add_giant(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *P0, const uint64_t *P1, uint64_t *G0, uint64_t *G1, bool first,
                   unsigned shift, const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logql, unsigned dimB, unsigned dimP,
                   unsigned batch, void *ws, void *stream) {
  int rc;
  if ((rc = gpq_he_rot_hoisted(c, first ? out_c0 : G0, first ? out_c1 : G1, P0, P1, &shift, rk0 + shift, rk1 + shift, 1, W, logql, dimB, dimP, batch, ws, stream))) return rc;
  if (first) return GPQ_OK;
  if ((rc = gpq_big_addsub(c, out_c0, out_c0, G0, W, batch, 0, stream))) return rc;
  return gpq_big_addsub(c, out_c1, out_c1, G1, W, batch, 0, stream);
}
// The sum of the giant steps leaves the call: centred (the adds' mpi_smod), then he_rs by Delta (:87, src/he-rescale.c:33-54).
int gemv_close(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, unsigned W, unsigned logDelta, unsigned logql, unsigned batch, void *stream) {
  int rc = gpq_he_rs(c, out_c0, out_c1, W, 0, logql, batch, stream);
  if (rc || !logDelta) return rc;
  return gpq_he_rs(c, out_c0, out_c1, W, logDelta, logql - logDelta, batch, stream);
}
}  // namespace

extern "C" size_t gpq_he_gemv_workspace_bytes(gpq_ctx *c, unsigned W, unsigned slots, unsigned dimB, unsigned dimP, unsigned dimpt, unsigned batch) {
  if (!c || !slots || !batch || !W) return 0;
  GemvPlan g;
  gemv_plan(c, W, slots, dimB, dimP, dimpt, batch, &g);
  return g.total;
}

extern "C" int gpq_he_gemv(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *diag,
                           const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned slots, unsigned W, unsigned logql,
                           unsigned logDelta, unsigned dimB, unsigned dimP, unsigned dimpt, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_he_gemv");
  if (rc || (rc = check(c, dimpt, batch, "gpq_he_gemv"))) return rc;
  if (!out_c0 || !out_c1 || !c0 || !c1 || !diag || !rk0 || !rk1 || !slots || !workspace || !logql || logDelta >= logql || W < (logql + 63) / 64)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv: bad arguments");
  unsigned n1, n2;
  gemv_steps(slots, &n1, &n2);
  hipStream_t s = (hipStream_t)stream;
  const size_t bigpoly = (size_t)W * c->n, big = batch * bigpoly;
  GemvPlan gp;
  gemv_plan(c, W, slots, dimB, dimP, dimpt, batch, &gp);
  if (!gp.total) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv: unsupported shape");
  char *w = (char *)workspace;
  uint64_t *R0 = (uint64_t *)w, *R1 = (uint64_t *)(w + gp.r / 2); w += gp.r;
  uint64_t *M = (uint64_t *)w; w += gp.mpt;
  uint64_t *P0 = (uint64_t *)w, *P1 = (uint64_t *)(w + gp.p / 2); w += gp.p;
  uint64_t *G0 = (uint64_t *)w, *G1 = (uint64_t *)(w + gp.g / 2); w += gp.g;
  void *ws = w;
  std::vector<unsigned> baby(n1);
  for (unsigned j = 0; j < n1; ++j) baby[j] = j;
  if ((rc = gpq_he_rot_hoisted(c, R0, R1, c0, c1, baby.data(), rk0, rk1, n1, W, logql, dimB, dimP, batch, ws, stream))) return rc;   // :63-68
  for (unsigned i = 0; i < n2; ++i) {
    for (unsigned j = 0; j < n1; ++j)                                                                                 // :70-72
      for (unsigned k = 0; k < batch; ++k)
        HIP_TRY(hipMemcpyAsync(M + ((size_t)j * batch + k) * bigpoly, diag + ((size_t)i * n1 + j) * bigpoly, bigpoly * 8, hipMemcpyDeviceToDevice, s));
    if ((rc = gpq_he_mulpt(c, P0, P1, R0, R1, M, W, logql, dimpt, n1 * batch, ws, stream))) return rc;                 // :74
    for (unsigned j = 1; j < n1; ++j)                                                                                 // :75-78
      if ((rc = gpq_big_addsub(c, P0, P0, P0 + j * big, W, batch, 0, stream)) || (rc = gpq_big_addsub(c, P1, P1, P1 + j * big, W, batch, 0, stream))) return rc;
    if ((rc = gpq_he_rs(c, P0, P1, W, 0, logql, batch, stream))) return rc;                                            // centred: he_rot decomposes it
    const unsigned shift = i * n1;
    if (!rk0[shift] || !rk1[shift]) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_gemv: key %u is NULL", shift);
    if ((rc = gemv_add_giant(c, out_c0, out_c1, P0, P1, G0, G1, i == 0, shift, rk0, rk1, W, logql, dimB, dimP, batch, ws, stream))) return rc;
  }
  if ((rc = gemv_close(c, out_c0, out_c1, W, logDelta, logql, batch, stream))) return rc;
  return launched("gpq_he_gemv");
}

#include "gemv_plan.hpp"   // he_gemv for a fixed matrix: gpq_gemv_plan_*, gpq_gemv_inner, gpq_he_gemv_planned
#include "gemv_multi.hpp"  // ... for several fixed matrices on the same ciphertexts: gpq_gemv_multi_*, gpq_he_gemv_multi

// Tail of he_relin / he_swk alone (src/he-mult.c:67-77): out = smod(rdiv(poly_rns2mpi(chat, P*q_l), P) + d, q_l).
extern "C" size_t gpq_relin_tail_workspace_bytes(gpq_ctx *c, unsigned W, unsigned dimB, unsigned dimP, unsigned batch) {
  TailPlan tp;
  return tail_plan(c, W, dimP, dimB, batch, &tp) == GPQ_OK ? tp.bytes + 64 : 0;
}
extern "C" int gpq_relin_tail(gpq_ctx *c, uint64_t *out, const uint64_t *chat, const uint64_t *d, unsigned W, unsigned logql,
                              unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_relin_tail");
  if (rc) return rc;
  if (!out || !chat || !workspace || !logql || W < (logql + 63) / 64) return gpq_fail(GPQ_ERR_INVALID, "gpq_relin_tail: bad arguments");
  return relin_tail(c, one_place(out), chat, one_place(d), W, dimP, dimB, logql, batch, workspace, (hipStream_t)stream);
}

// Big slabs between the kernels' layout (word-major) and rows of W words per coefficient (bridge_big_transpose): what the MPI-typed
// calls stage host data through.  to_rows = 0: rows -> words, 1: words -> rows.  n >= 64.
extern "C" int gpq_big_transpose(gpq_ctx *c, uint64_t *dst, const uint64_t *src, unsigned W, unsigned batch, int to_rows, void *stream) {
  if (!c || !dst || !src || W < 1 || W > 64 || batch < 1 || dst == src) return gpq_fail(GPQ_ERR_INVALID, "gpq_big_transpose: bad arguments");
  if (c->logn < 6) return gpq_fail(GPQ_ERR_INVALID, "gpq_big_transpose: n >= 64");
  BigTransposeArgs a{src, dst, W, c->logn, to_rows ? 1u : 0u};
  hipLaunchKernelGGL(bridge_big_transpose, dim3(c->n >> 6, batch), dim3(64), 0, (hipStream_t)stream, a);
  return launched("gpq_big_transpose");
}

// out = a + b / a - b / -a on `polys` big slabs of W words (two's complement, wrapping): the arithmetic of src/he-add.c before its mpi_smod
extern "C" int gpq_big_addsub(gpq_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, unsigned W, unsigned polys, int mode, void *stream) {
  if (!c || !out || !a || (mode != 2 && !b) || W < 1 || W > 64 || polys < 1 || mode < 0 || mode > 2) return gpq_fail(GPQ_ERR_INVALID, "gpq_big_addsub: bad arguments");
  BigAddSubArgs k{out, a, b, W, c->logn, (unsigned)mode};
  hipLaunchKernelGGL(bridge_big_addsub, dim3((c->n + 255) / 256, polys), dim3(256), 0, (hipStream_t)stream, k);
  return launched("gpq_big_addsub");
}

// The same tail for a caller that gives `chat` up as scratch: the CRT weights of the whole basis are put on it in place and the
// one-product kernel (tail_direct) finishes -- the form gpq_he_mul / gpq_he_swk reach without the extra pass, because their key
// switch delivers the weighted limbs.  Falls back to gpq_relin_tail's kernels when the product is not available (shape, settings).
extern "C" int gpq_relin_tail_overwriting(gpq_ctx *c, uint64_t *out, uint64_t *chat, const uint64_t *d, unsigned W, unsigned logql,
                                          unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dimB, batch, "gpq_relin_tail_overwriting");
  if (rc) return rc;
  if (!out || !chat || !workspace || !logql || W < (logql + 63) / 64) return gpq_fail(GPQ_ERR_INVALID, "gpq_relin_tail_overwriting: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  gpq_bridge_basis *bp, *bq;
  gpq_relin_tables *rt;
  if (dimB <= dimP) return gpq_fail(GPQ_ERR_INVALID, "relin: dimB=%u must exceed dimP=%u", dimB, dimP);
  if ((rc = get_basis(c, 0, dimP, &bp)) || (rc = get_basis(c, dimP, dimB - dimP, &bq)) || (rc = get_relin(c, dimP, dimB, &rt))) return rc;
  bool product = false;
  if ((rc = tail_product_tables(c, dimP, dimB, rt, bp, bq, &product))) return rc;
  int mode = 0;
  if (product && rt->d_scale) {
    LimbScaleArgs sc{c->d_tabs, chat, rt->d_scale, nullptr, dimB, c->logn};
    hipLaunchKernelGGL(bridge_limb_scale, dim3((c->n + 255) / 256, batch), dim3(256), 0, s, sc);
    mode = 3;
  }
  return relin_tail(c, one_place(out), chat, one_place(d), W, dimP, dimB, logql, batch, workspace, s, mode);
}

// gpq_he_mul / gpq_he_swk let their inverse transforms hand the CRT kernels limbs already multiplied by (P/p_d)^-1 (default on); off = the
// CRT kernels do that multiplication themselves.  Same results (tests run both).
extern "C" int gpq_set_prescale(gpq_ctx *c, int on) {      // 0: off, 1: the CRT weights only, 2: also w_j on the limbs above P for the relinearisation front, 3 (default): the one-product tail
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_set_prescale: null context");
  c->set.prescale = on != 0;
  c->set.prescale_upper = on >= 2;
  c->set.tail_direct = on >= 3;
  return GPQ_OK;
}

// gpq_he_mul / gpq_he_swk: bridge_stream.hpp's fused streaming kernels (default) or round 3's separate CRT / decompose / tail kernels.
// Same words either way (tests run both).
extern "C" int gpq_set_stream_bridge(gpq_ctx *c, int on) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_set_stream_bridge: null context");
  c->set.stream_bridge = on != 0;
  return GPQ_OK;
}

// gpq_he_mul / gpq_he_swk over more than one launch group: alternate groups on two streams (default) or all on the caller's.  Same words.
extern "C" int gpq_set_overlap(gpq_ctx *c, int on) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_set_overlap: null context");
  c->overlap = on < 0 ? -1 : (on != 0);
  return GPQ_OK;
}
// tests: make the next creation of the peer lane fail the way an allocation would (the call must run on one lane and say so once)
extern "C" int gpq_debug_fail_peer(gpq_ctx *c, int on) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_debug_fail_peer: null context");
  c->debug_peer_fail = on == 3 ? 0 : on;                         // 3: stop failing allocations but keep what was declined so far
  if (!on) { c->peer_failed = false; c->peer_ws_declined = 0; }
  return GPQ_OK;
}
// lanes the last gpq_he_mul / gpq_he_swk / gpq_he_mul_tensor / gpq_keyswitch call on this context ran on (1 or 2)
extern "C" unsigned gpq_last_lanes(const gpq_ctx *c) { return c ? c->last_lanes : 0; }

// gpq_he_mul: its own rns_decompose launches (src/he-mult.c:117-120, :59) may leave residues in (0, 3p) for the forward transforms that read them
// (default on; canonical with 0).  Same results: the transforms reduce lazily anyway.
extern "C" int gpq_set_lazy_decompose(gpq_ctx *c, int on) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_set_lazy_decompose: null context");
  c->set.lazy_decompose = on != 0;
  return GPQ_OK;
}

// Tests: bridge_stream.hpp's kernels also hand every coefficient whose index is a multiple of `every` to the exact kernels behind them (0: off).
extern "C" int gpq_debug_force_redo(gpq_ctx *c, unsigned every) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_debug_force_redo: null context");
  c->set.debug_force_redo = every;
  return GPQ_OK;
}

// Tests: force the exact (full-width) CRT kernel instead of the low-word fast path.
extern "C" int gpq_set_exact_crt(gpq_ctx *c, int on) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "gpq_set_exact_crt: null context");
  c->set.exact_crt = on != 0;
  return GPQ_OK;
}

// Diagnostics: how many of the first `count` coefficients the last fast CRT pass flagged for the exact kernel.
extern "C" long gpq_debug_redo_count(gpq_ctx *c, size_t count) {
  if (!c || !c->d_redo || count > c->d_redo.bytes) return -1;
  std::vector<unsigned char> h(count);
  if (hipMemcpy(h.data(), c->d_redo, count, hipMemcpyDeviceToHost) != hipSuccess) return -2;
  long k = 0;
  for (unsigned char v : h) k += v != 0;
  return k;
}

#include "bridge_general.hpp"   // any modulus q given as words: gpq_*_general, through the Barrett kernel

// ---------------------------------------------------------------------------
// he_mulpt, poly_rot / poly_conj, he_rot / he_conj at the big-slab level
// ---------------------------------------------------------------------------
extern "C" size_t gpq_he_mulpt_workspace_bytes(const gpq_ctx *c, unsigned dim, unsigned batch) {
  return 3ull * batch * ((size_t)dim << c->logn) * 8;
}

// he_mulpt, src/he-mult.c:159-196 (decl src/gpqhe.h:148): (c0, c1) * m per ciphertext, q_l = 2^logql.
// dim is the caller's (it depends on log2(pt->nu), a host double, :169).  Bookkeeping (:162-164) stays with the caller.
extern "C" int gpq_he_mulpt(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m,
                            unsigned W, unsigned logql, unsigned dim, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dim, batch, "gpq_he_mulpt");
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !c0 || !c1 || !m || !workspace || !logql) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_mulpt: bad arguments");
  const size_t poly = (size_t)dim << c->logn;
  uint64_t *s0 = (uint64_t *)workspace, *s1 = s0 + batch * poly, *sm = s1 + batch * poly;
  if ((rc = gpq_rns_decompose(c, sm, m, W, dim, batch, stream))) return rc;       // :176
  if ((rc = gpq_rns_decompose(c, s0, c0, W, dim, batch, stream))) return rc;      // :177
  if ((rc = gpq_rns_decompose(c, s1, c1, W, dim, batch, stream))) return rc;      // :178
  if ((rc = gpq_mulpt_rns(c, s0, s1, sm, s0, s1, dim, batch, stream))) return rc;                                          // :179-185
  if ((rc = gpq_rns_reconstruct(c, out_c0, W, s0, dim, batch, logql, stream))) return rc;                                 // :188
  return gpq_rns_reconstruct(c, out_c1, W, s1, dim, batch, logql, stream);                                                // :189
}

// ---------------------------------------------------------------------------
// constant plaintexts: he_const_pt's a + b x^(n/2) (constpt_kernels.hpp)
// ---------------------------------------------------------------------------
// src/he-encode.c:119-125 for Delta = 2^logDelta: the long double product is the double scaled by a power of two (exact), round() of it is
// half away from zero, and double_to_mpi takes the integer as it is.
extern "C" int gpq_const_pt(double re, double im, unsigned logDelta, int64_t *a, int64_t *b) {
  if (!a || !b || logDelta > 1023) return gpq_fail(GPQ_ERR_INVALID, "gpq_const_pt: bad arguments");
  int64_t out[2];
  const double in[2] = {re, im};
  for (int i = 0; i < 2; ++i) {
    const double r = std::round(std::ldexp(in[i], (int)logDelta));
    if (!std::isfinite(r) || r < -9223372036854775808.0 || r >= 9223372036854775808.0)
      return gpq_fail(GPQ_ERR_INVALID, "gpq_const_pt: %g * 2^%u is not finite or does not fit int64_t", in[i], logDelta);
    out[i] = (int64_t)r;
  }
  *a = out[0]; *b = out[1];
  return GPQ_OK;
}

namespace {
inline uint64_t magnitude(int64_t v) { return v < 0 ? 0 - (uint64_t)v : (uint64_t)v; }     // INT64_MIN -> 2^63
}

// The reference's he_mulpt returns smod(smod(v mod P, P), q_l) with P the product of the first `dim` primes (poly_rns2mpi, src/poly.c:109-120),
// which is smod(v, q_l) exactly when |v| < floor(P/2).  For inputs centred mod 2^logql, |v| <= (|a| + |b|) 2^(logql-1).
extern "C" int gpq_he_mulpt_const_fits(const gpq_ctx *c, int64_t a, int64_t b, unsigned logql, unsigned dim) {
  if (!c || !logql || dim < 1 || dim > c->nprimes) return 0;
  Big P{1};
  for (unsigned d = 0; d < dim; ++d) mul_small(P, c->p[d]);
  shr1(P);                                                                      // floor(P/2)
  const u128h sum = (u128h)magnitude(a) + magnitude(b);                          // < 2^65
  const unsigned sh = logql - 1, ws = sh >> 6, bs = sh & 63;
  Big lhs(ws + 3, 0);
  const uint64_t w[3] = {(uint64_t)sum, (uint64_t)(sum >> 64), 0};
  for (unsigned i = 0; i < 3; ++i) lhs[ws + i] = bs ? (w[i] << bs) | (i ? w[i - 1] >> (64 - bs) : 0) : w[i];
  return cmp_big(lhs, P) < 0;
}

extern "C" int gpq_he_mulpt_const(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, int64_t a, int64_t b,
                                  unsigned W, unsigned logql, unsigned dim, unsigned logDelta, unsigned batch, unsigned *bad_dev, void *stream) {
  int rc = check(c, dim, batch, "gpq_he_mulpt_const");
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !c0 || !c1 || W < 1 || W > 64 || logql < 1 || logql > 64 * W || logDelta >= logql || c->logn < 1 || batch > 32767)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_mulpt_const: bad arguments (1 <= logql <= 64 W, logDelta < logql)");
  if (!gpq_he_mulpt_const_fits(c, a, b, logql, dim))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_mulpt_const: (|a| + |b|) 2^%u reaches half the basis of %u limbs: he_mulpt's words are not the closed form", logql - 1, dim);
  const unsigned s = logDelta < 64 ? logDelta : 0;                               // wider shifts: the plain product, then gpq_he_rs
  MulptConstArgs k{out_c0, out_c1, c0, c1, magnitude(a), magnitude(b), a < 0, b < 0, W, c->logn, s, logql, bad_dev};
  {
    ProfScope prof(c, GPQ_K_MULPT_CONST, (hipStream_t)stream);
    const unsigned threads = b ? c->n >> 1 : c->n;
    const dim3 grid((threads + 255) / 256, 2 * batch), block(256);
    if (b) hipLaunchKernelGGL(he_mulpt_const<true>, grid, block, 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(he_mulpt_const<false>, grid, block, 0, (hipStream_t)stream, k);
  }
  if ((rc = launched("gpq_he_mulpt_const"))) return rc;
  return logDelta >= 64 ? gpq_he_rs(c, out_c0, out_c1, W, logDelta, logql - logDelta, batch, stream) : GPQ_OK;   // src/he-rescale.c:33-54
}

extern "C" int gpq_he_addpt_const(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, int64_t a, int64_t b,
                                  int sub, unsigned W, unsigned logql, unsigned batch, void *stream) {
  int rc = check(c, 1, batch, "gpq_he_addpt_const");
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !c0 || !c1 || W < 1 || W > 64 || logql < 1 || logql > 64 * W || c->logn < 1 || batch > 32767)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_addpt_const: bad arguments (1 <= logql <= 64 W)");
  AddptConstArgs k{out_c0, out_c1, c0, c1, a, b, sub ? 1u : 0u, W, c->logn, logql};
  {
    ProfScope prof(c, GPQ_K_ADDPT_CONST, (hipStream_t)stream);
    hipLaunchKernelGGL(he_addpt_const, dim3((c->n + 255) / 256, 2 * batch), dim3(256), 0, (hipStream_t)stream, k);
  }
  return launched("gpq_he_addpt_const");
}

// he_dec, src/he-encrypt.c:105-125, for q_l = 2^logql: m = smod(poly_mul(c1, sk, dim, q_l) + c0, q_l) for `batch` ciphertexts and ONE key.
// sk_ntt = the secret key as he_genswk would store it (gpq_evk_pack of its big slab): uint64_t[dim][n], read by every ciphertext of the
// batch through the pointwise kernel's shared operand -- the key exists once and the launches do not grow with the batch.  dim is the
// caller's (:113).  The words are the reference's also when c1 * sk wraps the dim-limb basis: the same residues, the same CRT.
extern "C" size_t gpq_he_dec_workspace_bytes(const gpq_ctx *c, unsigned dim, unsigned batch) {
  return c ? (size_t)batch * ((size_t)dim << c->logn) * 8 : 0;
}

extern "C" int gpq_he_dec(gpq_ctx *c, uint64_t *m, const uint64_t *c0, const uint64_t *c1, const uint64_t *sk_ntt, unsigned W, unsigned logql,
                          unsigned dim, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, dim, batch, "gpq_he_dec");
  if (rc) return rc;
  if (!m || !c0 || !c1 || !sk_ntt || !workspace || !logql) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_dec: bad arguments (q_l must be 2^logql, logql > 0)");
  if (W < 1 || 64ull * W <= logql) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_dec: %u words cannot hold a centred coefficient mod 2^%u (64 W > logql)", W, logql);
  const size_t big = (size_t)batch * W * c->n, key = (size_t)dim << c->logn;
  if (ranges_overlap(m, big, c0, big) || ranges_overlap(m, big, c1, big) || ranges_overlap(m, big, sk_ntt, key))
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_dec: the output aliases an input");
  StageRange stage("gpq_he_dec");
  uint64_t *x = (uint64_t *)workspace;
  if ((rc = gpq_rns_decompose(c, x, c1, W, dim, batch, stream))) return rc;              // src/poly.c:96-103 with the key's limbs already transformed
  if ((rc = gpq_ntt(c, x, dim, batch, stream))) return rc;
  if ((rc = gpq_rns_mul_shared(c, x, x, sk_ntt, dim, batch, (hipStream_t)stream))) return rc;
  if ((rc = gpq_invntt(c, x, dim, batch, stream))) return rc;
  if ((rc = gpq_rns_reconstruct(c, m, W, x, dim, batch, logql, stream))) return rc;       // poly_rns2mpi, :104
  return gpq_big_add(c, m, m, c0, W, logql, batch, stream);                                // src/he-encrypt.c:117-118
}

static int permute(gpq_ctx *c, uint64_t *r, const uint64_t *a, unsigned W, unsigned batch, unsigned long long power, int conj, void *stream) {
  if (!c || !r || !a || r == a || W < 1 || batch < 1) return gpq_fail(GPQ_ERR_INVALID, "poly_rot/poly_conj: bad arguments (not in place)");
  PermuteArgs p{a, r, W, c->logn, power, conj};
  hipLaunchKernelGGL(bridge_permute, dim3((c->n + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, p);
  return launched("bridge_permute");
}
// poly_rot, src/poly.c:263-275 (5^rot as :266-268 computes it, modulo 2^64 -- harmless since 2n divides 2^64)
extern "C" int gpq_poly_rot(gpq_ctx *c, uint64_t *r, const uint64_t *a, unsigned W, unsigned rot, unsigned batch, void *stream) {
  unsigned long long power = 1;
  for (unsigned j = 0; j < rot; ++j) power *= 5;
  return permute(c, r, a, W, batch, power, 0, stream);
}
// poly_conj, src/poly.c:277-283
extern "C" int gpq_poly_conj(gpq_ctx *c, uint64_t *r, const uint64_t *a, unsigned W, unsigned batch, void *stream) {
  return permute(c, r, a, W, batch, 1, 1, stream);
}

// he_add / he_sub / he_neg on one polynomial (src/he-add.c), q_l = 2^logql; r may alias a or b.
static int addsub(gpq_ctx *c, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned logql, unsigned mode, unsigned batch, void *stream) {
  if (!c || !r || !a || (mode < 2 && !b) || W < 1 || batch < 1 || !logql || logql > 64 * W) return gpq_fail(GPQ_ERR_INVALID, "gpq_big_add/sub/neg: bad arguments");
  AddSubArgs p{r, a, b, W, c->logn, logql, mode};
  hipLaunchKernelGGL(bridge_addsub, dim3((c->n + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, p);
  return launched("bridge_addsub");
}
extern "C" int gpq_big_add(gpq_ctx *c, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned logql, unsigned batch, void *stream) {
  return addsub(c, r, a, b, W, logql, 0, batch, stream);
}
extern "C" int gpq_big_sub(gpq_ctx *c, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned logql, unsigned batch, void *stream) {
  return addsub(c, r, a, b, W, logql, 1, batch, stream);
}
extern "C" int gpq_big_neg(gpq_ctx *c, uint64_t *r, const uint64_t *a, unsigned W, unsigned logql, unsigned batch, void *stream) {
  return addsub(c, r, a, nullptr, W, logql, 2, batch, stream);
}

// Key slabs as he_genswk stores them (src/he-kem.c:103-110): rns_decompose + ntt of a centred big-slab polynomial
// over dimevk limbs.  evk = uint64_t[batch][dimevk][n].
extern "C" int gpq_evk_pack(gpq_ctx *c, uint64_t *evk, const uint64_t *big, unsigned W, unsigned dimevk, unsigned batch, void *stream) {
  int rc = gpq_rns_decompose(c, evk, big, W, dimevk, batch, stream);
  return rc ? rc : gpq_ntt(c, evk, dimevk, batch, stream);
}

// he_genswk, src/he-kem.c:74-118, from the polynomials the reference samples on the host (p1 uniform mod P q_L, the error e) and
// the one the key hides (sp: s^2 for he_genrlk, the rotated / conjugated secret for he_genrk / he_genck):
//   swk.p0 = smod(-p1 * sk + e + P * sp, P q_L),  swk.p1 = smod(p1, P q_L),  both stored as rns_decompose + ntt over dimevk limbs.
// q_L = 2^logqL.  Big slabs of W words (W > bits(P q_L) / 64); one key per call.
namespace {
struct GenswkPlan { unsigned WPw, WF, dimmul, Lq; std::vector<uint64_t> PqL; size_t words; };
int genswk_plan(gpq_ctx *c, unsigned W, unsigned dimP, unsigned logqL, GenswkPlan *p) {
  gpq_bridge_basis *bp;
  int rc = get_basis(c, 0, dimP, &bp);
  if (rc) return rc;
  Big q = bp->h_P;
  const unsigned wsh = logqL / 64, bsh = logqL % 64;          // P << logqL
  Big sh(q.size() + wsh + 1, 0);
  for (size_t j = 0; j < q.size(); ++j) {
    sh[j + wsh] |= q[j] << bsh;
    if (bsh) sh[j + wsh + 1] |= q[j] >> (64 - bsh);
  }
  while (sh.size() > 1 && sh.back() == 0) sh.pop_back();
  p->PqL = sh; p->Lq = (unsigned)sh.size();
  p->WPw = (unsigned)bp->h_P.size();
  p->WF = W + p->WPw + 1;
  const unsigned nb = 64 * (p->Lq - 1) + (64 - __builtin_clzll(sh.back()));
  p->dimmul = (nb + c->logn) / 59 + 1;                          // src/he-kem.c:83
  if (W * 64 <= nb) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_genswk: %u words cannot hold values mod P q_L (%u bits)", W, nb);
  if (W > 32 || p->WPw > (unsigned)GENSWK_MAXP || p->dimmul > c->nprimes)
    return gpq_fail(GPQ_ERR_UNSUPPORTED, "gpq_he_genswk: W=%u, P of %u words, %u limbs", W, p->WPw, p->dimmul);
  p->words = ((size_t)(3 * W + p->WF) << c->logn) + (p->WPw + 7) / 8 * 8 + kModConstWords;
  return GPQ_OK;
}
}  // namespace

extern "C" size_t gpq_he_genswk_workspace_bytes(gpq_ctx *c, unsigned W, unsigned dimP, unsigned logqL) {
  GenswkPlan p;
  if (!c || genswk_plan(c, W, dimP, logqL, &p) != GPQ_OK) return 0;
  return p.words * 8 + gpq_poly_mul_general_workspace_bytes(c, p.dimmul, 1);
}

extern "C" int gpq_he_genswk(gpq_ctx *c, uint64_t *evk0, uint64_t *evk1, const uint64_t *p1, const uint64_t *sk, const uint64_t *e,
                             const uint64_t *sp, unsigned W, unsigned dimP, unsigned logqL, unsigned dimevk, void *workspace, void *stream) {
  if (!c || !evk0 || !evk1 || !p1 || !sk || !e || !sp || !workspace || !logqL) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_genswk: bad arguments");
  int rc = check(c, dimevk, 1, "gpq_he_genswk");
  if (rc) return rc;
  GenswkPlan gp;
  if ((rc = genswk_plan(c, W, dimP, logqL, &gp))) return rc;
  gpq_bridge_basis *bp;
  if ((rc = get_basis(c, 0, dimP, &bp))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = c->n;
  uint64_t *t = (uint64_t *)workspace, *x = t + W * n, *p0 = x + gp.WF * n, *p1c = p0 + W * n, *dP = p1c + W * n,
           *dconst = dP + (gp.WPw + 7) / 8 * 8;
  void *wsmul = dconst + kModConstWords;
  if ((rc = gpq_poly_mul_general(c, t, p1, sk, W, gp.dimmul, gp.PqL.data(), gp.Lq, 1, wsmul, stream))) return rc;      // :95
  HIP_TRY(hipMemcpyAsync(dP, bp->h_P.data(), gp.WPw * 8, hipMemcpyHostToDevice, s));
  GenswkArgs ga{t, e, sp, dP, x, W, gp.WPw, gp.WF, c->logn};
  hipLaunchKernelGGL(bridge_genswk_combine, dim3((c->n + 63) / 64), dim3(64), 0, s, ga);                                 // :96-98
  if ((rc = launch_smod_general(c, p0, W, x, gp.WF, gp.PqL.data(), gp.Lq, 1, dconst, s))) return rc;                    // :99
  if ((rc = launch_smod_general(c, p1c, W, p1, W, gp.PqL.data(), gp.Lq, 1, dconst, s))) return rc;                      // :100
  if ((rc = gpq_evk_pack(c, evk0, p0, W, dimevk, 1, stream)) || (rc = gpq_evk_pack(c, evk1, p1c, W, dimevk, 1, stream))) return rc;   // :103-110
  return launched("gpq_he_genswk");
}

#include "bridge_genswk.hpp"   // gpq_he_genswk_batch: `count` keys per call through the CRT split of P 2^k (genswk_crt_tail)
#include "bridge_algo.hpp"     // the evaluators of src/he-algo.c:131-458: gpq_he_lin_const, gpq_he_inv / _sqrt / _sigmoid / _log / _exp
