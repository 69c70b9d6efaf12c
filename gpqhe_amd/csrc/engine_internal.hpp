// engine_internal.hpp -- the context object behind the opaque gpq_ctx handle.
#pragma once
#include <atomic>
#include <cstdio>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "tables.hpp"

struct gpq_ctx;
int gpq_fail(int code, const char *fmt, ...);

// Is `s` inside a stream capture?  A failed query counts as "no" (*query_failed says so: gpq_peer_lane then takes no lane and clears the error).
inline bool gpq_capturing(hipStream_t s, bool *query_failed = nullptr) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool ok = hipStreamIsCapturing(s, &cap) == hipSuccess;
  if (query_failed) *query_failed = !ok;
  return ok && cap != hipStreamCaptureStatusNone;
}

// The one owner of a device allocation: move-only, frees in its destructor, hands out its pointer wherever a T * is wanted (launch code and
// kernel-argument structs read members of this type as plain pointers).  Bytes that upload() added to a table cache's device_bytes leave it
// again with the owner, so a builder that fails half way leaks nothing and over-counts nothing.
template <typename T>
struct gpq_dev {
  T *p = nullptr;
  size_t bytes = 0;
  size_t *counted = nullptr;          // the device_bytes these bytes are part of (read-only tables), or null
  gpq_dev() = default;
  gpq_dev(gpq_dev &&o) noexcept : p(o.p), bytes(o.bytes), counted(o.counted) { o.p = nullptr; o.bytes = 0; o.counted = nullptr; }
  gpq_dev &operator=(gpq_dev &&o) noexcept { if (this != &o) { reset(); std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(counted, o.counted); } return *this; }
  gpq_dev(const gpq_dev &) = delete;
  gpq_dev &operator=(const gpq_dev &) = delete;
  ~gpq_dev() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    if (counted) *counted -= bytes;
    p = nullptr; bytes = 0; counted = nullptr;
  }
  operator T *() const { return p; }
  template <typename U> explicit operator U *() const { return (U *)p; }
  // a fresh block of `nbytes` on the current device (what it held before is freed)
  hipError_t alloc(size_t nbytes) {
    reset();
    const hipError_t e = hipMalloc((void **)&p, nbytes);
    if (e == hipSuccess) bytes = nbytes; else p = nullptr;
    return e;
  }
  // a host vector as a read-only table of the context's cache, on the context's device; the copy is synchronous
  template <typename U> int upload(gpq_ctx *c, const std::vector<U> &v);
  // Scratch that grows at the first call of a new size: refused inside a stream capture (`refusal`: hipMalloc would go into the graph),
  // allocated on the context's device, zeroed on the LAUNCH stream if asked (a plain hipMemset goes to the null stream, which a non-blocking
  // stream -- torch's side streams, the peer lane's -- does not wait for: the words could be zeroed after a kernel wrote them); the
  // outgrown block is retired to the context, not freed: a HIP graph captured earlier may still use it.
  int grow(gpq_ctx *c, hipStream_t s, size_t nbytes, bool zero_on_stream, const char *refusal);
  void retire(gpq_ctx *c);
};

// ... and of a stream or an event
template <typename H, hipError_t (*Destroy)(H)>
struct gpq_handle {
  H h = nullptr;
  gpq_handle() = default;
  gpq_handle(gpq_handle &&o) noexcept : h(o.h) { o.h = nullptr; }
  gpq_handle &operator=(gpq_handle &&o) noexcept { std::swap(h, o.h); return *this; }
  ~gpq_handle() { if (h) (void)Destroy(h); }
  operator H() const { return h; }
};
using gpq_event = gpq_handle<hipEvent_t, hipEventDestroy>;
using gpq_stream_own = gpq_handle<hipStream_t, hipStreamDestroy>;

// Optional per-launch timing with HIP events recorded on the launch stream
// (bench.py's roofline leg).  Off by default: no events are created.
struct gpq_prof_rec { int kernel = 0; gpq_event a, b; };
enum { GPQ_K_STRIDED_FWD = 0, GPQ_K_STRIDED_INV, GPQ_K_CONTIG_FWD, GPQ_K_CONTIG_INV, GPQ_K_TENSOR_MID,
       GPQ_K_KEYSWITCH_MID, GPQ_K_POINTWISE, GPQ_K_SMALL, GPQ_K_REFERENCE,
       // the MPI <-> RNS bridge (bridge.hip): rns_decompose, the CRT fast paths, the relinearisation front, the exact /
       // masked kernels (bridge_reconstruct, bridge_roundfix, bridge_addround, bridge_exactdiv), he_rs
       GPQ_K_DECOMPOSE, GPQ_K_RECONSTRUCT, GPQ_K_RELIN_FRONT, GPQ_K_BRIDGE_EXACT, GPQ_K_RESCALE, GPQ_K_RELIN_TAIL_DIRECT,
       // bridge_stream.hpp: CRT(d2hat) -> rns_decompose in one kernel; the one-product tail with its addend's CRT in the same kernel
       GPQ_K_CRT_DECOMPOSE, GPQ_K_TAIL_STREAM,
       // gpq_he_rot_hoisted: the key switch of one rotation from the shared NTT-domain input (keyswitch_rot_mid8x2, two-pass rings); the plain
       // permutation of that input on single-pass rings (automorphism_gather)
       GPQ_K_KEYSWITCH_ROT_MID, GPQ_K_AUTOMORPHISM_GATHER,
       // planned he_gemv: the inner sum of one giant step in the NTT domain (gemv_mac)
       GPQ_K_GEMV_MAC,
       // he_ecd on the device: one workgroup per slot vector (he_ecd_lds, ecd_kernels.hpp)
       GPQ_K_ECD,
       // he_dcd on the device: one workgroup per plaintext (he_dcd_lds, dcd_kernels.hpp)
       GPQ_K_DCD,
       // samplers and encryption on the device (enc_kernels.hpp): the byte-fed samplers; small_to_rns_k / small_to_big_k / enc_tail_k
       GPQ_K_SAMPLE, GPQ_K_ENC,
       // gpq_he_genswk_batch: the CRT recombination of a switching key mod P 2^k (genswk_crt_tail, genswk_kernels.hpp)
       GPQ_K_GENSWK_TAIL,
       // the reference's deterministic randombytes by position (surf_stream_k, rng_kernels.hpp): a class of its own, so that the samplers' times stay theirs
       GPQ_K_RNG,
       // gpq_he_gemv_multi: one giant step's inner sums for several plans on the same ciphertexts (gemv_mac_multi)
       GPQ_K_GEMV_MAC_MULTI,
       // constant plaintexts (constpt_kernels.hpp): he_mulpt [+ he_rs] and he_addpt / he_subpt by a + b x^(n/2) as one pass over the big slabs
       GPQ_K_MULPT_CONST, GPQ_K_ADDPT_CONST,
       // the additive glue of the evaluators (algo_kernels.hpp): up to three signed terms, a constant plaintext and one mpi_smod in one pass
       GPQ_K_LIN_CONST, GPQ_K_COUNT };

// Constant matrix of the matrix-core CRT fast path for one basis and result width WL (bridge_mfma.hpp)
struct gpq_recon_mfma {
  gpq_dev<void> d_bfrag;
  gpq_dev<uint64_t> d_lk, d_kc, d_pm;
  unsigned KS = 0;
  size_t lds_bytes = 0;
};

// CRT constants of one prefix of the prime chain (bridge_tables.hpp)
struct gpq_bridge_basis {
  unsigned first = 0, dim = 0, pbits = 0;
  int WP = 0;
  gpq_dev<uint64_t> d_phat, d_phat_inv, d_pmult, d_phalf, d_inv128;
  std::vector<uint64_t> h_phat_inv;
  std::vector<uint64_t> h_P;          // the product itself, little-endian words
  std::vector<uint64_t> h_phat;       // [dim][WP]
  std::map<int, gpq_recon_mfma> mfma; // by result width WL
  gpq_dev<gpq::LimbTab> d_tabs_scaled;     // the context's LimbTab array with n^-1 * (P/p_d)^-1 for the limbs of this basis (get_scaled_tabs, bridge_tables.hpp)
};

// Constant matrix of the matrix-core rns_decompose for (first limb, limbs, words) (bridge_mfma.hpp)
struct gpq_decomp_mfma {
  gpq_dev<void> d_bfrag;
  gpq_dev<uint64_t> d_pk;
  unsigned NT = 0, KS = 0;
  size_t lds_bytes = 0;
};

// P^-1 mod p_d for the limbs above a P of dimP limbs (exact division in he_relin / he_swk)
struct gpq_relin_tables {
  gpq_dev<uint64_t> d_pinv;
  // bridge_relin_front_mfma (bridge_mfma.hpp): constant matrix and per-limb tables, built on first use
  bool front_tried = false;
  gpq_dev<void> d_bfrag;
  gpq_dev<uint64_t> d_lk, d_pk, d_tkp, d_kf;
  unsigned NT = 0, KS = 0;
  size_t lds_bytes = 0;
  // the same tables for limbs that arrive multiplied by w_j = P^-1 (Pi'/p_j)^-1, and the per-limb table that makes the key switch's
  // inverse pass deliver them so (bridge_tables.hpp: get_relin_front; bridge_tail.hpp: tail_prescale_mode)
  gpq_dev<void> d_bfrag_w;
  gpq_dev<uint64_t> d_pk_w, d_tkp_w;
  gpq_dev<gpq::LimbTab> d_tabs_w;
  // the one-product tail (bridge_tables.hpp: get_tail_direct): constant matrix of floor(Pi' 2^104 / p_d) over all dimB limbs, the per-limb table that
  // makes the key switch deliver CRT-weighted limbs (owned by the basis), the weights and their inverses for bridge_limb_scale
  bool direct_tried = false;
  gpq_recon_mfma direct;
  std::map<unsigned, gpq_recon_mfma> direct_padded;   // the same matrix zero-padded to KS k steps (bridge_stream.hpp's instantiations)
  const gpq::LimbTab *d_tabs_direct = nullptr;     // (the basis owns it)
  gpq_dev<uint64_t> d_scale, d_unscale;
};

// Constants of gpq_he_genswk_batch for one (dimP, logqL): P, P^-1 mod 2^(64 W2), M = P 2^logqL, floor(M/2), M + floor(M/2) in ONE device block
// (bridge_genswk.hpp)
struct gpq_genswk_tables {
  gpq_dev<uint64_t> d_const;
  unsigned WPw = 0, W2 = 0, LM = 0, nbits = 0, dimmul = 0;   // words of P, of 2^logqL, of the three multiples of M; bits of M; src/he-kem.c:83
  const uint64_t *P = nullptr, *Pinv = nullptr, *M = nullptr, *Mh = nullptr, *M3h = nullptr;   // into d_const
};

// Everything a context builds once and only reads afterwards on the device: the transform tables of upload_tables (engine.hip) and the bridge
// constants bridge_tables.hpp builds at first use.  ONE object per prime chain, held through a shared_ptr: a context's peer lane (gpq_ctx_clone)
// shares its parent's, so the second lane costs no table memory, no table-building time, "the peer's tables differ" is not a state the library
// can be in, and the tables live until the last of the two is gone, in whichever order they go.  Built and read by the one host thread that
// drives the context (single caller); uploads are synchronous hipMemcpy, so a launch on either lane's stream that follows a build
// on the host sees the table.  Every device pointer in it is a gpq_dev: the cache's destructor is the only release there is, and a builder
// enters its struct into a map only once every upload has succeeded.
struct gpq_table_cache {
  size_t device_bytes = 0;            // read-only device memory behind this cache (gpq_dev::upload); first: the owners below take their bytes off it as they go
  // transform tables (standard form); the contexts that share the cache read them through plain pointers of the same names
  gpq_dev<uint64_t> d_w, d_winv;
  gpq_dev<gpq::TwS> d_ws, d_winvs;    // split-twiddle pairs for the first nsplit_tables limbs (modarith.hpp)
  gpq_dev<gpq::LimbTab> d_tabs;
  std::vector<gpq::LimbTab> h_tabs;   // host copy (bridge_tables.hpp derives tables with pre-scaled n^-1 from it)
  std::map<std::pair<unsigned, unsigned>, gpq_bridge_basis> bases;   // by (first limb, count), built on first use
  std::map<std::pair<unsigned, unsigned>, gpq_relin_tables> relins;  // by (dimP, dimB)
  std::map<std::pair<std::pair<unsigned, unsigned>, unsigned>, gpq_decomp_mfma> decomps;  // by ((first limb, limbs), W)
  gpq_dev<uint16_t> d_error_table;    // gpq_sample_error's 65536 coefficient pairs (enc.hip), uploaded at first use
  std::map<std::pair<unsigned, unsigned>, gpq_genswk_tables> genswk;  // by (dimP, logqL)
  // Scaled per-limb tables (get_scaled_tabs, get_relin_front) one of whose split pairs fails the wide class's table check (modarith.hpp:
  // split_entry_fits_wide), with the first such limb: a context that reads the table runs that limb and those after it in the split class
  // (bridge_tables.hpp: apply_scaled_wide_limit).  Empty for every chain met so far (the failing constants are ~100 values in 2^59).
  std::map<const gpq::LimbTab *, unsigned> scaled_wide_limit;
};

// The switches that decide which kernels a call runs.  A member that decides which kernels a call runs belongs HERE: the peer lane follows the
// context it serves by one assignment (gpq_peer_lane: q->set = c->set), so a switch kept elsewhere would let the two lanes run different kernels
// -- both bit-exact, which no parity test notices.
struct gpq_settings {
  unsigned chunk = 32; // polynomials per fused launch group (measured: larger groups amortise launch tails; profiles/r01/v9_sweep_chunk.txt)
  unsigned limb_block = 0; // limbs per fused launch group (0 = all limbs of the slab); gpq_set_limb_block
  unsigned nsplit = 0;                // leading limbs that run the split-twiddle butterflies (c < GPQ_SPLIT_CMAX)
  unsigned nwide = 0;                 // leading limbs with c < GPQ_WIDE_CMAX (<= nsplit): forward stages as ct_bfly_wide
  bool bridge_mfma = true;            // matrix-core decompose / CRT (gpq_set_bridge_mfma(ctx, 0): the integer-VALU kernels)
  bool lazy_decompose = true;         // gpq_he_mul's own rns_decompose output in (0, 3p): the forward transforms take it (gpq_set_lazy_decompose)
  unsigned debug_force_redo = 0;      // tests (gpq_debug_force_redo)
  int nt_mode = -1;                   // slab traffic of the transform kernels with the nt cache policy: -1 by working set (nt_for), 0 never, 1 always
  bool stream_bridge = true;          // gpq_he_mul / gpq_he_swk: bridge_stream.hpp's fused streaming kernels (gpq_set_stream_bridge(ctx, 0): round 3's separate kernels)
  bool exact_crt = false;             // force the exact CRT kernel (tests)
  bool prescale = true;               // gpq_he_mul / gpq_he_swk: inverse passes write limbs pre-multiplied by (P/p_d)^-1 for the CRT kernels (gpq_set_prescale)
  bool prescale_upper = true;         // ... and the limbs above P by w_j for the relinearisation front
  bool tail_direct = true;            // ... or every limb by the weights of the whole basis: the relinearisation tail as ONE product (bridge_tables.hpp: get_tail_direct)
};

// Every device allocation, stream and event below is an owner: `delete` releases all a context holds, in any order.
struct gpq_ctx {
  int device = 0;
  unsigned logn = 0, n = 0, nprimes = 0;
  gpq_settings set;
  // host copies in the reference's own representation (struct rns_ctx, src/poly.h:28-41)
  std::vector<uint64_t> p, pinv_mont, pinv_barr, ninv_mont, psi;
  std::vector<uint64_t> zetas, zetas_inv;  // [nprimes][n], Montgomery form, bit-reversed index
  std::shared_ptr<gpq_table_cache> cache;  // the read-only tables: the transform tables and the lazily built bridge constants
  bool tables_borrowed = false;            // a peer lane: the cache is its parent's too (gpq_debug_table_bytes counts it once, for the parent)
  // the cache's transform tables, not owned
  const uint64_t *d_w = nullptr, *d_winv = nullptr;
  const gpq::TwS *d_ws = nullptr, *d_winvs = nullptr;
  const gpq::LimbTab *d_tabs = nullptr;
  unsigned nsplit_tables = 0;                     // for how many limbs the split pair tables exist (gpq_set_limb_classes can only lower nsplit)
  bool low9 = false;                              // n = 2^17: strided passes over 512-coefficient rows, 9 low stages (Lane8<9>)
  unsigned nwide_max = 0;                         // the most set.nwide may be
  gpq_dev<unsigned char> d_redo;      // per-coefficient "redo exactly" flags of the fast CRT path (its capacity: d_redo.bytes)
  std::vector<gpq_dev<void>> retired; // outgrown scratch (gpq_dev::grow): a HIP graph captured earlier may still use it, so it lives as long as the context
  gpq_dev<unsigned> d_wave_any;       // one word per wave of the last bridge_stream.hpp launch: did it flag a coefficient (FlagScope)
  // gpq_he_mul / gpq_he_swk over more than one launch group: every other group runs on a second stream through a PEER context (the parent's
  // read-only tables; its own scratch and flag words: nothing mutable is shared), so that the HBM-bound bridge kernels of one group run beside the issue-bound transforms
  // of the other and launch tails fill (gpq_set_overlap; bridge.hip: peer_lane).  The caller's stream orders the whole call as before.
  int overlap = -1;                   // gpq_set_overlap: -1 (default) = two lanes when the peer's workspace is affordable (kPeerAutoWorkspaceBytes), 0 = never, 1 = always
  bool peer_failed = false;           // the peer (its stream, events, flag words) could not be created once: one lane from then on
  size_t peer_ws_declined = 0;        // a peer workspace of this many bytes could not be allocated: shapes that need as much or more run on one lane, smaller ones still get two
  int debug_peer_fail = 0;            // tests (gpq_debug_fail_peer): 1 = the next attempt to create the peer fails as an allocation would, 2 = the next workspace allocation does
  unsigned last_lanes = 1;            // lanes the last multi-group entry point ran on (gpq_last_lanes)
  std::set<unsigned long long> peer_warm;   // call shapes the peer has run outside a stream capture (gpq_lane_key)
  gpq_ctx *peer = nullptr;            // (gpq_ctx_destroy)
  gpq_stream_own peer_stream;
  gpq_event ev_fork, ev_join;
  gpq_dev<void> peer_ws;
  gpq_dev<void> d_ecd_hand;           // gpq_he_ecd with a plan of more than one block: 32 slots bytes per vector between its three kernels (ecd.hip: encode)
  gpq_dev<unsigned> d_zflag;          // per-(polynomial, limb) "output contains a residue 0" flags of gpq_ntt (tables.hpp); zero between calls
  // gpq_debug_zero_watch: copies of the flag words of gpq_ntt's LAST launch group as the forward kernels left them (before ref_zero_redo) and
  // as ref_zero_redo left them (after), taken on the launch stream; [0, zwatch_cap) before, [zwatch_cap, 2 zwatch_cap) after
  gpq_dev<unsigned> d_zwatch;
  size_t zwatch_cap = 0, zwatch_count = 0;
  // profiling
  bool prof_on = false;
  std::vector<gpq_prof_rec> prof;     // launches recorded since the last reset
  std::vector<gpq_event> prof_pool;   // recycled events
};

// Makes `device` current for a scope and puts the caller's device back afterwards (context creation must not leave
// the calling thread on another GPU).
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int device) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(device); }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

template <typename T>
template <typename U>
int gpq_dev<T>::upload(gpq_ctx *c, const std::vector<U> &v) {
  DeviceScope on_device(c->device);
  hipError_t e = alloc(v.size() * sizeof(U));
  if (e == hipSuccess) {
    counted = &c->cache->device_bytes; *counted += bytes;
    e = hipMemcpy(p, v.data(), bytes, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) return GPQ_OK;
  reset();
  return gpq_fail(GPQ_ERR_HIP, "uploading a table of %zu bytes: %s", v.size() * sizeof(U), hipGetErrorString(e));
}
template <typename T>
void gpq_dev<T>::retire(gpq_ctx *c) {
  if (!p) return;
  gpq_dev<void> old;
  old.p = p; old.bytes = bytes; old.counted = counted;
  p = nullptr; bytes = 0; counted = nullptr;
  c->retired.push_back(std::move(old));
}
template <typename T>
int gpq_dev<T>::grow(gpq_ctx *c, hipStream_t s, size_t nbytes, bool zero_on_stream, const char *refusal) {
  if (gpq_capturing(s)) return gpq_fail(GPQ_ERR_INVALID, "%s", refusal);
  DeviceScope on_device(c->device);
  gpq_dev fresh;
  hipError_t e = fresh.alloc(nbytes);
  if (e == hipSuccess && zero_on_stream) e = hipMemsetAsync(fresh.p, 0, nbytes, s);
  if (e != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "scratch of %zu bytes: %s", nbytes, hipGetErrorString(e));
  retire(c);
  *this = std::move(fresh);
  return GPQ_OK;
}

// roctx range around a stage of the path (tracing).  The marker library is looked up at run time
// (librocprofiler-sdk-roctx / libroctx64, normally brought in by rocprofv3 --marker-trace); without it a range costs one
// pointer test.  Host-side ranges: they bracket the LAUNCHES of a stage, the kernels themselves appear in the kernel trace.
void gpq_range_push(const char *name);
void gpq_range_pop();
struct StageRange {
  explicit StageRange(const char *name) { gpq_range_push(name); }
  ~StageRange() { gpq_range_pop(); }
  StageRange(const StageRange &) = delete;
  StageRange &operator=(const StageRange &) = delete;
};

// Brackets one kernel launch (or a short run of them) with two events on its stream when profiling is on.
struct ProfScope {
  gpq_ctx *c; hipStream_t s; gpq_prof_rec r; bool on;
  ProfScope(const gpq_ctx *cc, int kernel, hipStream_t st) : c(const_cast<gpq_ctx *>(cc)), s(st), on(cc->prof_on) {
    if (!on) return;
    auto get = [&]() { gpq_event e; if (!c->prof_pool.empty()) { e = std::move(c->prof_pool.back()); c->prof_pool.pop_back(); } else (void)hipEventCreate(&e.h); return e; };
    r.kernel = kernel; r.a = get(); r.b = get();
    (void)hipEventRecord(r.a, s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(r.b, s);
    c->prof.push_back(std::move(r));
  }
  ProfScope(const ProfScope &) = delete;
  ProfScope &operator=(const ProfScope &) = delete;
};

// A second context over the same primes for the peer lane: every read-only device table (twiddles, split pairs, LimbTab, the bridge's constant
// cache) is the parent's, shared (gpq_table_cache); its own are only the mutable words (zero flags, redo flags, wave words, scratch).  Default settings, no
// peer of its own.
int gpq_ctx_clone(const gpq_ctx *c, gpq_ctx **out);
// Hoisted rotations (engine.hip; bridge.hip's gpq_he_rot_hoisted): the complete forward transform of `polys` polynomials of `dim` limbs
// in place (slab[k][d][i], canonical in [0, p], no zero watch: only products with a key read it), and the key switch of one rotation
// from it: c0 = invntt(X o sigma_g (*) evk0), c1 = invntt(X o sigma_g (*) evk1), the inverse pass reading `inv_tabs`.
// `workspace`: gpq_keyswitch_workspace_bytes(c, dim, polys) (single-pass rings only).
int gpq_hoist_forward(gpq_ctx *c, uint64_t *slab, unsigned dim, unsigned polys, hipStream_t s);
int gpq_keyswitch_rotated(gpq_ctx *c, uint64_t *c0, uint64_t *c1, const uint64_t *X, const uint64_t *evk0, const uint64_t *evk1,
                          unsigned dim, unsigned polys, unsigned g, void *workspace, hipStream_t s, const gpq::LimbTab *inv_tabs);
// gpq_he_mul_tensor / gpq_keyswitch with the per-limb table their inverse strided pass reads as an argument: nullptr = the context's own; else
// the same table with n^-1 (and winv[1] n^-1) multiplied by a CRT weight, so that the limbs leave the transform already scaled for the
// reconstruction that follows (bridge_tables.hpp: get_scaled_tabs).  A call that is handed such a table takes no lane of its own.
int gpq_he_mul_tensor_scaled(gpq_ctx *c, uint64_t *d0, uint64_t *d1, uint64_t *d2, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                             const uint64_t *b1, unsigned dim, unsigned batch, void *workspace, void *stream, const gpq::LimbTab *inv_tabs);
int gpq_keyswitch_scaled(gpq_ctx *c, uint64_t *c0, uint64_t *c1, const uint64_t *x, const uint64_t *evk0, const uint64_t *evk1, unsigned dim,
                         unsigned batch, void *workspace, void *stream, const gpq::LimbTab *inv_tabs);
// Planned he_gemv (engine.hip; bridge.hip's gpq_gemv_inner): acc0 / acc1[polys][dim][n] = the sums over `nterms` (rotation slot, diagonal)
// pairs (device array) of r0 / r1[slot][polys][dim][n] (*) diag[diagonal][dim][n], all in the NTT domain; canonical output, ONE launch.
int gpq_gemv_mac(gpq_ctx *c, uint64_t *acc0, uint64_t *acc1, const uint64_t *r0, const uint64_t *r1, const uint64_t *diag,
                 const void *terms, unsigned nterms, unsigned dim, unsigned polys, hipStream_t s);
// he_gemv for several plans on the same ciphertexts (engine.hip; gemv_multi.hpp's gpq_he_gemv_multi): the sums of gpq_gemv_mac for up to
// GPQ_GEMV_MULTI_NP plans in ONE launch that reads every rotation once.  r0 / r1[union slot][polys][rdim][n]; entries (device) =
// nentries x (1 + NP) words: the union slot, then per plan its diagonal or 0xffffffff where the plan has no live diagonal on that slot.
// plans[t].dim = 0: nothing at position t (neither read nor written); else the plan's diagonals and sums lie over its own dim <= rdim limbs.
// (BT, NP) = (4, 2): 118 VGPRs, no scratch -- DESIGN.md, "he_gemv for several matrices", has the other instantiations.
#ifndef GPQ_GEMV_MULTI_BT
#define GPQ_GEMV_MULTI_BT 4
#endif
#ifndef GPQ_GEMV_MULTI_NP
#define GPQ_GEMV_MULTI_NP 2
#endif
struct gpq_gemv_multi_arg { const uint64_t *diag; uint64_t *acc0, *acc1; unsigned dim; };
int gpq_gemv_mac_multi(gpq_ctx *c, const gpq_gemv_multi_arg *plans, const uint64_t *r0, const uint64_t *r1, const unsigned *entries,
                       unsigned nentries, unsigned rdim, unsigned polys, hipStream_t s);
// gpq_he_dec (bridge.hip): r[k] = x[k] (*) key for `polys` polynomials of `dim` limbs and ONE key slab uint64_t[dim][n] shared by all of them
// (pointwise<true, true>: the second operand is read without the polynomial's offset); r may alias x.
int gpq_rns_mul_shared(gpq_ctx *c, uint64_t *r, const uint64_t *x, const uint64_t *key, unsigned dim, unsigned polys, hipStream_t s);

// Launches a kernel whose dynamic LDS may exceed 64 KB.  That needs the function attribute (ceiling `lds_max`), set once per (kernel, device):
// per kernel through the template argument -- one flag array per kernel address -- and per device through the calling thread's current one.
// The flags are atomics because host threads that drive contexts on different devices meet here; a context and its peer still belong to one
// thread at a time (include/gpqhe_hip.h).  Two threads that find a flag clear both set the attribute, to the same value.
template <auto Kernel, typename Args>
int gpq_launch_lds(int lds_max, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &a) {
  static std::atomic<bool> raised[64] = {};
  int d = -1;
  hipError_t e = hipGetDevice(&d);
  const bool known = e == hipSuccess && d >= 0 && d < 64;
  if (e == hipSuccess && !(known && raised[d].load(std::memory_order_acquire))) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (e == hipSuccess && known) raised[d].store(true, std::memory_order_release);
  }
  if (e != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "dynamic LDS limit of a kernel: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
  return GPQ_OK;
}

// ---------------------------------------------------------------------------
// Two launch groups in flight (gpq_set_overlap).  A call over more than one launch group hands every other group to the context's PEER -- a
// second context over the same primes (the parent's read-only tables by pointer; own scratch and flag words: no mutable state is shared) on a second stream -- by calling the same
// entry point on it for that group's slice of the batch.  Launch tails of one lane fill with the other's work, and the bridge kernels of one
// group (HBM-bound) meet transforms of the other (issue-bound): +3.5 ... +4 % whole he_mul at the headline shape, +12 % at the reference's
// default shape (profiles/r04/v13_two_lanes_ab.txt).  The caller's stream still orders the call as a whole: the peer's stream waits for an
// event recorded on it at entry, and it waits for the peer's last launch before the call returns.  Not taken while profiling (the breakdown
// is that of one stream), for a single group, or when a stream capture would have to allocate.
// ---------------------------------------------------------------------------
struct PeerLane {
  gpq_ctx *c = nullptr;
  hipStream_t s = nullptr;
  void *ws = nullptr;
  // set once the peer stream has been forked off the caller's: the lane is joined on EVERY exit path of the call (an early `return rc` inside the
  // group loop must not leave queued peer work unordered against the caller's stream, nor a stream capture with an unjoined fork)
  gpq_ctx *owner = nullptr;
  hipStream_t caller = nullptr;
  PeerLane() = default;
  PeerLane(const PeerLane &) = delete;
  PeerLane &operator=(const PeerLane &) = delete;
  inline int join();
  ~PeerLane() { (void)join(); }
};
// What gpq_set_overlap(ctx, -1) -- the default -- allows the peer's per-group workspace to cost.  Two lanes pay through launch tails, so the gain
// shrinks as the kernels of a group grow: +10-15 % at the reference's default shape (logn 14: 0.1 GB per group) on every device measured,
// +0.15 ... +3.9 % by device at the headline shape (5.6 GB per group), +1.6 % for he_swk at n = 2^17 (7 GB); never a loss (profiles/r04/v13_two_lanes_ab.txt,
// BENCH_r04.json, profiles/r05).  The cost is device memory: this workspace (the tables are shared with the parent since round 6).
constexpr size_t kPeerAutoWorkspaceBytes = (size_t)16 << 30;
// lane->c stays null when the call runs on the caller's stream alone.  `key` names the call shape (entry point, dimensions, group size): a lane is
// only taken inside a stream capture when the peer has already run that very shape outside one (first-use table builds allocate and copy).
// `bytes(ctx)` = the workspace one launch group needs (evaluated on the context itself: the peer shares its tables and follows its settings).  A
// peer that cannot be created is not an error of the call: the HIP error is cleared, the context stops trying, and the call runs on one lane; a
// WORKSPACE that cannot be allocated declines shapes of that size only.
template <typename Bytes>
int gpq_peer_lane(gpq_ctx *c, hipStream_t s, unsigned long long key, Bytes bytes, PeerLane *lane) {
  if (c->overlap == 0 || c->peer_failed || c->prof_on) return GPQ_OK;
  bool query_failed = false;
  const bool capturing = gpq_capturing(s, &query_failed);
  if (query_failed) { (void)hipGetLastError(); return GPQ_OK; }
  if (capturing && (!c->peer || !c->peer_warm.count(key))) return GPQ_OK;     // (before bytes(): sizing a new shape may build tables, which allocates)
  // The price first, on the context itself (the peer runs the same settings over the same tables): a shape the auto mode declines, or one whose
  // workspace already failed to allocate, never creates the peer and costs nothing.
  const size_t need = bytes(c);
  if (!need) return GPQ_OK;
  if (c->overlap < 0 && need > kPeerAutoWorkspaceBytes) return GPQ_OK;        // auto: not at this price
  if (c->peer_ws_declined && need >= c->peer_ws_declined) return GPQ_OK;      // this size did not fit once
  auto give_up = [&](const char *what) {                                       // one lane from now on, for this context
    (void)hipGetLastError();
    c->peer_failed = true;
    fprintf(stderr, "gpqhe_hip: second lane unavailable (%s): this context continues on one lane\n", what);
    return (int)GPQ_OK;
  };
  if (!c->peer) {
    if (c->debug_peer_fail == 1) return give_up("gpq_debug_fail_peer");
    if (!c->peer_stream && hipStreamCreateWithFlags(&c->peer_stream.h, hipStreamNonBlocking) != hipSuccess) return give_up("hipStreamCreateWithFlags");
    if (!c->ev_fork && hipEventCreateWithFlags(&c->ev_fork.h, hipEventDisableTiming) != hipSuccess) return give_up("hipEventCreateWithFlags");
    if (!c->ev_join && hipEventCreateWithFlags(&c->ev_join.h, hipEventDisableTiming) != hipSuccess) return give_up("hipEventCreateWithFlags");
    if (gpq_ctx_clone(c, &c->peer) != GPQ_OK) { c->peer = nullptr; return give_up("peer context"); }   // last: a context with a peer has its stream and events
  }
  c->peer->set = c->set;                                                     // the peer follows the context it serves (gpq_settings)
  if (need > c->peer_ws.bytes) {
    if (capturing) return GPQ_OK;
    gpq_dev<void> fresh;
    if (c->debug_peer_fail == 2 || fresh.alloc(need) != hipSuccess) {         // this shape only: smaller ones keep their second lane, nothing else is given up
      (void)hipGetLastError();
      c->peer_ws_declined = need;
      fprintf(stderr, "gpqhe_hip: no room for a second lane's workspace of %zu bytes: shapes of this size run on one lane\n", need);
      return GPQ_OK;
    }
    c->peer_ws.retire(c);                                         // a graph captured earlier may still use it
    c->peer_ws = std::move(fresh);
  }
  hipError_t e = hipEventRecord(c->ev_fork, s);
  if (e == hipSuccess) e = hipStreamWaitEvent(c->peer_stream, c->ev_fork, 0);
  if (e != hipSuccess) return gpq_fail(GPQ_ERR_HIP, "forking the peer stream: %s", hipGetErrorString(e));
  if (!capturing) c->peer_warm.insert(key);
  lane->c = c->peer; lane->s = c->peer_stream; lane->ws = c->peer_ws; lane->owner = c; lane->caller = s;
  return GPQ_OK;
}
inline int PeerLane::join() {
  if (!c || !owner) return GPQ_OK;
  hipError_t e = hipEventRecord(owner->ev_join, s);
  if (e == hipSuccess) e = hipStreamWaitEvent(caller, owner->ev_join, 0);
  c = nullptr; owner = nullptr;
  return e == hipSuccess ? (int)GPQ_OK : gpq_fail(GPQ_ERR_HIP, "joining the peer stream: %s", hipGetErrorString(e));
}
// Polynomials (ciphertexts) per launch group of the multi-group entry points
inline unsigned gpq_group_size(const gpq_ctx *c, unsigned batch) { return batch < c->set.chunk ? batch : c->set.chunk; }
// The launch groups of a two-lane entry point: `batch` items in groups of `chunk` (gpq_group_size), every other group on the peer when the
// call gets a lane (gpq_peer_lane with the call's `key` and `bytes`).  own(k0, count) runs a group on the caller's context and stream;
// peer(lane, k0, count) is the SAME entry point on lane.c with lane.ws and lane.s for that group's slice of the batch -- with that entry's
// own checks and its last_lanes bookkeeping, which is why the call's own is recorded after the groups.  A body's error ends the call; the
// lane is joined on that path too (PeerLane's destructor).
template <typename Bytes, typename Own, typename Peer>
int gpq_launch_groups(gpq_ctx *c, hipStream_t s, unsigned batch, unsigned chunk, unsigned long long key, Bytes bytes, Own own, Peer peer) {
  int rc;
  PeerLane lane;
  if (batch > chunk && (rc = gpq_peer_lane(c, s, key, bytes, &lane))) return rc;
  for (unsigned k0 = 0; k0 < batch; k0 += chunk) {
    const unsigned count = batch - k0 < chunk ? batch - k0 : chunk;
    if ((rc = lane.c && ((k0 / chunk) & 1) ? peer(lane, k0, count) : own(k0, count))) return rc;
  }
  const unsigned lanes_used = lane.c ? 2u : 1u;
  if ((rc = lane.join())) return rc;
  c->last_lanes = lanes_used;
  return GPQ_OK;
}
inline unsigned long long gpq_lane_key(unsigned entry, unsigned a, unsigned b, unsigned c3, unsigned d, unsigned e) {
  unsigned long long h = 0xcbf29ce484222325ull;
  for (unsigned v : {entry, a, b, c3, d, e}) { h ^= v; h *= 0x100000001b3ull; }
  return h;
}

