/*
 * gpqhe_hip.h -- C ABI of libgpqhe_hip.so, the MI355X engine behind GPQHE's
 * RNS/NTT hot path.  Plain C: pointers, sizes, opaque handles; no HIP or
 * torch types (a hipStream_t travels as void*).
 *
 * Two groups of entry points:
 *
 *  (1) Reference-named drop-in symbols (gpqhe_hip_compat.h): `ntt`, `invntt`,
 *      `poly_rns_mul`, `poly_rns_add`, `montgomery_*`, `barrett_*` with the
 *      reference's exact signatures (host pointers, one limb, synchronous),
 *      plus the north-star aliases `poly_ntt`, `poly_invntt`.
 *
 *  (2) The slab API below: whole limb-major slabs `uint64_t[batch][dim][n]`
 *      resident in HBM, asynchronous on a caller-supplied stream.  These are
 *      what the reference's limb loops (src/poly.c:96-103, src/he-mult.c:
 *      116-138 and :58-66, src/he-automorphism.c:59-67) become once the loop
 *      body is a kernel launch instead of a per-limb function call.
 *
 * Value contract (same as the reference): inputs are
 * canonical residues < p_d, outputs canonical; forward output order is the
 * reference's bit-reversed order; slab element (d, i) lives at d*n + i
 * (src/poly.c:99, src/rns.c:67).
 *
 * Concurrency: like the reference (SURVEY.md 8b "Threading: none") a context serves one caller at
 * a time: calls on one context must be issued to one stream at a time (the context owns small
 * scratch that successive launches reuse in stream order).  Use one context per stream otherwise.
 *
 * Errors: the slab API returns GPQ_OK or a negative code and records a
 * message (gpq_last_error); it never aborts.  The drop-in symbols keep the
 * reference's convention: void return, errno=EINVAL + message + abort() on
 * misuse (src/reduce.c:95-100).
 */
#ifndef GPQHE_HIP_H
#define GPQHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPQ_OK 0
#define GPQ_ERR_INVALID (-1)     /* bad argument / unsupported ring size        */
#define GPQ_ERR_HIP (-2)         /* HIP runtime error, see gpq_last_error()      */
#define GPQ_ERR_UNSUPPORTED (-3) /* prime outside the 2^59+c family the kernels fold */
#define GPQ_ERR_NOMEM (-4)

typedef struct gpq_ctx gpq_ctx;

/* ---- context: replaces polyctx_init's RNS part ------------------------------
 * Builds the reference's prime chain and per-prime tables for ring degree
 * n = 2^logn and uploads them to `device`:
 *   primes      p_0 < p_1 < ..., next prime == 1 (mod 2n) above 2^59+1   src/precomp.c:358, :372-376
 *   constants   pinv_mont, pinv_barr, ninv                               src/precomp.c:246-248
 *   twiddles    psi = g^((p-1)/2n), g least primitive root; tables in
 *               bit-reversed order                                       src/precomp.c:206-242, :251-263
 * `nprimes` plays polyctx.dimub (src/precomp.c:357).  logn in [1,17].
 */
int gpq_ctx_create(gpq_ctx **out, unsigned logn, unsigned nprimes, int device);

/* Same, but adopting tables the caller already has in the reference's format
 * (struct rns_ctx fields p / zetas / zetas_inv, Montgomery form): what the
 * drop-in symbols use so that results follow the caller's tables exactly. */
int gpq_ctx_create_from_tables(gpq_ctx **out, unsigned logn, unsigned nprimes, const uint64_t *primes,
                               const uint64_t *const *zetas_mont, const uint64_t *const *zetas_inv_mont, int device);
void gpq_ctx_destroy(gpq_ctx *ctx);

unsigned gpq_ctx_logn(const gpq_ctx *ctx);
unsigned gpq_ctx_nprimes(const gpq_ctx *ctx);
int gpq_ctx_device(const gpq_ctx *ctx);
/* Per-prime constants exactly as the reference's struct rns_ctx holds them
 * (src/poly.h:28-41): which = 0 p, 1 pinv_mont, 2 pinv_barr, 3 ninv, 4 psi. */
uint64_t gpq_ctx_const(const gpq_ctx *ctx, unsigned d, int which);
/* Host copies of rns->zetas / rns->zetas_inv (Montgomery form), n entries. */
const uint64_t *gpq_ctx_zetas(const gpq_ctx *ctx, unsigned d, int inverse);

/* polyctx.dimub for a modulus of logq bits, src/precomp.c:357 (logqub=logq). */
unsigned gpq_dimub(unsigned logn, unsigned logq);

const char *gpq_last_error(void);

/* ---- device memory helpers (for hosts without another allocator) ---------- */
int gpq_malloc(void **dptr, size_t bytes);
int gpq_free(void *dptr);
int gpq_upload(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int gpq_download(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int gpq_copy(void *dst_dev, const void *src_dev, size_t bytes, void *stream);      /* device to device, same device */
int gpq_stream_sync(void *stream);
/* Stream-to-stream ordering without blocking the host: work queued on `waiter` AFTER this call starts only when everything queued on `on` BEFORE it
 * has finished.  With it a plain-C host pipelines sub-batches over three streams -- gpq_upload of k+1 | the stages of k | gpq_download of k-1 -- and the
 * full-duplex link carries uploads and downloads at once (PCIe-inclusive he_mul/s 302 -> 470 on one MI355X; tests/c/shard_host.c `pipe`). */
int gpq_stream_wait(void *waiter, void *on);
/* Several devices from one C program: gpq_malloc and gpq_stream_create act on the calling thread's current device
 * (gpq_set_device); a context belongs to the device given to gpq_ctx_create and is used with streams and buffers of that
 * device.  Independent ciphertexts shard over devices without any exchange (tests/c/shard_host.c). */
int gpq_device_count(void);
/* Yardstick for the HBM-bound kernels (bench.py `copy_rate`): a plain stream over `bytes` (multiple of 16) with the library's own access shape --
 * 16 bytes per lane, `blocks` persistent workgroups of `threads` threads, `unroll` (1, 2, 4, 8) independent accesses in flight per lane.
 * kind 0: dst <- src, 1: read src only, 2: write dst only.  Device pointers; asynchronous on `stream`. */
int gpq_probe_stream(void *dst, const void *src, size_t bytes, int kind, unsigned blocks, unsigned threads, unsigned unroll, void *stream);
int gpq_set_device(int device);
int gpq_stream_create(void **stream);        /* non-blocking stream on the current device */
int gpq_stream_destroy(void *stream);
/* Page-locked host memory: gpq_upload / gpq_download from / to it are asynchronous DMA; with pageable memory the copies
 * are staged and a download waits for the work queued before it. */
int gpq_malloc_host(void **hptr, size_t bytes);
int gpq_free_host(void *hptr);
/* Host placement on a multi-socket node (no counterpart in the reference, which is single-threaded: SURVEY.md 8e).  A C host that drives several
 * GPUs runs one worker thread per device and calls gpq_bind_thread_to_device(device) as the thread's FIRST action -- before gpq_set_device -- so
 * that the thread, and the page-locked buffers it allocates next, sit on the socket the GPU hangs off.  Pure sysfs, no HIP call: HIP device i is
 * the i-th GPU node of /sys/class/kfd/kfd/topology/nodes whose render node this process can open, after ROCR_VISIBLE_DEVICES and HIP_VISIBLE_DEVICES
 * (integer lists); its CPUs are /sys/class/drm/renderD<minor>/device/local_cpulist.  Returns the number of CPUs the thread is now confined to, or 0
 * when nothing was changed (unknown topology, one memory domain, already confined, not allowed): never an error.
 * gpq_device_local_cpus only looks: the count and, in `cpulist`, the kernel's list text ("0-47,96-143"); `sysfs_root` NULL = "/" (tests hand it a
 * fake tree).  The rank processes of bench.py do the same in Python (gpqhe_amd/affinity.py) before their first HIP call. */
int gpq_bind_thread_to_device(int device);
int gpq_device_local_cpus(int device, const char *sysfs_root, char *cpulist, size_t cap);

/* ---- slab operations ------------------------------------------------------
 * All slabs are device pointers to uint64_t[batch][dim][n] using primes
 * 0..dim-1 of the context.  `stream` is a hipStream_t (NULL = default).
 * Kernels launch on the calling thread's CURRENT device, which must be the context's (gpq_set_device(gpq_ctx_device(ctx)));
 * a call from a thread on another device returns GPQ_ERR_INVALID instead of launching there.  A context and the calls on it
 * are not thread-safe: one host thread per context at a time -- and ONE STREAM per context at a time: a context carries scratch
 * that its launches share in stream order (gpq_ntt's zero flags, the per-coefficient redo flags and per-wave words of the bridge,
 * the table override of gpq_he_mul's inverse passes).  Work that should overlap on several streams uses one context per stream
 * (contexts of the same ring share nothing mutable; tools/ntt_stream_probe.py, tests/c/shard_host.c do exactly that).
 * A context and its peer lane (gpq_set_overlap) belong to ONE host thread at a time.  Threads that drive different contexts, one per
 * device, may call concurrently: the only state they share is the once-per-(kernel, device) LDS attribute flags, which are atomic.
 */

/* ---- stream classes: what `void *stream` promises, function by function -------------------------------------------------------
 * Every function below that takes a stream queues ALL its device work -- kernels, memsets, copies, the fork and join of a peer lane --
 * on that stream: nothing goes to the null stream, which a non-blocking stream (gpq_stream_create's, torch's side streams) does not
 * wait for.  Tables a call builds at first use are uploaded by host-synchronous copies BEFORE its first launch.  Beyond that there are
 * four classes; tests/stream_contract.py holds the same table, tests/test_stream_contract_cover.py fails when a prototype with a
 * `void *stream` is in none, and tests/test_stream_contract_gpu.py runs every call behind a delayed producer on a non-blocking side
 * stream and, where the class allows it, inside a captured and replayed graph.
 * CAPTURABLE: after ONE warm call of the same shape on the same context (first-use tables, scratch that grows with the batch, the
 *   dynamic-LDS attribute of a kernel, the peer lane) the call makes no host synchronisation, no allocation and no host read-back, so
 *   it may be captured into a graph and replayed; host arguments (rotation amounts, Galois elements, key pointer arrays, a seed, a
 *   stream position) are read before the call returns and are part of the captured launches:
 *     gpq_ntt gpq_invntt gpq_ntt_reference gpq_rns_mul gpq_rns_add gpq_poly_mul_rns gpq_mulpt_rns gpq_he_mul_tensor gpq_keyswitch
 *     gpq_rns_decompose gpq_rns_decompose_limbs gpq_rns_reconstruct gpq_poly_mul gpq_he_rs gpq_he_rescale gpq_he_mul gpq_he_mul_rs
 *     gpq_relin_tail gpq_relin_tail_overwriting gpq_big_transpose gpq_big_addsub gpq_big_add gpq_big_sub gpq_big_neg gpq_he_swk
 *     gpq_he_mulpt gpq_poly_rot gpq_poly_conj gpq_he_mulpt_const gpq_he_addpt_const gpq_he_rot_hoisted gpq_he_gemv gpq_gemv_inner
 *     gpq_he_gemv_planned gpq_he_gemv_multi gpq_he_ecd gpq_he_ecd_diagonals gpq_he_dcd gpq_he_dec gpq_sample_zo gpq_sample_error
 *     gpq_sample_uniform gpq_small_to_big gpq_he_enc_pk gpq_he_enc_sk gpq_surf_bytes gpq_rng_device_bytes gpq_evk_pack
 *     gpq_he_genswk_batch
 * ORDERED: the device work is ordered on `stream` as above, but every call may wait for `stream` on the host or allocate, so it is for
 *   eager use on any stream and never for a capture.  The general-modulus calls wait once per Barrett reduction (its constants are
 *   copied from a host buffer of the call), the plan constructors allocate the plan, read their measurement back and refuse a
 *   capturing stream with the error code for a bad argument:
 *     gpq_rns_reconstruct_general gpq_poly_mul_general gpq_he_rs_general gpq_relin_tail_general gpq_he_mul_general
 *     gpq_he_mulpt_general gpq_he_swk_general gpq_he_genswk gpq_gemv_plan_create gpq_gemv_plan_create_from_matrix
 * REFUSES_IN_CAPTURE: allocates and fills its tables by host-synchronous copies and queues nothing on `stream`, which it takes only
 *   to refuse a capturing one, before anything is allocated:
 *     gpq_gemv_multi_create
 * NOT_A_LAUNCH: a plain runtime operation on the stream, no kernel of a context and no scratch -- hipMemcpyAsync (gpq_upload,
 *   gpq_download, gpq_copy), hipStreamSynchronize (gpq_stream_sync), an event recorded on one stream and awaited by the other
 *   (gpq_stream_wait), hipStreamDestroy (gpq_stream_destroy), hipEventRecord (gpq_timer_start, gpq_timer_stop), and the copy-rate
 *   yardstick's one copy kernel (gpq_probe_stream).
 */

/* ntt / invntt over every limb of every polynomial, in place.
 * Replaces the per-limb calls `ntt(a, rns)` / `invntt(a, rns)`, src/ntt.c:37,54.
 * Inputs are canonical residues in [0, p_d) (what rns_decompose and poly_rns_mul produce); gpq_invntt also takes the word p_d for a
 * residue 0 -- the domain of the reference's invntt, and what gpq_ntt hands out -- so gpq_ntt's output goes straight into gpq_invntt
 * (tests/test_ntt_zero_repr_gpu.py: round trips and limbs that are p_d throughout, every kernel class).  Outputs are the reference's
 * words: gpq_invntt's are canonical; gpq_ntt's are canonical except that a residue 0 is stored as p_d wherever
 * src/ntt.c:47 stores it so (a sum leg x + t == p is kept as p, and survives while its partner's product is 0):
 * limbs whose output contains a zero are redone with the reference's own arithmetic (ref_zero_redo, ntt_kernels.hpp). */
int gpq_ntt(gpq_ctx *ctx, uint64_t *slab, unsigned dim, unsigned batch, void *stream);
int gpq_invntt(gpq_ctx *ctx, uint64_t *slab, unsigned dim, unsigned batch, void *stream);
/* src/ntt.c:37-52 (inverse = 0) or :54-73 executed as written on every limb, for ANY 64-bit input words (the reference's
 * unsigned wrap-around included): the slow kernel gpq_ntt redoes flagged limbs with, what the drop-in `ntt` / `invntt`
 * take for inputs outside [0, p), and an in-device cross-check of the two-pass kernels. */
int gpq_ntt_reference(gpq_ctx *ctx, uint64_t *slab, unsigned dim, unsigned batch, int inverse, void *stream);

/* r = a (*) b and r = a + b, coefficient-wise mod p_d; r may alias a or b.
 * Replace poly_rns_mul / poly_rns_add, src/poly.c:71-82 (decl src/poly.h:84-85). */
int gpq_rns_mul(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned dim, unsigned batch, void *stream);
int gpq_rns_add(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned dim, unsigned batch, void *stream);

/* Limb loop of poly_mul, src/poly.c:96-103 (without rns_decompose):
 * r = invntt(ntt(a) (*) ntt(b)).  a and b are distinct slabs and are overwritten (scratch: for n >= 2^13 the loop runs
 * as three kernels -- strided pass, fused low stages + product, strided pass -- and leaves them half transformed);
 * r may be a or b. */
int gpq_poly_mul_rns(gpq_ctx *ctx, uint64_t *r, uint64_t *a, uint64_t *b, unsigned dim, unsigned batch, void *stream);
/* Limb loop of he_mulpt, src/he-mult.c:179-185: r0 = invntt(ntt(m) (*) ntt(x0)), r1 = invntt(ntt(m) (*) ntt(x1)).
 * m, x0, x1 are distinct slabs and are overwritten; r0 / r1 may be x0 / x1. */
int gpq_mulpt_rns(gpq_ctx *ctx, uint64_t *r0, uint64_t *r1, uint64_t *m, uint64_t *x0, uint64_t *x1, unsigned dim, unsigned batch,
                  void *stream);

/* The fused operations process the batch in groups of `chunk` polynomials so
 * that the scratch stays bounded (default 32; larger groups amortise launch tails). */
int gpq_set_chunk(gpq_ctx *ctx, unsigned chunk);
/* ... and, inside a group of polynomials, in blocks of `limbs` limbs (0 = all limbs at once, the default): the three
 * kernels of a block run back to back, so a block of chunk x limbs x 7 slabs x n x 8 bytes that fits the 256 MiB
 * Infinity Cache is re-read from there instead of from HBM.  Results do not depend on either setting. */
int gpq_set_limb_block(gpq_ctx *ctx, unsigned limbs);
/* Butterfly classes (modarith.hpp): by default every limb runs the cheapest arithmetic its prime p = 2^59 + c admits --
 * the first limbs (c < 2^27) the wide-split butterflies, the limbs up to c < 2^29/3 the split-twiddle ones, the rest the
 * 7-multiply ones.  This call restricts the first two classes to the first `wide` / `split` limbs (clamped to what the
 * chain admits; (0, 0) = the general butterflies everywhere).  Results are bit-identical for every setting; it exists so
 * that each class can be run on every limb and compared (tests/test_ntt_gpu.py). */
int gpq_set_limb_classes(gpq_ctx *ctx, unsigned wide, unsigned split);

/* Bytes of scratch the two fused operations below need for this shape. */
size_t gpq_tensor_workspace_bytes(const gpq_ctx *ctx, unsigned dim, unsigned batch);
size_t gpq_keyswitch_workspace_bytes(const gpq_ctx *ctx, unsigned dim, unsigned batch);

/* Tensor stage of he_mul, src/he-mult.c:116-138 without the rns_decompose
 * calls: a0,a1,b0,b1 stand for the decomposed ct1.c0, ct1.c1, ct2.c0, ct2.c1;
 *   d0 = a0*b0, d2 = a1*b1, d1 = a0*b1 + a1*b0   (negacyclic, per limb).
 * Inputs are preserved.  Outputs may not alias inputs.  b0 == a0 and b1 == a1 (a squaring: he_mul(&ct, &ct, &ct, rlk),
 * src/he-algo.c:151) is recognised and runs two forward transforms instead of four; the results are the same residues. */
int gpq_he_mul_tensor(gpq_ctx *ctx, uint64_t *d0, uint64_t *d1, uint64_t *d2,
                      const uint64_t *a0, const uint64_t *a1, const uint64_t *b0, const uint64_t *b1,
                      unsigned dim, unsigned batch, void *workspace, void *stream);

/* Key-switch inner product of he_relin / he_swk, src/he-mult.c:58-66 ==
 * src/he-automorphism.c:59-67 without rns_decompose: x is the decomposed d2
 * (or d1); evk0/evk1 are ONE key's NTT-domain slabs uint64_t[dim][n] as built
 * by he_genswk (src/he-kem.c:103-110), shared by the whole batch.
 *   c0 = invntt(ntt(x) (*) evk0), c1 = invntt(ntt(x) (*) evk1).  x preserved. */
int gpq_keyswitch(gpq_ctx *ctx, uint64_t *c0, uint64_t *c1, const uint64_t *x,
                  const uint64_t *evk0, const uint64_t *evk1,
                  unsigned dim, unsigned batch, void *workspace, void *stream);

/* ---- MPI <-> RNS bridge ---------------------------------
 * The reference keeps coefficients as libgcrypt MPIs.  On the device a polynomial of
 * big integers is a "big slab": uint64_t[batch][W][n], word j of coefficient i at
 * j*n + i, little-endian words, two's complement over 64*W bits (centred
 * coefficients are signed).  The entry points with a `logq` / `logql` / `logDelta` argument are the
 * tuned ones for power-of-two moduli, as in every parameter set of the reference's tests
 * (tests/gpqhe.c:1349-1352, tests/polymul.c:84-87); the `*_general` entry points further down take
 * any modulus as little-endian words and any 64-bit Delta.
 */
unsigned gpq_big_words(unsigned bits);
/* rns->phat_invmp[d] of the node with `dim` limbs (src/precomp.c:288-289); bit length of its P. */
uint64_t gpq_ctx_phat_invmp(gpq_ctx *ctx, unsigned dim, unsigned d);
unsigned gpq_ctx_pbits(gpq_ctx *ctx, unsigned dim);

/* rns_decompose for every limb at once, src/rns.c:37-48: slab[k][d][i] = big[k][.][i] mod p_d (>= 0). */
int gpq_rns_decompose(gpq_ctx *ctx, uint64_t *slab, const uint64_t *big, unsigned W, unsigned dim, unsigned batch, void *stream);
/* The same for limbs first .. first+count-1 only (the reference's rns_decompose is per limb): slab[k][d][i], d < count. */
int gpq_rns_decompose_limbs(gpq_ctx *ctx, uint64_t *slab, const uint64_t *big, unsigned W, unsigned first, unsigned count,
                            unsigned batch, void *stream);
/* rns_reconstruct, src/rns.c:60-75, for ONE coefficient: `dim` reduced residues in host memory -> value in [0, P) as
 * Wout host words (64*Wout > bits of P).  Synchronous; the per-coefficient spelling of the reference, kept for its callers. */
int gpq_rns_reconstruct_one(gpq_ctx *ctx, uint64_t *words, unsigned Wout, const uint64_t *residues, unsigned dim);
/* poly_rns2mpi, src/poly.c:109-120, with q = 2^logq: rns_reconstruct (src/rns.c:60-75), centre
 * mod P, centre mod q.  logq = 0 stops after centring mod P (Wout must then hold P's bits + 1). */
int gpq_rns_reconstruct(gpq_ctx *ctx, uint64_t *big, unsigned Wout, const uint64_t *slab, unsigned dim, unsigned batch,
                        unsigned logq, void *stream);
/* gpq_rns_reconstruct takes a low-word fast path when q is a power of two shorter than P and redoes the
 * (rare) coefficients whose rounding it cannot decide with the exact full-width kernel; this forces the
 * exact kernel for everything (used by the tests to cross-check the two).
 * Reaches every call that reconstructs: gpq_rns_reconstruct itself, gpq_poly_mul, gpq_he_mulpt, gpq_he_dec, gpq_he_enc_pk / _sk, gpq_gemv_inner
 * and the plans' inner sums, and the relinearisation tail of gpq_he_mul / gpq_he_mul_rs / gpq_he_swk / gpq_he_rot_hoisted / gpq_he_gemv /
 * gpq_he_gemv_planned / gpq_he_gemv_multi, which then leaves the one-product tail for the matrix-core front.  Same words
 * (tests/test_settings_derived_gpu.py, tests/test_settings_bridge_calls_gpu.py). */
int gpq_set_exact_crt(gpq_ctx *ctx, int on);
/* gpq_he_mul / gpq_he_swk: 1 (default) = the bridge as streaming kernels (gpqhe_amd/csrc/bridge_stream.hpp): poly_rns2mpi(d2) -> rns_decompose
 * (src/he-mult.c:140, :59) in one kernel, and the relinearisation tail (:67-77) as one product that makes its addend d0 / d1 (:139, :141) from the
 * limbs on the spot -- d0, d1, d2 never exist as words; 0 = round 3's separate CRT, decompose and tail kernels.  Same words (the tests run both).
 * The streaming tail is also the tail of gpq_he_rot_hoisted, gpq_he_gemv, gpq_he_gemv_planned and gpq_he_gemv_multi (every rotation goes through it),
 * so the switch reaches them as it reaches gpq_he_swk; the CRT -> decompose kernel is gpq_he_mul's alone.  The calls without a key switch
 * (gpq_he_mulpt, gpq_poly_mul, gpq_he_dec, gpq_he_enc_*, gpq_he_genswk*, the gemv plans) do not read it. */
int gpq_set_stream_bridge(gpq_ctx *ctx, int on);
/* gpq_he_mul / gpq_he_swk / gpq_he_mul_tensor / gpq_keyswitch over more than one launch group (batch > gpq_set_chunk's group): with two LANES every
 * other group runs on a second, internal stream through an internal peer context, so that the launch tails of one group fill with the other's
 * kernels; the caller's stream still orders the call as a whole (work queued before it is waited for, work queued after it waits for both lanes).
 * `on` = -1 (default): two lanes when the peer's per-group workspace costs at most 16 GiB; 0: never; 1: always.  Same words either way.
 * COST: a workspace for one launch group (the size gpq_*_workspace_bytes reports for a batch of one group: 5.6 GB for gpq_he_mul at the headline
 * shape), allocated at the first multi-group call that will use it.  The peer borrows every read-only device table of the context (twiddles, split
 * pairs, per-limb constants, bridge constants: gpq_debug_table_bytes) and owns only its flag words and scratch.  GAIN: +10-15 % at the reference's default shape (logn 14) on every device measured; at the headline
 * shape it depends on the device (+0.15 % ... +3.9 %: a group's kernels are long, the lanes share one power cap); never a loss.  If the peer cannot
 * be created the context continues on one lane; if a workspace cannot be allocated, shapes of that size do (one line on stderr, no error).  Not taken while gpq_profile is on.
 * gpq_last_lanes: the lanes (1 or 2) the last such call on this context ran on.
 * Only gpq_he_mul, gpq_he_mul_rs, gpq_he_swk, gpq_he_mul_tensor and gpq_keyswitch split their groups over the lanes.  gpq_he_rot_hoisted and the
 * gpq_he_gemv family run their launch groups in order on the caller's stream (their inner gpq_he_swk calls see one group each); they give the
 * same words on a context with the setting on. */
int gpq_set_overlap(gpq_ctx *ctx, int on);
unsigned gpq_last_lanes(const gpq_ctx *ctx);
/* Tests: 1 = the next attempt to create the peer lane fails as an allocation would (the call runs on one lane, one line on stderr, and the context
 * stops trying); 2 = the next allocation of the peer's WORKSPACE fails (shapes that need that many bytes or more run on one lane from then on,
 * smaller ones keep two); 3 = stop failing but remember what was declined; 0 = back to normal (and the context may try again). */
int gpq_debug_fail_peer(gpq_ctx *ctx, int on);
/* Tests / accounting: read-only device memory (bytes) behind the context -- which = 0: the transform tables and every bridge constant built so far,
 * owned by the context; 1: what its peer lane owns of the same kind (0 by construction: the peer borrows); 2: 1 when a peer lane exists; 3: 1 when
 * every table pointer of the peer IS the context's. */
size_t gpq_debug_table_bytes(const gpq_ctx *ctx, int which);
/* gpq_he_mul: 1 (default) = its internal rns_decompose launches leave residues in (0, 3p), which the forward transforms behind them accept;
 * 0 = canonical residues.  Same results.  Read by gpq_he_mul / gpq_he_mul_rs and gpq_he_swk on two-pass rings (logn > 12), hence by the
 * single-rotation path of gpq_he_rot_hoisted and the giant steps of the gpq_he_gemv family, which are gpq_he_swk calls.  The hoisted decomposition
 * of gpq_he_rot_hoisted (two rotations or more), the plans and the calls without a key switch always produce canonical residues. */
int gpq_set_lazy_decompose(gpq_ctx *ctx, int on);
/* Cache policy of the slab loads / stores of the transform kernels (gpq_ntt, gpq_invntt, gpq_poly_mul_rns, gpq_mulpt_rns, gpq_he_mul_tensor,
 * gpq_keyswitch and everything built on them): -1 (default) = non-temporal when a launch group's slabs exceed the Infinity Cache (288 MiB is the
 * threshold), the default policy when they fit; 0 = never; 1 = always.  Never changes a word. */
int gpq_set_nt_policy(gpq_ctx *ctx, int mode);
/* Tests: the streaming kernels also flag every coefficient whose index is a multiple of `every` for the exact kernels behind them (0 = off).
 * The streaming kernels are gpq_he_mul's CRT -> decompose and the one-product tail, so this reaches the tail of gpq_he_mul / gpq_he_mul_rs /
 * gpq_he_swk / gpq_he_rot_hoisted / gpq_he_gemv / gpq_he_gemv_planned / gpq_he_gemv_multi where that tail runs; nothing else reads it. */
int gpq_debug_force_redo(gpq_ctx *ctx, unsigned every);
/* Tests (host only, no device needed): the check every split-twiddle pair (x, y) = (p - w, p - w 2^31 mod p) of a limb must pass before the limb
 * may run the wide-split butterflies -- for every multiplicand up to 8p - 1 the 92-bit sum of the split multiply, with its injected constant
 * 2^64 + 31c - 1, stays below 2^91.  1 = passes, 0 = fails (the limb and those after it take the split class), -1 = p is not a prime shape of
 * the wide class (2^59 < p < 2^59 + GPQ_WIDE_CMAX) or x, y > p. */
int gpq_debug_split_entry_fits_wide(uint64_t p, uint64_t x, uint64_t y);
/* Tests: the zero watch of gpq_ntt (the reference stores p, not 0, at some positions of a forward transform, src/ntt.c:45-48; the forward
 * kernels flag every (polynomial, limb) whose output holds a residue 0 and a kernel that executes src/ntt.c as written redoes those limbs).
 * With the watch on, each launch group of gpq_ntt leaves a copy of its flag words as the forward kernels wrote them and a copy as the redo
 * kernel left them; gpq_debug_zero_flags waits for the device and hands out both for the LAST launch group (word [polynomial * dim + limb];
 * `before` 1 = flagged, `after` all 0), returning the number of words of that group (at most `capacity` are written), -1 without a watch. */
int gpq_debug_zero_watch(gpq_ctx *ctx, int on);
long gpq_debug_zero_flags(gpq_ctx *ctx, unsigned *before, unsigned *after, size_t capacity);
/* gpq_he_mul / gpq_he_swk: the inverse transforms hand the kernels that follow limbs already multiplied by their CRT weights -- 3 (default): the key
 * switch's limbs carry the weights of its WHOLE basis and the relinearisation tail is one product (quotient, rounding and centring together);
 * 2: (P/p_d)^-1 on the limbs of each basis and w_j = P^-1 (Pi'/p_j)^-1 on the limbs above P for the relinearisation front; 1: the former only;
 * 0: neither.  Same results.  Two-pass rings (logn > 12) only; smaller rings never pre-multiply.  gpq_he_rot_hoisted makes the same choice
 * for its permuted key switch and tail (gpq_he_gemv, gpq_he_gemv_planned and gpq_he_gemv_multi rotate through it), and gpq_relin_tail_overwriting
 * takes the one-product tail only under 3.  The calls without a key switch do not read it. */
int gpq_set_prescale(gpq_ctx *ctx, int on);
/* rns_decompose is a product of the coefficients' bytes with a fixed matrix (256^k mod p_j) and runs on the matrix cores
 * (v_mfma_i32_32x32x32_i8, exact) by default; 0 selects the integer-VALU kernel instead (the tests cross-check the two).
 * 0 also turns off the matrix-core CRT sum of gpq_rns_reconstruct and the matrix-core tails (the relinearisation tail becomes the integer-VALU
 * one).  Every call that decomposes or reconstructs reads it: the gpq_he_mul / gpq_he_swk / gpq_he_rot_hoisted / gpq_he_gemv* family, gpq_he_mulpt,
 * gpq_poly_mul, gpq_he_dec, gpq_he_enc_*, gpq_he_genswk*, gpq_gemv_plan_create*.  Same words for all of them. */
int gpq_set_bridge_mfma(gpq_ctx *ctx, int on);

/* poly_mul, src/poly.c:84-107 (decl src/poly.h:86-87), q = 2^logq, on big slabs of W words. */
size_t gpq_poly_mul_workspace_bytes(const gpq_ctx *ctx, unsigned dim, unsigned batch);
int gpq_poly_mul(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned dim, unsigned logq,
                 unsigned batch, void *workspace, void *stream);
/* The same two for ANY modulus q (little-endian words q_words[0..Lq)): he_genswk calls poly_mul with
 * q = P*q_L (src/he-kem.c:95).  Second centring by multiword Barrett reduction; a key-generation path,
 * not tuned (Horner over Lq-word blocks, one Barrett step each). */
size_t gpq_poly_mul_general_workspace_bytes(gpq_ctx *ctx, unsigned dim, unsigned batch);
int gpq_rns_reconstruct_general(gpq_ctx *ctx, uint64_t *big, unsigned Wout, const uint64_t *slab, unsigned dim, unsigned batch,
                                const uint64_t *q_words, unsigned Lq, void *scratch, void *stream);
int gpq_poly_mul_general(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned dim,
                         const uint64_t *q_words, unsigned Lq, unsigned batch, void *workspace, void *stream);

/* he_rs, src/he-rescale.c:33-54 (decl src/gpqhe.h:136), Delta = 2^logDelta, q_l = 2^logql: c0, c1 of
 * `batch` ciphertexts in place: mpi_rdiv by Delta then mpi_smod q_l.  The l / nu / B bookkeeping
 * (:36-38) stays with the caller.  gpq_he_rescale is the north-star spelling of the same call. */
int gpq_he_rs(gpq_ctx *ctx, uint64_t *c0, uint64_t *c1, unsigned W, unsigned logDelta, unsigned logql, unsigned batch, void *stream);
int gpq_he_rescale(gpq_ctx *ctx, uint64_t *c0, uint64_t *c1, unsigned W, unsigned logDelta, unsigned logql, unsigned batch, void *stream);

/* Limb counts the reference derives from the modulus chain for q_L = 2^logqL, q_l = 2^logql:
 * dimP = hectx.dim (src/precomp.c:401; hectx.P is the product of the first dimP primes),
 * dimA = tensor stage of he_mul (src/he-mult.c:99), dimB = he_relin / he_swk (src/he-mult.c:51,
 * src/he-automorphism.c:52), dimevk (src/precomp.c:407).  Any output pointer may be NULL. */
int gpq_he_dims(gpq_ctx *ctx, unsigned logqL, unsigned logql, unsigned *dimP, unsigned *dimA, unsigned *dimB, unsigned *dimevk);

/* he_mul, src/he-mult.c:88-156 (decl src/gpqhe.h:147), on big slabs of W words with q_l = 2^logql:
 * decompose the four polynomials to dimA limbs, tensor stage, poly_rns2mpi of d0,d1,d2, then he_relin
 * (:40-85): decompose d2 to dimB limbs, key-switch with rlk (NTT-domain slabs of >= dimB limbs,
 * src/he-kem.c:103-110), c = rdiv(poly_rns2mpi(.), P) + d, centred mod q_l.  The l/nu/B bookkeeping
 * (:92-95) stays with the caller.  Outputs may not alias inputs. */
size_t gpq_he_mul_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch);
int gpq_he_mul(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
               const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
               unsigned logql, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);
/* he_mul followed by he_rs (src/he-mult.c:88-156, then src/he-rescale.c:33-54 with Delta = 2^logDelta and q_(l-1) = 2^(logql - logDelta)): the same words
 * as gpq_he_mul + gpq_he_rs(out_c0, out_c1, W, logDelta, logql - logDelta), with the rounding division applied by the relinearisation tail on the way
 * out (1 <= logDelta <= 63 and the streaming tail; every other case runs the two calls), so that the outputs are not read and written once more:
 * BASELINE configs[2] is "he_mul + he_rescale".  Workspace as gpq_he_mul. */
int gpq_he_mul_rs(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
                  const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
                  unsigned logql, unsigned dimA, unsigned dimB, unsigned dimP, unsigned logDelta, unsigned batch, void *workspace, void *stream);

/* The tail of he_relin / he_swk on its own, src/he-mult.c:67-77: chat = key-switch output slab of dimB
 * limbs, d = big slab added afterwards (NULL: none, as for c1 in he_swk):
 *   out = mpi_smod(mpi_addm(mpi_rdiv(poly_rns2mpi(chat, P*q_l), P), d, q_l), q_l),  q_l = 2^logql. */
size_t gpq_relin_tail_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimB, unsigned dimP, unsigned batch);
int gpq_relin_tail(gpq_ctx *ctx, uint64_t *out, const uint64_t *chat, const uint64_t *d, unsigned W, unsigned logql,
                   unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);
/* Big slabs between the kernels' layout (word j of coefficient i at j*n + i) and rows of W words per coefficient (i*W + j), the layout a host
 * fills or reads sequentially; to_rows = 0: rows -> words, 1: words -> rows.  n >= 64, dst != src, `batch` polynomials one after another. */
int gpq_big_transpose(gpq_ctx *ctx, uint64_t *dst, const uint64_t *src, unsigned W, unsigned batch, int to_rows, void *stream);
/* out = a + b (mode 0), a - b (mode 1), -a (mode 2; b unused) on `polys` big slabs of W words per coefficient (two's complement,
 * wrapping at 2^(64 W); out may alias a or b): the arithmetic of he_add / he_sub / he_addpt / he_subpt / he_neg before their mpi_smod
 * (src/he-add.c:32-140); gpq_he_rs with logDelta = 0 (or gpq_he_rs_general with delta = 1) is that mpi_smod. */
int gpq_big_addsub(gpq_ctx *ctx, uint64_t *out, const uint64_t *a, const uint64_t *b, unsigned W, unsigned polys, int mode, void *stream);
/* The same with `chat` given up as scratch (overwritten): the tail as ONE matrix-core product over all dimB limbs (what gpq_he_mul / gpq_he_swk use
 * internally, where the key switch already delivers CRT-weighted limbs); same results. */
int gpq_relin_tail_overwriting(gpq_ctx *ctx, uint64_t *out, uint64_t *chat, const uint64_t *d, unsigned W, unsigned logql,
                               unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);

/* he_swk, src/he-automorphism.c:40-85: key-switch d1 with swk and add d0 into c0, big slabs, q_l = 2^logql
 * (the rotation / conjugation permutations of src/poly.c:263-283 are the caller's). */
size_t gpq_he_swk_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimB, unsigned dimP, unsigned batch);
int gpq_he_swk(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *d0, const uint64_t *d1,
               const uint64_t *swk0, const uint64_t *swk1, unsigned W, unsigned logql, unsigned dimB, unsigned dimP,
               unsigned batch, void *workspace, void *stream);

/* he_mulpt, src/he-mult.c:159-196 (decl src/gpqhe.h:148): ciphertext times plaintext polynomial m on big slabs,
 * q_l = 2^logql, over `dim` limbs (the reference derives dim from log2(pt->nu), :169: caller's). */
size_t gpq_he_mulpt_workspace_bytes(const gpq_ctx *ctx, unsigned dim, unsigned batch);
int gpq_he_mulpt(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m,
                 unsigned W, unsigned logql, unsigned dim, unsigned batch, void *workspace, void *stream);
/* poly_rot / poly_conj, src/poly.c:263-283, on big slabs (r must not alias a): with gpq_he_swk they are he_rot / he_conj,
 * src/he-automorphism.c:87-115. */
int gpq_poly_rot(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, unsigned W, unsigned rot, unsigned batch, void *stream);
int gpq_poly_conj(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, unsigned W, unsigned batch, void *stream);

/* ---- constant plaintexts ("Constant plaintexts") ------------------------------------------------------------------
 * he_const_pt (src/he-encode.c:119-125) writes two integers, m[0] = a and m[n/2] = b, into a plaintext that is 0 elsewhere.  The product of
 * a ciphertext polynomial c with a + b x^h (h = n/2) in Z[x]/(x^n + 1) is the closed form
 *   v[k] = a c[k] - b c[k+h] (k < h),   v[k] = a c[k] + b c[k-h] (k >= h)
 * and the reference's he_mulpt returns smod(smod(v mod P, P), q_l), P = the product of the first `dim` primes: smod(v, q_l) exactly when
 * |v| < floor(P/2).  Inputs centred mod 2^logql (what every call of this library returns) give |v| <= (|a| + |b|) 2^(logql-1), so
 *   fits(a, b, logql, dim)  <=>  (|a| + |b|) 2^(logql-1) < floor(P_dim / 2)
 * is what the host can decide; with the reference's dim (src/he-mult.c:168) it holds for every |re|, |im| up to about n.  No workspace;
 * asynchronous on `stream` and capturable. */

/* he_const_pt's two integers (src/he-encode.c:119-125) for Delta = 2^logDelta, where every step of the reference's
 * expression is exact: round-half-away-from-zero of re * 2^logDelta and im * 2^logDelta.  GPQ_ERR_INVALID if either
 * is not finite or does not fit int64_t.  Host only, no device call. */
int gpq_const_pt(double re, double im, unsigned logDelta, int64_t *a, int64_t *b);

/* 1 when the constant path gives he_mulpt's words for inputs centred mod 2^logql on `dim` limbs (condition above), else 0 */
int gpq_he_mulpt_const_fits(const gpq_ctx *ctx, int64_t a, int64_t b, unsigned logql, unsigned dim);

/* he_mulpt (src/he-mult.c:159-196) by the plaintext a + b x^(n/2), then -- logDelta != 0 -- he_rs (src/he-rescale.c:33-54):
 * the words of gpq_he_mulpt [+ gpq_he_rs(W, logDelta, logql - logDelta)] for centred inputs.  !fits -> GPQ_ERR_INVALID,
 * outputs untouched.  out may be the input of the same polynomial; no other overlap.  bad_dev: NULL or a device counter, to which
 * the call adds the number of input coefficients that are not centred mod 2^logql (the outputs are the closed form regardless).
 * 1 <= logql <= 64 W, logDelta < logql.  One launch for logDelta <= 63; beyond, the plain product followed by gpq_he_rs. */
int gpq_he_mulpt_const(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1,
                       int64_t a, int64_t b, unsigned W, unsigned logql, unsigned dim, unsigned logDelta,
                       unsigned batch, unsigned *bad_dev, void *stream);

/* he_addpt (sub = 0) / he_subpt (sub = 1) with that plaintext, src/he-add.c:80-123, any W-word inputs: one launch.  In place allowed. */
int gpq_he_addpt_const(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1,
                       int64_t a, int64_t b, int sub, unsigned W, unsigned logql, unsigned batch, void *stream);

/* ---- hoisted rotations and he_gemv --------------------------------------------------------------------------------------------
 * sigma of the automorphism X -> X^g (g odd) in the NTT domain, in the reference's forward output order (bit-reversed):
 *   NTT(poly_rot(a, rot))[j] = NTT(a)[idx[j]] (mod p) with g = 5^rot mod 2n (g = 2n - 1 for poly_conj), where
 *   2 brv(idx[j]) + 1 = (2 brv(j) + 1) g (mod 2n), brv = logn-bit reversal.  Host only (no device); idx holds n = 2^logn words.
 *   GPQ_ERR_INVALID for an even g or logn outside [1, 17]. */
int gpq_automorphism_index(unsigned logn, uint64_t g, uint32_t *idx);
/* he_rot (src/he-automorphism.c:101-115) of the same `batch` ciphertexts by rots[0..nrot): for every r the words of gpq_poly_rot on c0 and
 * c1 followed by gpq_he_swk with the key rk0[r] / rk1[r] (host arrays of device pointers, NTT-domain keys of >= dimB limbs), q_l = 2^logql.
 * c1 is decomposed and transformed once per launch group and every rotation permutes that transform ("Hoisted rotations").
 * Outputs are rotation-major: ciphertext k of rotation r at (r * batch + k) * W * n.  Any rot (0, repeats, >= slots); nrot = 1 runs
 * poly_rot + gpq_he_swk.  GPQ_ERR_INVALID when an output overlaps the other output or an input. */
size_t gpq_he_rot_hoisted_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimB, unsigned dimP, unsigned nrot, unsigned batch);
int gpq_he_rot_hoisted(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1,
                       const unsigned *rots, const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned nrot,
                       unsigned W, unsigned logql, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);
/* he_gemv, src/he-algo.c:47-93, followed by its he_rs (Delta = 2^logDelta; logDelta = 0: no rescale): n1, n2 as :51-54; diag[i n1 + j]
 * = the plaintext big slab (W words) of he_ecd(zrotdiag(A, i n1 + j, -i n1)), shared by the batch; rk0 / rk1 indexed by the rotation
 * (rk[j] for the baby steps, rk[i n1] for the giant ones); dimpt = he_mulpt's limb count (src/he-mult.c:168).  The output is centred
 * mod 2^(logql - logDelta); the l / nu / B bookkeeping stays with the caller.  out may alias c0 / c1. */
size_t gpq_he_gemv_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned slots, unsigned dimB, unsigned dimP, unsigned dimpt, unsigned batch);
int gpq_he_gemv(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *diag,
                const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned slots, unsigned W, unsigned logql,
                unsigned logDelta, unsigned dimB, unsigned dimP, unsigned dimpt, unsigned batch, void *workspace, void *stream);

/* ---- he_gemv with a plan: a FIXED matrix applied to many ciphertexts ("Planned he_gemv") --------------------------------
 * A plan holds the matrix's diagonals once, decomposed and forward-transformed, and the inner sum of a giant step is accumulated in the
 * NTT domain (gemv_mac): one inverse transform and one reconstruction per ciphertext polynomial and giant step instead of n1, and no
 * per-call work on the diagonals at all.  The words are those of gpq_he_gemv.  Why: for q_l = 2^logql the reference's inner sum
 * (src/he-algo.c:65-79: he_mulpt -> poly_rns2mpi(., q) -> he_add -> mpi_smod) is the centred residue mod q_l of S = sum_j rot_j(ct) (*)
 * pt_ij whenever each product is exact in the reference's own dimpt-limb basis; S is exact in a basis that holds its bits, and
 * gpq_rns_reconstruct returns the centred residue mod 2^logql of the centred value mod P.
 *   Bound: ciphertext coefficients are centred, |c| <= 2^(logql-1); diagonal coefficients |d| <= 2^diag_bits - 1; a product coefficient
 *   is a sum of n = 2^logn terms and S of at most n1 products: |S| < 2^(logql - 1 + diag_bits + logn + ceil(log2 n1)) =: 2^L.  S is
 *   recovered from its residues when 2 |S| < P, and P > 2^(59 d) for d primes (every prime exceeds 2^59): L + 1 <= 59 d suffices.
 *   gpq_gemv_acc_dim is the smallest such d (host only, no device).
 *   Guard: when ONE product can wrap the reference's basis (logql - 1 + diag_bits + logn + 1 > 59 dimpt) the reference's result is not the
 *   exact product any more and summing first cannot reproduce it: the plan is created with exact = 0 and holds nothing, and
 *   gpq_gemv_inner / gpq_he_gemv_planned refuse it with GPQ_ERR_INVALID (callers use gpq_he_gemv).  The same when
 *   dim = max(dimpt, gpq_gemv_acc_dim(..)) exceeds the context's limbs.
 * gpq_gemv_plan_create: diag = device big slabs [slots][W][n] as gpq_he_gemv takes them (index i n1 + j); measures diag_bits on the device
 * and returns after the plan's slab (slots x dim x n words, gpq_gemv_plan_info's `bytes`) is queued on `stream`: work on another stream
 * orders itself with gpq_stream_wait.  It waits for `stream` once (the measurement).  Diagonals that are identically zero are recorded and
 * never read again: `live` counts the others.  A plan belongs to its context and must be destroyed before it. */
typedef struct gpq_gemv_plan gpq_gemv_plan;
unsigned gpq_gemv_acc_dim(unsigned logql, unsigned diag_bits, unsigned logn, unsigned n1);
int gpq_gemv_plan_create(gpq_ctx *ctx, gpq_gemv_plan **plan, const uint64_t *diag, unsigned slots, unsigned W, unsigned logql,
                         unsigned dimpt, void *stream);
void gpq_gemv_plan_destroy(gpq_gemv_plan *plan);
int gpq_gemv_plan_info(const gpq_gemv_plan *plan, unsigned *dim, size_t *bytes, unsigned *live, int *exact);
/* needed[r] = 1 for every rotation r < slots whose key gpq_he_gemv_planned reads (live baby rotations, giant steps with a live diagonal), else 0 */
int gpq_gemv_plan_rotations(const gpq_gemv_plan *plan, unsigned char *needed);
/* One giant step's inner sum: out = smod(sum_j R_j (*) diag[giant n1 + j], 2^logql) for `batch` ciphertexts; R0 / R1 = n1 x batch big slabs,
 * rotation-major as gpq_he_rot_hoisted writes them (rotations whose diagonal is zero are not read); a giant step without a live diagonal
 * gives zeros.  Outputs may not overlap the inputs. */
size_t gpq_gemv_inner_workspace_bytes(gpq_ctx *ctx, const gpq_gemv_plan *plan, unsigned batch);
int gpq_gemv_inner(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *R0, const uint64_t *R1, const gpq_gemv_plan *plan,
                   unsigned giant, unsigned W, unsigned batch, void *workspace, void *stream);
/* gpq_he_gemv with the plan in place of `diag`, `slots`, `logql` and `dimpt`: the same words.  Baby rotations none of whose diagonals is
 * live and giant steps without a live diagonal are skipped (both contribute exact zeros), so rk0[r] / rk1[r] may be NULL exactly for the
 * rotations the plan does not need; the rotation by 0 is a key switch with rk[0] like any other.  Launch groups of gpq_set_chunk;
 * outputs may not overlap the inputs or each other (GPQ_ERR_INVALID before anything is launched, as for a NULL key of a live rotation, a
 * plan of another context, or W words that cannot hold q_l). */
size_t gpq_he_gemv_planned_workspace_bytes(gpq_ctx *ctx, const gpq_gemv_plan *plan, unsigned W, unsigned dimB, unsigned dimP, unsigned batch);
int gpq_he_gemv_planned(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const gpq_gemv_plan *plan,
                        const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logDelta, unsigned dimB, unsigned dimP,
                        unsigned batch, void *workspace, void *stream);

/* ---- he_gemv for several matrices: a SET of plans applied to the same ciphertexts ("he_gemv for several matrices") ----------
 * A tall matrix of k slots rows, the four products of he_coeff2slot, several heads on one input: k plans, one ciphertext.  What k calls of
 * gpq_he_gemv_planned repeat depends on the ciphertext alone -- the hoisted baby rotations, their rns_decompose + forward transform, and
 * the reads of those transforms inside every giant step -- and gpq_he_gemv_multi does it once: ONE gpq_he_rot_hoisted over the union of the
 * plans' live baby rotations, one decomposition + transform over the largest `dim`, and per giant step one gemv_mac_multi launch per group
 * of gpq_gemv_multi_width() plans that loads every rotation word once for the group.  Behind the inner sums every plan runs what
 * gpq_he_gemv_planned runs (inverse transform, two reconstructions over its own dim, the rotation by i n1, the wrapping sum, he_rs); the
 * giant rotations of different plans are NOT stacked into one key switch.  out_c0[t] / out_c1[t] are word for word what
 * gpq_he_gemv_planned writes for plans[t]: the sums leave the kernel as canonical residues of the same terms.
 * gpq_gemv_multi_create: `count` plans (1..16; the same plan may appear twice) of this context, all exact, with the same slots and logql
 *   (their `dim` may differ); GPQ_ERR_INVALID otherwise, or when `stream` is capturing, before anything is allocated.  The set BORROWS the
 *   plans: they outlive it.  It holds only small index tables on the device (`bytes`), built once so that the call uploads nothing: the
 *   diagonals stay in the plans.  `baby` = the size of the union of live baby rotations, `dim` = the largest dim among the plans.
 * gpq_gemv_multi_rotations: needed[r] = 1 for every rotation r < slots that some plan of the set needs (the union of
 *   gpq_gemv_plan_rotations); rk0[r] / rk1[r] may be NULL for the others.
 * gpq_he_gemv_multi: out_c0 / out_c1 = host arrays of `count` device slabs of batch x W x n words.  Launch groups of gpq_set_chunk (the
 *   words do not depend on the grouping).  A plan without a live diagonal writes exact zeros.  GPQ_ERR_INVALID before anything is launched
 *   for a null argument or output, a set of another context, W words that cannot hold q_l, logDelta >= logql, an output that overlaps an
 *   input or another output, or a NULL key of the union.  Allocates no device memory and does not synchronise. */
typedef struct gpq_gemv_multi gpq_gemv_multi;
unsigned gpq_gemv_multi_width(void);
int gpq_gemv_multi_create(gpq_ctx *ctx, gpq_gemv_multi **set, const gpq_gemv_plan *const *plans, unsigned count, void *stream);
void gpq_gemv_multi_destroy(gpq_gemv_multi *set);
int gpq_gemv_multi_info(const gpq_gemv_multi *set, unsigned *count, unsigned *baby, unsigned *dim, size_t *bytes);
int gpq_gemv_multi_rotations(const gpq_gemv_multi *set, unsigned char *needed);
size_t gpq_he_gemv_multi_workspace_bytes(gpq_ctx *ctx, const gpq_gemv_multi *set, unsigned W, unsigned dimB, unsigned dimP, unsigned batch);
int gpq_he_gemv_multi(gpq_ctx *ctx, uint64_t *const *out_c0, uint64_t *const *out_c1, const uint64_t *c0, const uint64_t *c1,
                      const gpq_gemv_multi *set, const uint64_t *const *rk0, const uint64_t *const *rk1, unsigned W, unsigned logDelta,
                      unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);

/* ---- he_ecd on the device ("Encoding on the device") ----------------------------------------------------------------------
 * he_ecd, src/he-encode.c:53-64 and :107-111 with invcanemb, src/canemb.c:62-81: `slots` complex doubles -> the plaintext polynomial as a
 * big slab, one workgroup per vector (he_ecd_lds).  The butterflies are the reference's, every double operation rounded on its own (no
 * fused multiply-add), so the words are those of the reference compiled for x86-64 -- GIVEN THE SAME ROOT TABLE: the kernel holds no
 * trigonometry of its own.  All the encoder reads of polyctx.ring.zetas for `slots` slots are the 4 slots + 1 entries
 * T[t] = zetas[t m / (4 slots)] = (cos, sin)(2 PI t / (4 slots)); a table for S slots serves every power of two below S by stride.
 *   Range: Delta = 2^logDelta, logDelta <= 63 (any other Delta needs the x87 product of src/he-encode.c:61 and has no entry point here).
 *   A rounded coefficient must satisfy |v| < 2^63; one that does not, or that is not finite, is stored as 0 and counted in *bad_dev
 *   (a device word the caller zeroes; NULL: not counted).  The other coefficients and vectors of the call are unaffected.
 * gpq_ecd_roots: host only, no device.  table = 2 (4 slots + 1) doubles, (re, im) pairs, from the C library's sincos on
 *   2 PI t / (4 slots) with the reference's PI (src/params.h:52) -- what gcc -O2 makes of src/precomp.c:306-309 -- and T[4 slots] = T[0].
 * gpq_ecd_plan_create: slots = a power of two, <= n/2 and <= 8192 (16 bytes per slot in LDS; more: GPQ_ERR_INVALID).  roots = the caller's
 *   table for roots_slots >= slots (a power of two), read by stride -- a host that has polyctx.ring.zetas passes it with roots_slots = m/4
 *   and gets the words of its own encoder under any libm; NULL = gpq_ecd_roots.  A plan belongs to its context and is destroyed before it.
 * gpq_ecd_plan_create_split: the same plan for slots = a power of two, <= n/2 and <= 65536 (more, or no power of two: GPQ_ERR_INVALID,
 *   nothing allocated), with block_slots as gpq_ecd_plan_set_block takes it.  A vector of more slots than the block B is shared:
 *   slots = 2^k B, k <= 3: the k highest stages run one column per lane on global memory, the rest one block of B slots per workgroup,
 *   and the slab is written by the whole device (he_ecd_cols, he_ecd_block, he_ecd_slab; the decoder mirrors it with he_dcd_block,
 *   he_dcd_cols).  The same individually rounded operations in another order of execution: the words do not depend on the split.
 *   gpq_ecd_plan_create keeps its limit of one workgroup, so a caller that relies on its refusal above 8192 slots still gets it.
 * gpq_he_ecd: z_dev = [count][slots] (re, im) pairs on the device; out = [count][W][n], W <= 32: slot i as W sign-extended words at
 *   coefficient i gap (real part) and i gap + n/2 (imaginary part), gap = n / (2 slots), zero everywhere else.  The call writes every word
 *   of `out`: the caller does not clear it.  Asynchronous on `stream`.  A plan of more than one block takes 32 slots bytes per vector of
 *   hand-off memory from the context, allocated at the first call of a larger batch -- that call runs outside a stream capture, later
 *   ones may be captured -- and wants `out` 16-byte aligned.
 * gpq_ecd_plan_set_block: slots per workgroup for both directions of this plan, a tuning and test knob like gpq_set_chunk: the words
 *   never depend on it.  0 = the default, min(slots, 8192); else a power of two with 2 <= block_slots <= min(slots, 8192) and
 *   slots / block_slots <= 8 (anything else: GPQ_ERR_INVALID, the plan unchanged).  block_slots < slots selects the kernels for more than
 *   one block.  Not while a call on the plan is being issued by another thread.
 * gpq_he_ecd_diagonals: A_dev = a slots x slots row-major matrix of (re, im) pairs; out[i n1 + j] = he_ecd(zrotdiag(A, i n1 + j, -i n1))
 *   (src/he-algo.c:29-43, :63-72; n1 as :51-54): the `diag` of gpq_he_gemv and gpq_gemv_plan_create, gathered by the kernel's load.
 *   A plan above 8192 slots is refused here and by gpq_gemv_plan_create_from_matrix (GPQ_ERR_INVALID): its slots x slots matrix alone
 *   is 4 GiB or more.
 * gpq_gemv_plan_create_from_matrix: gpq_gemv_plan_create on the diagonals of A_dev encoded into a W = 1 slab (8 n bytes per diagonal: every
 *   encodable value fits), which is released before the call returns.  A coefficient out of range fails the call with GPQ_ERR_INVALID
 *   and leaves no plan.  Waits for `stream` as gpq_gemv_plan_create does (the bad count arrives with its measurement), and for the
 *   device when it releases the slab. */
typedef struct gpq_ecd_plan gpq_ecd_plan;
#define GPQ_ECD_MAX_BLOCK_SLOTS 8192u /* slots one workgroup holds: gpq_ecd_plan_create's limit, and a block's */
#define GPQ_ECD_MAX_SLOTS 65536u      /* 8 blocks: gpq_ecd_plan_create_split's limit                           */
int gpq_ecd_roots(double *table, unsigned slots);
int gpq_ecd_plan_create(gpq_ctx *ctx, gpq_ecd_plan **plan, unsigned slots, const double *roots, unsigned roots_slots);
int gpq_ecd_plan_create_split(gpq_ctx *ctx, gpq_ecd_plan **plan, unsigned slots, unsigned block_slots, const double *roots, unsigned roots_slots);
void gpq_ecd_plan_destroy(gpq_ecd_plan *plan);
int gpq_ecd_plan_set_block(gpq_ecd_plan *plan, unsigned block_slots);
int gpq_he_ecd(gpq_ctx *ctx, const gpq_ecd_plan *plan, uint64_t *out, const double *z_dev, unsigned logDelta, unsigned W, unsigned count,
               uint32_t *bad_dev, void *stream);
int gpq_he_ecd_diagonals(gpq_ctx *ctx, const gpq_ecd_plan *plan, uint64_t *out, const double *A_dev, unsigned logDelta, unsigned W,
                         uint32_t *bad_dev, void *stream);
int gpq_gemv_plan_create_from_matrix(gpq_ctx *ctx, gpq_gemv_plan **plan, const gpq_ecd_plan *ecd, const double *A_dev, unsigned logDelta,
                                     unsigned logql, unsigned dimpt, void *stream);
/* the largest coefficient of the plan's diagonals in bits, as gpq_gemv_plan_create measured it (the `diag_bits` of the bound above) */
unsigned gpq_gemv_plan_diag_bits(const gpq_gemv_plan *plan);

/* ---- he_dec and he_dcd on the device ("Decoding on the device") ------------------------------------------------------------
 * he_dcd, src/he-encode.c:66-74 and :114-117 with canemb, src/canemb.c:43-60: a plaintext big slab -> `slots` complex doubles, one
 * workgroup per plaintext (he_dcd_lds) or, for a plan of more than one block (gpq_ecd_plan_create_split above 8192 slots, or gpq_ecd_plan_set_block), one workgroup
 * per block and then one lane per column in place on z_dev (he_dcd_block, he_dcd_cols; no scratch; z_dev 16-byte aligned), on the SAME
 * gpq_ecd_plan as the encoder (its root table and powers of 5; no plan type of its own).
 * The doubles are the reference's bit for bit, given the same root table:
 *   - mpi_to_double (src/types.c:77-106) is `num = num * 2 + bit` in double arithmetic, neither correctly rounded nor truncating: a
 *     magnitude of more than 53 bits becomes M' 2^(L - 53) with M its top 53 bits, b the 54th and M' = M + (b & M & 1); every lower bit is
 *     ignored; +-inf from 2^1024 (a 32-word slab can reach it).  The kernel computes exactly that, sign last;
 *   - the division by nu is the IEEE-rounded one, real and imaginary part on their own: nu is ANY finite double > 0 (after he_mul / he_rs
 *     it is no power of two);
 *   - the butterflies are the reference's, every double operation rounded on its own (no fused multiply-add).
 * gpq_he_dcd: in = [count][W][n] big slabs (two's complement, -2^(64 W - 1) included), W in 1..32; only the 2 slots W words of the
 *   coefficients i gap and i gap + n/2 (gap = n / (2 slots)) of each are read.  z_dev = [count][slots] (re, im) pairs on the device, written
 *   completely: 16 slots bytes per plaintext are what a host downloads.  Asynchronous on `stream`.  GPQ_ERR_INVALID before anything is
 *   launched for a null argument, a plan of another context, W outside 1..32, count = 0, nu not finite or <= 0, or the wrong current device.
 * gpq_he_dec: he_dec, src/he-encrypt.c:105-125, for q_l = 2^logql on big slabs of W words (64 W > logql):
 *   m = smod(poly_mul(c1, sk, dim, q_l) + c0, q_l) for `batch` ciphertexts; sk_ntt = the secret key as ONE NTT-domain slab uint64_t[dim][n]
 *   (gpq_evk_pack of its big slab, batch 1), shared by the batch: the key is never replicated.  dim = (logql + 1) / 59 + 1 is the caller's
 *   (:113).  The words are the reference's also when c1 * sk wraps the dim-limb basis.  Outputs may not alias inputs. */
int gpq_he_dcd(gpq_ctx *ctx, const gpq_ecd_plan *plan, double *z_dev, const uint64_t *in, double nu, unsigned W, unsigned count, void *stream);
size_t gpq_he_dec_workspace_bytes(const gpq_ctx *ctx, unsigned dim, unsigned batch);
int gpq_he_dec(gpq_ctx *ctx, uint64_t *m, const uint64_t *c0, const uint64_t *c1, const uint64_t *sk_ntt, unsigned W, unsigned logql,
               unsigned dim, unsigned batch, void *workspace, void *stream);

/* ---- samplers and encryption on the device ("Encrypting on the device") ------------------------------------------------------
 * The randomness is the caller's, as for he_gen*k: the library never invents entropy, it turns the caller's BYTES (device memory, at any
 * byte address: a caller slices one stream) into the polynomials the reference's samplers make of the same bytes.  A "small slab" is
 * int8_t[count][n], one signed byte per coefficient.  All calls are asynchronous on `stream`; outputs may not overlap inputs or each other.
 * gpq_sample_error_table: host only, no device.  table = 65536 x 2 entries, T[b0][b1] = ((int16_t)floor(rr cos(theta) + 0.5), (int16_t)floor(rr
 *   sin(theta) + 0.5)) with theta = 2 PI b0 / 256, rr = sqrt(-2 log(b1 / 256)) SIGMA (src/sample.c:64-71, src/params.h:52, :55).  Every entry lies
 *   in [-11, 11]; the argument of floor stays 5e-5 away from the integers, so the table does not depend on the libm.  For b1 = 0 (log 0 = -inf:
 *   the conversion is undefined in C) it holds (0, 0), what the reference executed on x86-64 gives.  The context builds and uploads it (128 KiB,
 *   counted in gpq_debug_table_bytes) at the first gpq_sample_error, which therefore runs once outside a stream capture -- by the one
 *   host thread that drives the context, like every other table built at first use (see "slab operations" above: a context is not thread-safe).
 * gpq_sample_zo: sample_zo, src/sample.c:112-131.  bytes_dev = [count][n/4]; with Z the little-endian integer of a polynomial's bytes,
 *   coefficient i = 0 when bit 2i of Z is 0, else +1 when bit 2i + 1 is 0, else -1.  logn >= 2.
 * gpq_sample_error: sample_error, :60-82.  bytes_dev = [count][n]; (coefficient i, i + 1) = T[byte i][byte i + 1] for even i.
 * gpq_sample_uniform: sample_uniform, :133-141 with loadmpi_littleendian (src/types.c:166-184).  nbits = the bit length of q (logq + 1 for
 *   q = 2^logq); bytes_dev = [count][n][nbits / 8 + 1]; a coefficient = the low nbits bits of its bytes' little-endian integer (the rest of the
 *   last byte -- all of it when nbits % 8 == 0 -- is consumed and dropped), in [0, 2^nbits): NOT reduced and NOT centred.  big = a big slab
 *   [count][W][n] of non-negative values, 64 W > nbits, W <= 32; every word of it is written.
 * gpq_small_to_big: a small slab sign-extended into a big slab of W words, the format gpq_he_genswk's `e` and every other entry point takes.
 * gpq_he_enc_pk: he_enc_pk, src/he-encrypt.c:37-73, for q = 2^logq on `batch` plaintexts:
 *     c0 = smod(poly_mul(pk.p0, v, dim, q) + m + e0, q),  c1 = smod(poly_mul(pk.p1, v, dim, q) + e1, q)
 *   m = plaintext big slabs [batch][W][n] (NULL: none); v, e0, e1 = small slabs [batch][n] (sample_zo, sample_error, sample_error, in the
 *   reference's order); pk0_ntt / pk1_ntt = the public key as ONE NTT-domain slab pair uint64_t[dim][n] (gpq_evk_pack of the centred key
 *   polynomials, batch 1), shared by the batch.  dim is the caller's (hectx.dim, src/precomp.c:401).  v goes straight to residues and is
 *   transformed once for both products (gpq_keyswitch with the key pair, its launch groups and lanes included).
 * gpq_he_enc_sk: he_enc_sk, :75-103:  c0 = smod(-poly_mul(a, sk, dim, q) + m + e, q),  c1 = smod(a, q)
 *   a = the RAW sample of gpq_sample_uniform (nbits = logq + 1), big slabs [batch][W][n] with 64 W > logq + 1: the reference multiplies the
 *   uncentred sample (:91) and centres it afterwards (:97), and so does this call; e = small slabs; sk_ntt = the secret key as gpq_he_dec
 *   takes it.  The words are the reference's also when a * sk wraps the dim-limb basis.  m == NULL is no plaintext: exactly he_keypair's
 *   pk.p0, pk.p1 (src/he-kem.c:59-65) from its sample_error and sample_uniform(q_L) -- he_keypair has no entry point of its own.
 * Sampler order and bytes: he_enc_pk zo, error, error (n/4 + 2n); he_enc_sk error, uniform (n + n (nbits / 8 + 1)); he_keypair sample_sk
 * (sequential rejection sampling: the host's), error, uniform.  The l / nu / B bookkeeping (:40-42) stays with the caller.
 * GPQ_ERR_INVALID before anything is launched for: a null argument (except m); W outside 1..32, 64 W <= logq (gpq_he_enc_sk: <= logq + 1)
 * or <= nbits; logq or nbits = 0; count or batch = 0; batch (and gpq_small_to_big's count) above 65535, a sampler's count beyond one
 * launch (2^31 - 1 workgroups); logn < 2 for gpq_sample_zo, < 1 for gpq_sample_error; a dim the context lacks; an overlap of an output with an input,
 * the other output or the workspace; the wrong current device.  workspace: gpq_he_enc_workspace_bytes(ctx, dim, batch, pk = 1 for gpq_he_enc_pk, 0 for gpq_he_enc_sk). */
int gpq_sample_error_table(int8_t *table);
int gpq_sample_zo(gpq_ctx *ctx, int8_t *out, const uint8_t *bytes_dev, unsigned count, void *stream);
int gpq_sample_error(gpq_ctx *ctx, int8_t *out, const uint8_t *bytes_dev, unsigned count, void *stream);
int gpq_sample_uniform(gpq_ctx *ctx, uint64_t *big, const uint8_t *bytes_dev, unsigned nbits, unsigned W, unsigned count, void *stream);
int gpq_small_to_big(gpq_ctx *ctx, uint64_t *big, const int8_t *small, unsigned W, unsigned count, void *stream);
size_t gpq_he_enc_workspace_bytes(const gpq_ctx *ctx, unsigned dim, unsigned batch, int pk);
int gpq_he_enc_pk(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *m, const int8_t *v, const int8_t *e0, const int8_t *e1,
                  const uint64_t *pk0_ntt, const uint64_t *pk1_ntt, unsigned W, unsigned logq, unsigned dim, unsigned batch, void *workspace,
                  void *stream);
int gpq_he_enc_sk(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *m, const uint64_t *a, const int8_t *e,
                  const uint64_t *sk_ntt, unsigned W, unsigned logq, unsigned dim, unsigned batch, void *workspace, void *stream);

/* ---- random bytes on the device ("Random bytes on the device") ---------------------------------------------------------------
 * The samplers above take the caller's bytes; these calls make the bytes the reference's default build would have drawn -- its deterministic
 * randombytes, src/rng.c:36-77 (SUPERCOP's surf generator, -DSUPERCOP) -- where the samplers read them.  The library still invents no entropy:
 * a stream is a function of the caller's 32-word seed and nothing else; seed == NULL is the reference's own seed (src/rng.c:36-38), public test
 * data.  The generator runs in counter mode (a 128-bit block counter, incremented before each block of 8 bytes), so a stream is addressed by a
 * 128-bit BYTE position (pos_lo, pos_hi): byte k is the low byte of out[7 - k % 8] of the block with counter k / 8 + 1, and the first call of
 * the reference's randombytes(x, len) in a process returns the bytes [0, len).  A 128-bit byte position cannot overflow the block counter.
 * The other randombytes variants of src/rng.c (RANDOM, GCRY_RANDOM, AES256) are non-deterministic or sequential and have no counterpart here.
 * gpq_surf_bytes: bytes [pos, pos + len) of the stream into bytes_dev[0..len), device memory at any byte address; no byte outside it is
 *   written.  Where (address - pos) % 8 == 0 every aligned 16 bytes leave as one store (a 16-byte aligned buffer filled from a position
 *   that is a multiple of 8: the fast case); any other combination gives the same bytes more slowly.  Asynchronous on `stream`, no
 *   allocation, no synchronisation: capturable -- and seed and position are launch arguments, so a REPLAYED graph repeats its bytes.
 *   More than 2^30 bytes run as several launches.
 * gpq_surf_bytes_host: the same bytes into host memory on one CPU thread (the rate of the reference's randombytes); no device needed.
 * gpq_rng: a stream with a position.  gpq_rng_host_bytes / gpq_rng_device_bytes hand out the next len bytes and advance the position
 *   (the device call when its launches are queued: what it reserved is spent even if a captured graph is never replayed); calls of both
 *   kinds on one object, in any mix, give one contiguous slice.  An object serialises its callers (a mutex); the device work is ordered by
 *   `stream` as usual.  gpq_rng_seek / gpq_rng_tell set and read the position (pos[0] low, pos[1] high).
 * GPQ_ERR_INVALID before anything is launched or written for: a null pointer (except seed), len = 0, pos + len beyond 2^128, and for the
 * device calls the wrong current device.
 * gpq_debug_rng_split: tests: the bytes of one launch (a multiple of 16; 0 = the default 2^30).  Process-wide. */
typedef struct gpq_rng gpq_rng;
int gpq_surf_bytes(gpq_ctx *ctx, uint8_t *bytes_dev, size_t len, const uint32_t seed[32], uint64_t pos_lo, uint64_t pos_hi, void *stream);
int gpq_surf_bytes_host(uint8_t *x, size_t len, const uint32_t seed[32], uint64_t pos_lo, uint64_t pos_hi);
int gpq_rng_create(gpq_rng **rng, const uint32_t seed[32]);
void gpq_rng_destroy(gpq_rng *rng);
int gpq_rng_seek(gpq_rng *rng, uint64_t pos_lo, uint64_t pos_hi);
int gpq_rng_tell(const gpq_rng *rng, uint64_t pos[2]);
int gpq_rng_host_bytes(gpq_rng *rng, uint8_t *x, size_t len);
int gpq_rng_device_bytes(gpq_ctx *ctx, gpq_rng *rng, uint8_t *bytes_dev, size_t len, void *stream);
int gpq_debug_rng_split(size_t bytes);

/* ---- general moduli: any q_l (little-endian words ql_words[0..Lq)) and any Delta (uint64_t, as hectx_init takes it,
 * src/gpqhe.h:100).  Same reference semantics, through the multiword Barrett kernel: slow-path quality, meant for parameter
 * sets outside the powers of two that the fast entry points above cover. */
size_t gpq_he_general_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch);
int gpq_he_rs_general(gpq_ctx *ctx, uint64_t *c0, uint64_t *c1, unsigned W, unsigned long long delta, const uint64_t *ql_words,
                      unsigned Lq, unsigned batch, void *scratch /* 192 words */, void *stream);
int gpq_relin_tail_general(gpq_ctx *ctx, uint64_t *out, const uint64_t *chat, const uint64_t *d, unsigned W, const uint64_t *ql_words,
                           unsigned Lq, unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);
int gpq_he_mul_general(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *ct1c0, const uint64_t *ct1c1,
                       const uint64_t *ct2c0, const uint64_t *ct2c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W,
                       const uint64_t *ql_words, unsigned Lq, unsigned dimA, unsigned dimB, unsigned dimP, unsigned batch,
                       void *workspace, void *stream);
/* workspace: gpq_he_mulpt_workspace_bytes + gpq_poly_mul_general_workspace_bytes */
int gpq_he_mulpt_general(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m,
                         unsigned W, const uint64_t *ql_words, unsigned Lq, unsigned dim, unsigned batch, void *workspace, void *stream);
int gpq_he_swk_general(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *d0, const uint64_t *d1,
                       const uint64_t *swk0, const uint64_t *swk1, unsigned W, const uint64_t *ql_words, unsigned Lq,
                       unsigned dimB, unsigned dimP, unsigned batch, void *workspace, void *stream);

/* he_add / he_sub / he_neg on one big-slab polynomial (src/he-add.c:32-142: mpi_addm / mpi_subm + mpi_smod), q_l = 2^logql.
 * Not NTT work; offered so that ciphertexts can stay in HBM between multiplications.  r may alias a or b. */
int gpq_big_add(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned logql, unsigned batch, void *stream);
int gpq_big_sub(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, const uint64_t *b, unsigned W, unsigned logql, unsigned batch, void *stream);
int gpq_big_neg(gpq_ctx *ctx, uint64_t *r, const uint64_t *a, unsigned W, unsigned logql, unsigned batch, void *stream);
/* The storage step of he_genswk (src/he-kem.c:103-110): a centred key polynomial (big slab) -> NTT-domain slab of dimevk limbs. */
int gpq_evk_pack(gpq_ctx *ctx, uint64_t *evk, const uint64_t *big, unsigned W, unsigned dimevk, unsigned batch, void *stream);
/* he_genswk, src/he-kem.c:74-118, from the polynomials the reference samples on the host: p1 (uniform mod P*q_L), e (error) and the
 * polynomial the key hides (sp = s^2 for he_genrlk, the rotated / conjugated secret for he_genrk / he_genck), all big slabs of W words
 * (64 W > bits of P*q_L), q_L = 2^logqL:  swk.p0 = smod(-p1*sk + e + P*sp, P*q_L), swk.p1 = smod(p1, P*q_L), each stored as
 * rns_decompose + ntt over dimevk limbs (evk0, evk1: uint64_t[dimevk][n]). */
size_t gpq_he_genswk_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimP, unsigned logqL);
int gpq_he_genswk(gpq_ctx *ctx, uint64_t *evk0, uint64_t *evk1, const uint64_t *p1, const uint64_t *sk, const uint64_t *e,
                  const uint64_t *sp, unsigned W, unsigned dimP, unsigned logqL, unsigned dimevk, void *workspace, void *stream);
/* `count` switching keys in one call ("Key generation on the device"): for key j the words of he_genswk (src/he-kem.c:74-118)
 * and of gpq_he_genswk above,  swk.p0 = smod(-poly_mul(p1_j, sk, dimmul, P q_L) + e_j + P sp_j, P q_L),  swk.p1 = smod(p1_j, P q_L),
 * each stored as rns_decompose + ntt over dimevk limbs: evk0, evk1 = uint64_t[count][dimevk][n].
 *   p1     = [count][W][n]: the RAW gpq_sample_uniform output with nbits = the bit length of P q_L (not reduced, not centred: the
 *            reference multiplies the raw sample, :95, and centres it afterwards, :101); 64 W > nbits
 *   e      = small slabs [count][n] (gpq_sample_error)
 *   sk_ntt = the secret as ONE NTT-domain slab uint64_t[dimmul][n] (gpq_evk_pack of its big slab over dimmul =
 *            gpq_he_genswk_dimmul(ctx, dimP, logqL) limbs, :83), shared by all keys, as gpq_he_dec takes it.  The words are the
 *            reference's also when p1 * sk wraps the dimmul-limb basis.
 *   galois = HOST array [count] of odd g, or NULL.  Given: sp_j is the image of the secret under X -> X^g, g as gpq_automorphism_index
 *            takes it (5^rot mod 2^64: poly_rot, src/poly.c:263-275; 2n - 1: poly_conj), gathered by the kernel from sk_small =
 *            int8_t[n], the secret itself: coefficient t is sk[i'] for i' = t g^-1 mod 2n < n and -sk[i' - n] otherwise; a rotated
 *            secret never exists in memory.  The values are read before the call returns.
 *            NULL: sp = the hidden polynomials as big slabs [count][Wsp][n] (he_genrlk: s^2 centred mod q_L); sk_small is not read.
 * Asynchronous on `stream`, no host synchronisation; the constants of (dimP, logqL) are built at the first call of that pair (which
 * therefore runs once outside a stream capture) and stay with the context.  Keys run in launch groups of gpq_set_chunk; the words do
 * not depend on the grouping.  workspace: gpq_he_genswk_batch_workspace_bytes (0 on error).
 * GPQ_ERR_INVALID before anything is launched for: a null argument (outside the either/or of galois + sk_small / sp + Wsp), an even
 * g, logqL = 0, count = 0, 64 W <= bits of P q_L, a dimP, dimevk or dimmul the context lacks, an output that overlaps an input, the
 * other output or the workspace, the wrong current device.  GPQ_ERR_UNSUPPORTED where gpq_he_genswk returns it (W > 32, P above 32 words). */
size_t gpq_he_genswk_batch_workspace_bytes(gpq_ctx *ctx, unsigned W, unsigned dimP, unsigned logqL, unsigned dimevk, unsigned count);
int gpq_he_genswk_batch(gpq_ctx *ctx, uint64_t *evk0, uint64_t *evk1, const uint64_t *p1, const int8_t *e, const uint64_t *sk_ntt,
                        const int8_t *sk_small, const uint64_t *galois, const uint64_t *sp, unsigned Wsp, unsigned W, unsigned dimP,
                        unsigned logqL, unsigned dimevk, unsigned count, void *workspace, void *stream);
unsigned gpq_he_genswk_dimmul(gpq_ctx *ctx, unsigned dimP, unsigned logqL);   /* src/he-kem.c:83; 0 on error */

/* ---- per-kernel profile ----------------------------------------------------
 * When enabled every kernel launch of this context is bracketed by two HIP
 * events on its own stream.  gpq_profile_collect waits for them and adds the
 * durations per kernel (index < gpq_profile_kernels()) into the two arrays. */
int gpq_profile_enable(gpq_ctx *ctx, int on);
int gpq_profile_kernels(void);
const char *gpq_profile_kernel_name(int kernel);
int gpq_profile_collect(gpq_ctx *ctx, double *total_ms, unsigned long long *launches);

/* ---- timing on the stream the kernels run on (HIP events) ----------------- */
typedef struct gpq_timer gpq_timer;
int gpq_timer_create(gpq_timer **t);
int gpq_timer_start(gpq_timer *t, void *stream);
int gpq_timer_stop(gpq_timer *t, void *stream);
int gpq_timer_elapsed_ms(gpq_timer *t, float *ms); /* synchronises on the stop event */
void gpq_timer_destroy(gpq_timer *t);

#ifdef __cplusplus
}
#endif
#endif /* GPQHE_HIP_H */
