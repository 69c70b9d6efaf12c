/* gpqhe_hip_algo.h -- the evaluators of src/he-algo.c:131-548 (he_inv, he_sqrt, he_sigmoid, he_log, he_exp, he_cmp, he_cmppt) as single device
 * calls on big slabs, and the one kernel they add to the library, gpq_he_lin_const (with a dense plaintext term: gpq_he_lin_pt).  Companion of gpqhe_hip.h (contexts, slab layout, error codes, every call the
 * evaluators are made of); DESIGN.md section 6, "Evaluators".
 *
 * Stream class (gpqhe_hip.h, "stream classes"): every function below that takes a `void *stream` is CAPTURABLE -- all its device work is queued
 * on `stream`, nothing on the null stream, and after one warm call of the same shape on the same context it makes no host synchronisation, no
 * allocation and no host read-back, so it may be captured into a graph and replayed.  Host arguments (constants, iteration counts) are read
 * before the call returns and are part of the captured launches. */
#ifndef GPQHE_HIP_ALGO_H
#define GPQHE_HIP_ALGO_H

#include "gpqhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The additive glue of the evaluators in one launch.  he_neg, he_add, he_sub, he_addpt, he_subpt (src/he-add.c:32-140), he_moddown
 * (src/he-rescale.c:56-70) and he_copy_ct are each "add, then mpi_smod(., q_l)" (src/types.c:108-113); every q_l is a power of two, so a chain of
 * them is the wrapping sum of its terms followed by the last mpi_smod.  With x^h = x^(n/2):
 *   out.c0 = smod(s_0 x_0.c0 + .. + s_(K-1) x_(K-1).c0 + (a + b x^h), 2^logql)
 *   out.c1 = smod(s_0 x_0.c1 + .. + s_(K-1) x_(K-1).c1,               2^logql)
 * K = 1..3 terms, sign[k] = +1 or -1, a and b = he_const_pt's two integers (gpq_const_pt; 0 for none).  The terms are any W-word two's-complement
 * big slabs of `batch` ciphertexts -- typically centred for a larger modulus, which is he_moddown -- and the output is in mpi_smod's range,
 * sign-extended to W words: the words gpq_he_rs(.., logDelta = 0, logql) writes.  1 <= logql <= 64 W.  out_c0 / out_c1 may be x_c0[k] / x_c1[k]
 * of any one term (the same position); no other overlap.  No workspace.  CAPTURABLE. */
int gpq_he_lin_const(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *const x_c0[3], const uint64_t *const x_c1[3],
                     const int sign[3], unsigned K, int64_t a, int64_t b, unsigned W, unsigned logql, unsigned batch, void *stream);

/* The evaluators.  `kind` for the two host functions: */
enum { GPQ_ALGO_INV = 0, GPQ_ALGO_SQRT = 1, GPQ_ALGO_SIGMOID = 2, GPQ_ALGO_LOG = 3, GPQ_ALGO_EXP = 4 };

/* Levels the evaluator consumes: he_inv iter + 1, he_sqrt 2 iter, he_sigmoid 4, he_log 4, he_exp 4 + iter (`iter` is ignored by the two without
 * one); -1 for an unknown kind.  Host only. */
int gpq_he_algo_depth(int kind, unsigned iter);

/* Bytes of the one workspace an evaluator call takes its temporaries from: the named temporaries of the reference's function as big slabs of
 * `batch` ciphertexts, plus the maximum over the levels it multiplies at of gpq_he_mul_workspace_bytes (and, for he_exp, of
 * gpq_he_mulpt_workspace_bytes and one copy of the plaintext per ciphertext).  0 when the call would be refused (gpq_last_error says why). */
size_t gpq_he_algo_workspace_bytes(gpq_ctx *ctx, int kind, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                                   unsigned batch);

/* he_inv (src/he-algo.c:131-164), he_sqrt (:166-206), he_sigmoid (:208-277), he_log (:279-361), he_exp (:364-458) of `batch` ciphertexts with
 * q_L = 2^logqL, q_l = 2^logql the INPUT's modulus and Delta = 2^logDelta: the reference's sequence, call for call, where
 *   he_mul + he_rs                    is gpq_he_mul_rs (a squaring passes the same slabs twice),
 *   he_const_pt + he_mulpt + he_rs    is gpq_he_mulpt_const, the constant being the reference's C double expression through gpq_const_pt,
 *   he_ecd + he_mulpt + he_rs         (he_exp's one dense plaintext) is gpq_he_mulpt + gpq_he_rs,
 *   everything additive               is gpq_he_lin_const.
 * The output is centred mod 2^(logql - depth logDelta), depth = gpq_he_algo_depth.  rlk0 / rlk1: the relinearisation key's NTT-domain slabs of at
 * least dimB(logql) limbs (gpq_he_dims).  Inputs are centred mod 2^logql, as for gpq_he_mulpt_const; they are not written, and out_c0 / out_c1
 * may be c0 / c1.  l / nu / B stay with the caller, as everywhere in the slab API.
 * Refused with GPQ_ERR_INVALID before anything is launched, the outputs untouched: logDelta outside 1..63; a level that would fall below
 * logql = 1; a constant that does not pass gpq_he_mulpt_const_fits at the reference's limb count; a limb count (gpq_he_dims, he_mulpt's) beyond
 * the context's primes; W < ceil(logql / 64).
 * `workspace`: gpq_he_algo_workspace_bytes.  No allocation, no host synchronisation, nothing on the null stream.  CAPTURABLE. */
int gpq_he_inv(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0,
               const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter, unsigned batch,
               void *workspace, void *stream);
int gpq_he_sqrt(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0,
                const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter, unsigned batch,
                void *workspace, void *stream);
int gpq_he_sigmoid(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0,
                   const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned batch, void *workspace,
                   void *stream);
int gpq_he_log(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0,
               const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned batch, void *workspace,
               void *stream);
/* he_exp: m = the big slab (W words, ONE polynomial shared by the batch) of he_ecd applied to the constant vector a / 2^iter (:444-448), encoded
 * by gpq_he_ecd or on the host; dimpt = he_mulpt's limb count for it (src/he-mult.c:168), at most the reference's value for nu = Delta. */
int gpq_he_exp(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m, unsigned dimpt,
               const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
               unsigned batch, void *workspace, void *stream);

/* gpq_he_lin_const plus ONE dense plaintext: he_addpt (msign = +1) / he_subpt (msign = -1) by any plaintext (src/he-add.c:80-123) as one more
 * addend of the same launch.
 *   out.c0 = smod(s_0 x_0.c0 + .. + s_(K-1) x_(K-1).c0 + msign m + (a + b x^h), 2^logql)          out.c1 as gpq_he_lin_const's
 * m: a W-word two's-complement big slab of ONE polynomial, shared by the whole batch (no batch stride), as gpq_he_exp takes its plaintext.
 * Everything else, the refusals included, is gpq_he_lin_const's; also refused: m NULL, msign not +-1, m overlapping an output.  CAPTURABLE. */
int gpq_he_lin_pt(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *const x_c0[3], const uint64_t *const x_c1[3],
                  const int sign[3], unsigned K, const uint64_t *m, int msign, int64_t a, int64_t b, unsigned W, unsigned logql, unsigned batch,
                  void *stream);

/* he_cmp and he_cmppt (src/he-algo.c:460-548) as single calls.
 * The reference derives its round count from alpha: t = (unsigned)log2(alpha / log2(1 + pow(2, -(int)alpha))) (:519-520).  gpq_he_cmp_rounds
 * evaluates that C double expression for 1 <= alpha <= 52 and returns -1 otherwise (alpha = 0 takes log2(0), alpha >= 53 divides by
 * log2(1.0) = 0: the reference converts an infinity to unsigned, which is undefined).  he_cmppt's own expression (:537) negates an UNSIGNED
 * alpha and is undefined for every alpha, so both calls below take t, and a caller of he_cmppt says which t it means.  Host only. */
int gpq_he_cmp_rounds(unsigned alpha);
/* (3 + iter)(1 + t), the levels both consume; -1 where that overflows or exceeds 4096.  Host only. */
int gpq_he_cmp_depth(unsigned iter, unsigned t);
/* Bytes of the workspace of gpq_he_cmp (with_pt = 0) / gpq_he_cmppt (1): four temporaries and a spare as big slabs of `batch` ciphertexts, two
 * slabs of 2 batch ciphertexts (an and bn side by side: the two squarings of a round are ONE gpq_he_mul_rs over 2 batch ciphertexts, out of one
 * into the other), plus the largest gpq_he_mul_workspace_bytes of the levels, at 2 batch where there is a round.  0 when the call would be
 * refused (gpq_last_error says why). */
size_t gpq_he_cmp_workspace_bytes(gpq_ctx *ctx, int with_pt, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                                  unsigned t, unsigned batch);
/* out = he_cmp(a, b) / he_cmppt(ct, m) of `batch` ciphertexts, the contract of the five evaluators above: the reference's sequence call for
 * call with every additive chain in one gpq_he_lin_const / gpq_he_lin_pt, the nested he_inv included (its text, run once more on other
 * temporaries); he_cmp_core's last bn = 1 - an feeds nothing and is not computed.  Inputs centred mod 2^logql and never written; the output is
 * centred mod 2^(logql - gpq_he_cmp_depth(iter, t) logDelta).  out_c0 / out_c1 may be a_c0 / a_c1 (c0 / c1) and overlap nothing else.
 * m: ONE plaintext big slab (W words) shared by the batch, any integers: it enters through one mpi_smod at the input's level.
 * Refusals as above, decided before anything is launched; also batch > 16383 where t > 0.  `workspace`: gpq_he_cmp_workspace_bytes.
 * CAPTURABLE. */
int gpq_he_cmp(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *a_c0, const uint64_t *a_c1, const uint64_t *b_c0,
               const uint64_t *b_c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta,
               unsigned iter, unsigned t, unsigned batch, void *workspace, void *stream);
int gpq_he_cmppt(gpq_ctx *ctx, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m,
                 const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                 unsigned t, unsigned batch, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
