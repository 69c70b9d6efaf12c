// bridge_algo.hpp -- host fragment of bridge.hip: gpq_he_lin_const / gpq_he_lin_pt (algo_kernels.hpp) and the evaluators gpq_he_inv / gpq_he_sqrt /
// gpq_he_sigmoid / gpq_he_log / gpq_he_exp / gpq_he_cmp / gpq_he_cmppt (include/gpqhe_hip_algo.h).  The sequences themselves are algo_seq.hpp's;
// AlgoDevice below is the implementation of their operations that launches -- through the public entry points only (gpq_he_mul_rs,
// gpq_he_mulpt_const, gpq_he_mulpt, gpq_he_rs, gpq_he_lin_const, gpq_he_lin_pt): an evaluator is straight-line host code around calls that exist.
#pragma once
#include "algo_seq.hpp"

namespace {
// gpq_he_lin_const (pt = false: m and msign are not looked at) and gpq_he_lin_pt behind one set of checks and one launch
int he_lin(gpq_ctx *c, const char *who, bool pt, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *const x_c0[3], const uint64_t *const x_c1[3],
           const int sign[3], unsigned K, const uint64_t *m, int msign, int64_t a, int64_t b, unsigned W, unsigned logql, unsigned batch, void *stream) {
  int rc = check(c, 1, batch, who);
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !x_c0 || !x_c1 || !sign || K < 1 || K > 3 || W < 1 || W > 64 || logql < 1 || logql > 64 * W || c->logn < 1 || batch > 32767)
    return gpq_fail(GPQ_ERR_INVALID, "%s: bad arguments (1 <= K <= 3, 1 <= logql <= 64 W)", who);
  if (pt && (!m || (msign != 1 && msign != -1))) return gpq_fail(GPQ_ERR_INVALID, "%s: the plaintext is NULL or msign is not +-1", who);
  LinConstArgs k{out_c0, out_c1, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, a, b, 0u, W, c->logn, logql, pt ? m : nullptr, pt && msign < 0 ? 1u : 0u};
  const size_t words = (size_t)batch * W * c->n;
  if (ranges_overlap(out_c0, words, out_c1, words)) return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs overlap", who);
  if (pt && (ranges_overlap(out_c0, words, m, (size_t)W * c->n) || ranges_overlap(out_c1, words, m, (size_t)W * c->n)))
    return gpq_fail(GPQ_ERR_INVALID, "%s: an output overlaps the plaintext", who);   // every ciphertext of the batch reads all of m
  for (unsigned t = 0; t < K; ++t) {
    if (!x_c0[t] || !x_c1[t] || (sign[t] != 1 && sign[t] != -1)) return gpq_fail(GPQ_ERR_INVALID, "%s: term %u is NULL or its sign is not +-1", who, t);
    // a lane reads and writes its own coefficient only: the output may BE a term's slab of the same polynomial, and may overlap nothing else
    if ((x_c0[t] != out_c0 && ranges_overlap(out_c0, words, x_c0[t], words)) || (x_c1[t] != out_c1 && ranges_overlap(out_c1, words, x_c1[t], words)) ||
        ranges_overlap(out_c0, words, x_c1[t], words) || ranges_overlap(out_c1, words, x_c0[t], words))
      return gpq_fail(GPQ_ERR_INVALID, "%s: an output overlaps term %u other than in the same position", who, t);
    k.x0[t] = x_c0[t]; k.x1[t] = x_c1[t];
    if (sign[t] < 0) k.neg |= 1u << t;
  }
  {
    ProfScope prof(c, GPQ_K_LIN_CONST, (hipStream_t)stream);
    const dim3 grid((c->n + 255) / 256, 2 * batch), block(256);
    if (pt) {
      if (K == 1) hipLaunchKernelGGL((he_lin_const<1, true>), grid, block, 0, (hipStream_t)stream, k);
      else if (K == 2) hipLaunchKernelGGL((he_lin_const<2, true>), grid, block, 0, (hipStream_t)stream, k);
      else hipLaunchKernelGGL((he_lin_const<3, true>), grid, block, 0, (hipStream_t)stream, k);
    } else if (K == 1) hipLaunchKernelGGL(he_lin_const<1>, grid, block, 0, (hipStream_t)stream, k);
    else if (K == 2) hipLaunchKernelGGL(he_lin_const<2>, grid, block, 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(he_lin_const<3>, grid, block, 0, (hipStream_t)stream, k);
  }
  return launched(who);
}
}  // namespace

extern "C" int gpq_he_lin_const(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *const x_c0[3], const uint64_t *const x_c1[3],
                                const int sign[3], unsigned K, int64_t a, int64_t b, unsigned W, unsigned logql, unsigned batch, void *stream) {
  return he_lin(c, "gpq_he_lin_const", false, out_c0, out_c1, x_c0, x_c1, sign, K, nullptr, 1, a, b, W, logql, batch, stream);
}
extern "C" int gpq_he_lin_pt(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *const x_c0[3], const uint64_t *const x_c1[3],
                             const int sign[3], unsigned K, const uint64_t *m, int msign, int64_t a, int64_t b, unsigned W, unsigned logql,
                             unsigned batch, void *stream) {
  return he_lin(c, "gpq_he_lin_pt", true, out_c0, out_c1, x_c0, x_c1, sign, K, m, msign, a, b, W, logql, batch, stream);
}

namespace {

// Workspace of an evaluator call: the named temporaries and one spare (c0 | c1 of `batch` ciphertexts each), he_exp's plaintext once per
// ciphertext (gpq_he_mulpt multiplies slab by slab), then the products' own workspace, the largest of the levels.
// `paired` (he_cmp): two more buffers of DOUBLE width, c0 of 2 batch ciphertexts | c1 of 2 batch ciphertexts, whose halves hold an and bn side
// by side, so that one gpq_he_mul_rs over 2 batch ciphertexts squares both from one into the other.
struct AlgoPlan { size_t ct, pool, half, pair, m, total; unsigned buffers; };
AlgoPlan algo_plan(const gpq_ctx *c, unsigned temporaries, bool mulpt, unsigned W, unsigned batch, size_t ws, bool paired = false) {
  AlgoPlan p;
  p.buffers = temporaries + 1;
  p.ct = align64((size_t)batch * W * c->n * 8);
  p.pool = 2 * p.ct * p.buffers;
  // Not rounded: the two halves are ONE slab of 2 batch ciphertexts.  Half 1 is that slab's ciphertext number `batch`, at the batch stride of
  // W n 8 bytes every slab call gives ciphertext k >= 1 (64-byte aligned from n = 8 on); no call needs more of a ciphertext than of a caller's.
  p.half = (size_t)batch * W * c->n * 8;
  p.pair = paired ? 2 * align64(2 * p.half) : 0;
  p.m = mulpt ? p.ct : 0;
  p.total = p.pool + 2 * p.pair + p.m + align64(ws);
  return p;
}
AlgoPlan algo_plan(const gpq_ctx *c, int kind, unsigned W, unsigned batch, size_t ws) {
  return algo_plan(c, gpq_algo::temporaries(kind), kind == GPQ_ALGO_EXP, W, batch, ws);
}

// The operations of algo_seq.hpp on the device.  A slot's value lives in one of the workspace's buffers, in the caller's input (slot 0 and,
// for he_cmp, slot 1: never written) or -- the result, when the sequence's last operation writes it -- in the caller's output.  A slot is rewritten in place only where the
// entry point allows it and nobody else names the buffer (alias); otherwise the new value takes a free buffer and the old one is released.
struct AlgoDevice : gpq_algo::Book {
  enum { POOL = gpq_algo::SLOTS, IN = POOL, OUT = POOL + 1, IN2 = POOL + 2 };
  uint64_t *b0[POOL], *b1[POOL];
  int ref[POOL], at[gpq_algo::SLOTS];
  unsigned buffers;
  const uint64_t *in0, *in1, *rlk0, *rlk1, *m;     // m: the call's one dense plaintext (he_exp's factor, he_cmppt's addend)
  const uint64_t *in2_0 = nullptr, *in2_1 = nullptr;
  uint64_t *out0, *out1, *mrep;
  void *wsp, *stream;
  unsigned total_ops;                // of the plan: the last one may write the caller's output
  int result_slot;                   // -1: the result is copied out at the end
  int rc = GPQ_OK;
  int PB = -1, pair_slot[2] = {-1, -1};

  AlgoDevice(const gpq_algo::Book &plan, const AlgoPlan &lay, uint64_t *o0, uint64_t *o1, const uint64_t *c0, const uint64_t *c1, const uint64_t *k0,
             const uint64_t *k1, const uint64_t *m_, void *workspace, void *stream_)
      : gpq_algo::Book(plan.c, plan.W, plan.batch, plan.logqL, plan.logql0, plan.s, plan.dimpt_m, false), buffers(lay.buffers), in0(c0), in1(c1),
        rlk0(k0), rlk1(k1), m(m_), out0(o0), out1(o1), stream(stream_), total_ops(plan.nops), result_slot(plan.result_is_last_write() ? plan.result : -1) {
    char *w = (char *)workspace;
    for (unsigned i = 0; i < POOL; ++i) {
      b0[i] = i < buffers ? (uint64_t *)(w + 2 * lay.ct * i) : nullptr;
      b1[i] = i < buffers ? (uint64_t *)(w + 2 * lay.ct * i + lay.ct) : nullptr;
      ref[i] = 0;
    }
    mrep = (uint64_t *)(w + lay.pool + 2 * lay.pair);
    wsp = w + lay.pool + 2 * lay.pair + lay.m;
    for (int &a : at) a = -1;
    at[0] = IN;
    pt_nu = plan.pt_nu;
    if (lay.pair) {                                          // entries PB + 2 p + h: half h of double buffer p (they fit: algo_seq.hpp's static_assert)
      PB = (int)buffers;
      for (int p = 0; p < 2; ++p)
        for (int h = 0; h < 2; ++h) {
          b0[PB + 2 * p + h] = (uint64_t *)(w + lay.pool + p * lay.pair + h * lay.half);
          b1[PB + 2 * p + h] = (uint64_t *)(w + lay.pool + p * lay.pair + lay.pair / 2 + h * lay.half);
        }
    }
  }
  // slots x and y live in the halves of the double buffers (x in half 0, y beside it in half 1) and are squared together (sq2)
  void paired(int x, int y) { pair_slot[0] = x; pair_slot[1] = y; }
  bool in_pair(int ph) const { return PB >= 0 && ph >= PB && ph < PB + 4; }
  void second_input(const uint64_t *c0, const uint64_t *c1) { gpq_algo::Book::second_input(0, 0); in2_0 = c0; in2_1 = c1; at[1] = IN2; }
  const uint64_t *r0(int ph) const { return ph == IN ? in0 : ph == IN2 ? in2_0 : ph == OUT ? out0 : b0[ph]; }
  const uint64_t *r1(int ph) const { return ph == IN ? in1 : ph == IN2 ? in2_1 : ph == OUT ? out1 : b1[ph]; }
  uint64_t *w0(int ph) const { return ph == OUT ? out0 : b0[ph]; }
  uint64_t *w1(int ph) const { return ph == OUT ? out1 : b1[ph]; }
  bool broke(int code) { if (!rc) rc = code; if (!err) { err = code; why = "a launch failed"; } return false; }
  // where the next value of slot d goes; own_ok: the call may write over d's present buffer
  int place(int d, bool own_ok) {
    if (result_slot == d && nops + 1 == total_ops) return OUT;
    const int cur = at[d];
    if (PB >= 0 && d == pair_slot[1]) {                                          // half 1, beside its partner -- wherever it was before
      const int a = at[pair_slot[0]], ph = in_pair(a) ? PB + 2 * ((a - PB) / 2) + 1 : -1;
      if (ph >= 0 && (ph == cur ? own_ok : !ref[ph])) return ph;
    } else if (own_ok && cur >= 0 && cur < POOL && ref[cur] == 1) {
      return cur;
    } else if (PB >= 0 && d == pair_slot[0]) {                                   // half 0 of the other double buffer
      const int ph = in_pair(cur) ? PB + 2 * (1 - (cur - PB) / 2) : PB;
      if (!ref[ph]) return ph;
    } else {
      for (unsigned f = 0; f < buffers; ++f) if (!ref[f]) return (int)f;
    }
    broke(gpq_fail(GPQ_ERR_INVALID, "evaluator: out of temporaries"));
    return -1;
  }
  void settle(int d, int ph) {
    const int cur = at[d];
    if (cur == ph) return;
    if (cur >= 0 && cur < POOL) --ref[cur];
    if (ph >= 0 && ph < POOL) ++ref[ph];
    at[d] = ph;
  }

  bool mul(int d, int x, int y) {
    const int ph = place(d, d != x && d != y);                                  // gpq_he_mul_rs: outputs may not alias inputs
    if (ph < 0 || !Book::mul(d, x, y)) return false;
    const int px = at[x], py = at[y];
    const int e = gpq_he_mul_rs(c, w0(ph), w1(ph), r0(px), r1(px), r0(py), r1(py), rlk0, rlk1, W, logql(v[d].lv - 1), dimA, dimB, dimP, s, batch, wsp, stream);
    if (e) return broke(e);
    settle(d, ph);
    return true;
  }
  bool sq2(int x, int y) {
    const int px = at[x], py = at[y];
    if (!in_pair(px) || (px - PB) % 2 || py != px + 1) return broke(gpq_fail(GPQ_ERR_INVALID, "evaluator: the pair to square is not side by side"));
    const int ox = PB + 2 * (1 - (px - PB) / 2), oy = ox + 1;                   // gpq_he_mul_rs is never in place: into the other double buffer
    if (ref[ox] || ref[oy]) return broke(gpq_fail(GPQ_ERR_INVALID, "evaluator: out of temporaries"));
    if (!Book::sq2(x, y)) return false;
    const int e = gpq_he_mul_rs(c, b0[ox], b1[ox], b0[px], b1[px], b0[px], b1[px], rlk0, rlk1, W, logql(v[x].lv - 1), dimA, dimB, dimP, s, 2 * batch, wsp, stream);
    if (e) return broke(e);
    settle(x, ox);
    settle(y, oy);
    return true;
  }
  bool mulc(int d, int x, double re) {
    const int ph = place(d, true);                                             // gpq_he_mulpt_const: out may be the input of the same polynomial
    if (ph < 0 || !Book::mulc(d, x, re)) return false;
    const int px = at[x];
    const int e = gpq_he_mulpt_const(c, w0(ph), w1(ph), r0(px), r1(px), ca, 0, W, logql(v[d].lv - 1), dim, s, batch, nullptr, stream);
    if (e) return broke(e);
    settle(d, ph);
    return true;
  }
  bool mulpt(int d, int x) {
    const int ph = place(d, d != x);
    if (ph < 0 || !Book::mulpt(d, x)) return false;
    const int px = at[x];
    const size_t poly = (size_t)W << logn;
    for (unsigned k = 0; k < batch; ++k)                                        // one plaintext for the whole batch (as gpq_he_gemv hands out its diagonals)
      if (hipMemcpyAsync(mrep + k * poly, m, poly * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return broke(gpq_fail(GPQ_ERR_HIP, "gpq_he_exp: copying the plaintext failed"));
    const unsigned lq = logql(v[d].lv - 1);
    int e = gpq_he_mulpt(c, w0(ph), w1(ph), r0(px), r1(px), mrep, W, lq, dim, batch, wsp, stream);       // src/he-algo.c:449
    if (!e) e = gpq_he_rs(c, w0(ph), w1(ph), W, s, lq - s, batch, stream);                               // :450
    if (e) return broke(e);
    settle(d, ph);
    return true;
  }
  bool lin(int d, const gpq_algo::Term *t, unsigned K, unsigned lv_out, bool has_c = false, double re = 0.0, int csign = 1, int msign = 0) {
    const int ph = place(d, true);                                              // gpq_he_lin_const: out may be a term in the same position
    if (ph < 0 || !Book::lin(d, t, K, lv_out, has_c, re, csign, msign)) return false;
    const uint64_t *x0[3] = {nullptr, nullptr, nullptr}, *x1[3] = {nullptr, nullptr, nullptr};
    int sg[3] = {1, 1, 1};
    for (unsigned k = 0; k < K; ++k) { x0[k] = r0(at[t[k].slot]); x1[k] = r1(at[t[k].slot]); sg[k] = t[k].sign; }
    const int e = msign ? gpq_he_lin_pt(c, w0(ph), w1(ph), x0, x1, sg, K, m, msign, ca, 0, W, logql(lv_out), batch, stream)
                        : gpq_he_lin_const(c, w0(ph), w1(ph), x0, x1, sg, K, ca, 0, W, logql(lv_out), batch, stream);
    if (e) return broke(e);
    settle(d, ph);
    return true;
  }
  bool alias(int d, int x) {
    if (!Book::alias(d, x)) return false;
    settle(d, at[x]);
    return true;
  }
  bool ret(int d) {
    if (!Book::ret(d)) return false;
    if (at[d] == OUT) return true;
    const uint64_t *x0[3] = {r0(at[d]), nullptr, nullptr}, *x1[3] = {r1(at[d]), nullptr, nullptr};   // he_copy_ct(ct_dest, .): the value as it is (centred already)
    const int sg[3] = {1, 1, 1};
    const int e = gpq_he_lin_const(c, out0, out1, x0, x1, sg, 1, 0, 0, W, logql(v[d].lv), batch, stream);
    return e ? broke(e) : true;
  }
};

int he_algo(gpq_ctx *c, int kind, const char *who, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m,
            unsigned dimpt, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
            unsigned batch, void *workspace, void *stream) {
  int rc = check(c, 1, batch, who);
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !c0 || !c1 || !rlk0 || !rlk1 || !workspace || (kind == GPQ_ALGO_EXP && !m) || W < 1 || W > 64 || W < (logql + 63) / 64 ||
      c->logn < 1 || batch > 32767)
    return gpq_fail(GPQ_ERR_INVALID, "%s: bad arguments (W >= ceil(logql / 64))", who);
  // everything that can refuse the call is decided here, on the host, before the first launch
  gpq_algo::Book plan(c, W, batch, logqL, logql, logDelta, dimpt, false);
  if (!gpq_algo::run(plan, kind, iter)) return gpq_fail(plan.err, "%s: %s", who, plan.why);
  const size_t words = (size_t)batch * W * c->n;
  const bool in_place = out_c0 == c0 && out_c1 == c1;
  if (ranges_overlap(out_c0, words, out_c1, words) || ranges_overlap(out_c0, words, c1, words) || ranges_overlap(out_c1, words, c0, words) ||
      (!in_place && (ranges_overlap(out_c0, words, c0, words) || ranges_overlap(out_c1, words, c1, words))) ||
      (in_place && plan.result_is_last_write() && plan.last_mul_reads_input))
    return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs overlap each other or the inputs other than in the same position", who);
  const AlgoPlan lay = algo_plan(c, kind, W, batch, 0);
  AlgoDevice dev(plan, lay, out_c0, out_c1, c0, c1, rlk0, rlk1, m, workspace, stream);
  StageRange stage(who);
  gpq_algo::run(dev, kind, iter);
  if (dev.rc) return dev.rc;
  if (dev.err) return gpq_fail(dev.err, "%s: %s", who, dev.why);
  return launched(who);
}

// gpq_he_cmp (b0 / b1: the second ciphertext, m NULL) and gpq_he_cmppt (m: the plaintext) behind one set of checks
int he_cmp_call(gpq_ctx *c, const char *who, bool with_pt, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                const uint64_t *b1, const uint64_t *m, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql,
                unsigned logDelta, unsigned iter, unsigned t, unsigned batch, void *workspace, void *stream) {
  int rc = check(c, 1, batch, who);
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !a0 || !a1 || (with_pt ? !m : (!b0 || !b1)) || !rlk0 || !rlk1 || !workspace || W < 1 || W > 64 || W < (logql + 63) / 64 ||
      c->logn < 1 || batch > 32767)
    return gpq_fail(GPQ_ERR_INVALID, "%s: bad arguments (W >= ceil(logql / 64))", who);
  gpq_algo::Book plan(c, W, batch, logqL, logql, logDelta, 0, false);
  if (!with_pt) plan.second_input(1.0, 0.0);
  if (!gpq_algo::run_cmp(plan, iter, t, with_pt)) return gpq_fail(plan.err, "%s: %s", who, plan.why);
  const size_t words = (size_t)batch * W * c->n;
  const bool in_place = out_c0 == a0 && out_c1 == a1;
  bool bad = ranges_overlap(out_c0, words, out_c1, words) || ranges_overlap(out_c0, words, a1, words) || ranges_overlap(out_c1, words, a0, words) ||
             (!in_place && (ranges_overlap(out_c0, words, a0, words) || ranges_overlap(out_c1, words, a1, words))) ||
             (in_place && plan.result_is_last_write() && plan.last_mul_reads_input);        // the plan writes the output in its last operation only
  if (with_pt) bad = bad || ranges_overlap(out_c0, words, m, (size_t)W * c->n) || ranges_overlap(out_c1, words, m, (size_t)W * c->n);
  else bad = bad || ranges_overlap(out_c0, words, b0, words) || ranges_overlap(out_c0, words, b1, words) || ranges_overlap(out_c1, words, b0, words) ||
             ranges_overlap(out_c1, words, b1, words);
  if (bad) return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs overlap each other or an input other than the first in the same position", who);
  const AlgoPlan lay = algo_plan(c, gpq_algo::CMP_SINGLES, false, W, batch, 0, true);
  AlgoDevice dev(plan, lay, out_c0, out_c1, a0, a1, rlk0, rlk1, m, workspace, stream);
  dev.paired(gpq_algo::CMP_AN, gpq_algo::CMP_BN);
  if (!with_pt) dev.second_input(b0, b1);
  StageRange stage(who);
  gpq_algo::run_cmp(dev, iter, t, with_pt);
  if (dev.rc) return dev.rc;
  if (dev.err) return gpq_fail(dev.err, "%s: %s", who, dev.why);
  return launched(who);
}

}  // namespace

extern "C" int gpq_he_cmp_rounds(unsigned alpha) {
  if (alpha < 1 || alpha > 52) return -1;                 // log2(0), and 1 + 2^-53 == 1.0: the reference's conversion of +-inf is undefined
  const double cc = 1 + pow(2, -(int)alpha);              // src/he-algo.c:519
  return (int)(unsigned)log2(alpha / log2(cc));           // :520
}

extern "C" int gpq_he_cmp_depth(unsigned iter, unsigned t) { return gpq_algo::cmp_depth(iter, t); }

extern "C" size_t gpq_he_cmp_workspace_bytes(gpq_ctx *c, int with_pt, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                                             unsigned t, unsigned batch) {
  if (!c || !W || !batch) { (void)gpq_fail(GPQ_ERR_INVALID, "gpq_he_cmp_workspace_bytes: bad arguments"); return 0; }
  gpq_algo::Book plan(c, W, batch, logqL, logql, logDelta, 0, true);
  if (!with_pt) plan.second_input(1.0, 0.0);
  if (!gpq_algo::run_cmp(plan, iter, t, with_pt != 0)) { (void)gpq_fail(plan.err, "gpq_he_cmp_workspace_bytes: %s", plan.why); return 0; }
  return algo_plan(c, gpq_algo::CMP_SINGLES, false, W, batch, plan.ws, true).total;
}

extern "C" int gpq_he_cmp(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *a_c0, const uint64_t *a_c1, const uint64_t *b_c0,
                          const uint64_t *b_c1, const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql,
                          unsigned logDelta, unsigned iter, unsigned t, unsigned batch, void *workspace, void *stream) {
  return he_cmp_call(c, "gpq_he_cmp", false, out_c0, out_c1, a_c0, a_c1, b_c0, b_c1, nullptr, rlk0, rlk1, W, logqL, logql, logDelta, iter, t, batch,
                     workspace, stream);
}
extern "C" int gpq_he_cmppt(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m,
                            const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                            unsigned t, unsigned batch, void *workspace, void *stream) {
  return he_cmp_call(c, "gpq_he_cmppt", true, out_c0, out_c1, c0, c1, nullptr, nullptr, m, rlk0, rlk1, W, logqL, logql, logDelta, iter, t, batch,
                     workspace, stream);
}

extern "C" int gpq_he_algo_depth(int kind, unsigned iter) { return gpq_algo::depth(kind, iter > 4096 ? 4096 : iter); }

extern "C" size_t gpq_he_algo_workspace_bytes(gpq_ctx *c, int kind, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                                              unsigned batch) {
  if (!c || !W || !batch || gpq_algo::depth(kind, 0) < 0) { (void)gpq_fail(GPQ_ERR_INVALID, "gpq_he_algo_workspace_bytes: bad arguments"); return 0; }
  gpq_algo::Book plan(c, W, batch, logqL, logql, logDelta, kind == GPQ_ALGO_EXP ? (logql + 1 + logDelta + c->logn) / 59u + 1 : 0, true);
  if (!gpq_algo::run(plan, kind, iter)) { (void)gpq_fail(plan.err, "gpq_he_algo_workspace_bytes: %s", plan.why); return 0; }
  return algo_plan(c, kind, W, batch, plan.ws).total;
}

extern "C" int gpq_he_inv(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0, const uint64_t *rlk1,
                          unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter, unsigned batch, void *workspace, void *stream) {
  return he_algo(c, GPQ_ALGO_INV, "gpq_he_inv", out_c0, out_c1, c0, c1, nullptr, 0, rlk0, rlk1, W, logqL, logql, logDelta, iter, batch, workspace, stream);
}
extern "C" int gpq_he_sqrt(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0, const uint64_t *rlk1,
                           unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter, unsigned batch, void *workspace, void *stream) {
  return he_algo(c, GPQ_ALGO_SQRT, "gpq_he_sqrt", out_c0, out_c1, c0, c1, nullptr, 0, rlk0, rlk1, W, logqL, logql, logDelta, iter, batch, workspace, stream);
}
extern "C" int gpq_he_sigmoid(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0,
                              const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned batch, void *workspace, void *stream) {
  return he_algo(c, GPQ_ALGO_SIGMOID, "gpq_he_sigmoid", out_c0, out_c1, c0, c1, nullptr, 0, rlk0, rlk1, W, logqL, logql, logDelta, 0, batch, workspace, stream);
}
extern "C" int gpq_he_log(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *rlk0, const uint64_t *rlk1,
                          unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned batch, void *workspace, void *stream) {
  return he_algo(c, GPQ_ALGO_LOG, "gpq_he_log", out_c0, out_c1, c0, c1, nullptr, 0, rlk0, rlk1, W, logqL, logql, logDelta, 0, batch, workspace, stream);
}
extern "C" int gpq_he_exp(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *c0, const uint64_t *c1, const uint64_t *m, unsigned dimpt,
                          const uint64_t *rlk0, const uint64_t *rlk1, unsigned W, unsigned logqL, unsigned logql, unsigned logDelta, unsigned iter,
                          unsigned batch, void *workspace, void *stream) {
  return he_algo(c, GPQ_ALGO_EXP, "gpq_he_exp", out_c0, out_c1, c0, c1, m, dimpt, rlk0, rlk1, W, logqL, logql, logDelta, iter, batch, workspace, stream);
}
