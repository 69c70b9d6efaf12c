// bridge_algo.hpp -- host fragment of bridge.hip: gpq_he_lin_const (algo_kernels.hpp) and the evaluators gpq_he_inv / gpq_he_sqrt / gpq_he_sigmoid /
// gpq_he_log / gpq_he_exp (include/gpqhe_hip_algo.h).  The sequences themselves are algo_seq.hpp's; AlgoDevice below is the implementation of
// their operations that launches -- through the public entry points only (gpq_he_mul_rs, gpq_he_mulpt_const, gpq_he_mulpt, gpq_he_rs,
// gpq_he_lin_const): an evaluator is straight-line host code around calls that exist.
#pragma once
#include "algo_seq.hpp"

extern "C" int gpq_he_lin_const(gpq_ctx *c, uint64_t *out_c0, uint64_t *out_c1, const uint64_t *const x_c0[3], const uint64_t *const x_c1[3],
                                const int sign[3], unsigned K, int64_t a, int64_t b, unsigned W, unsigned logql, unsigned batch, void *stream) {
  int rc = check(c, 1, batch, "gpq_he_lin_const");
  if (rc) return rc;
  if (!out_c0 || !out_c1 || !x_c0 || !x_c1 || !sign || K < 1 || K > 3 || W < 1 || W > 64 || logql < 1 || logql > 64 * W || c->logn < 1 || batch > 32767)
    return gpq_fail(GPQ_ERR_INVALID, "gpq_he_lin_const: bad arguments (1 <= K <= 3, 1 <= logql <= 64 W)");
  LinConstArgs k{out_c0, out_c1, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, a, b, 0u, W, c->logn, logql};
  const size_t words = (size_t)batch * W * c->n;
  if (ranges_overlap(out_c0, words, out_c1, words)) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_lin_const: the outputs overlap");
  for (unsigned t = 0; t < K; ++t) {
    if (!x_c0[t] || !x_c1[t] || (sign[t] != 1 && sign[t] != -1)) return gpq_fail(GPQ_ERR_INVALID, "gpq_he_lin_const: term %u is NULL or its sign is not +-1", t);
    // a lane reads and writes its own coefficient only: the output may BE a term's slab of the same polynomial, and may overlap nothing else
    if ((x_c0[t] != out_c0 && ranges_overlap(out_c0, words, x_c0[t], words)) || (x_c1[t] != out_c1 && ranges_overlap(out_c1, words, x_c1[t], words)) ||
        ranges_overlap(out_c0, words, x_c1[t], words) || ranges_overlap(out_c1, words, x_c0[t], words))
      return gpq_fail(GPQ_ERR_INVALID, "gpq_he_lin_const: an output overlaps term %u other than in the same position", t);
    k.x0[t] = x_c0[t]; k.x1[t] = x_c1[t];
    if (sign[t] < 0) k.neg |= 1u << t;
  }
  {
    ProfScope prof(c, GPQ_K_LIN_CONST, (hipStream_t)stream);
    const dim3 grid((c->n + 255) / 256, 2 * batch), block(256);
    if (K == 1) hipLaunchKernelGGL(he_lin_const<1>, grid, block, 0, (hipStream_t)stream, k);
    else if (K == 2) hipLaunchKernelGGL(he_lin_const<2>, grid, block, 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(he_lin_const<3>, grid, block, 0, (hipStream_t)stream, k);
  }
  return launched("gpq_he_lin_const");
}

namespace {

// Workspace of an evaluator call: the named temporaries and one spare (c0 | c1 of `batch` ciphertexts each), he_exp's plaintext once per
// ciphertext (gpq_he_mulpt multiplies slab by slab), then the products' own workspace, the largest of the levels.
struct AlgoPlan { size_t ct, pool, m, total; unsigned buffers; };
AlgoPlan algo_plan(const gpq_ctx *c, int kind, unsigned W, unsigned batch, size_t ws) {
  AlgoPlan p;
  p.buffers = gpq_algo::temporaries(kind) + 1;
  p.ct = align64((size_t)batch * W * c->n * 8);
  p.pool = 2 * p.ct * p.buffers;
  p.m = kind == GPQ_ALGO_EXP ? p.ct : 0;
  p.total = p.pool + p.m + align64(ws);
  return p;
}

// The operations of algo_seq.hpp on the device.  A slot's value lives in one of the workspace's buffers, in the caller's input (slot 0, never
// written) or -- the result, when the sequence's last operation writes it -- in the caller's output.  A slot is rewritten in place only where the
// entry point allows it and nobody else names the buffer (alias); otherwise the new value takes a free buffer and the old one is released.
struct AlgoDevice : gpq_algo::Book {
  enum { POOL = gpq_algo::SLOTS, IN = POOL, OUT = POOL + 1 };
  uint64_t *b0[POOL], *b1[POOL];
  int ref[POOL], at[gpq_algo::SLOTS];
  unsigned buffers;
  const uint64_t *in0, *in1, *rlk0, *rlk1, *m;
  uint64_t *out0, *out1, *mrep;
  void *wsp, *stream;
  unsigned total_ops;                // of the plan: the last one may write the caller's output
  int result_slot;                   // -1: the result is copied out at the end
  int rc = GPQ_OK;

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
    mrep = (uint64_t *)(w + lay.pool);
    wsp = w + lay.pool + lay.m;
    for (int &a : at) a = -1;
    at[0] = IN;
  }
  const uint64_t *r0(int ph) const { return ph == IN ? in0 : ph == OUT ? out0 : b0[ph]; }
  const uint64_t *r1(int ph) const { return ph == IN ? in1 : ph == OUT ? out1 : b1[ph]; }
  uint64_t *w0(int ph) const { return ph == OUT ? out0 : b0[ph]; }
  uint64_t *w1(int ph) const { return ph == OUT ? out1 : b1[ph]; }
  bool broke(int code) { if (!rc) rc = code; if (!err) { err = code; why = "a launch failed"; } return false; }
  // where the next value of slot d goes; own_ok: the call may write over d's present buffer
  int place(int d, bool own_ok) {
    if (result_slot == d && nops + 1 == total_ops) return OUT;
    const int cur = at[d];
    if (own_ok && cur >= 0 && cur < POOL && ref[cur] == 1) return cur;
    for (unsigned f = 0; f < buffers; ++f) if (!ref[f]) return (int)f;
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
  bool mulc(int d, int x, double re) {
    const int ph = place(d, true);                                              // gpq_he_mulpt_const: out may be the input of the same polynomial
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
  bool lin(int d, const gpq_algo::Term *t, unsigned K, unsigned lv_out, bool has_c = false, double re = 0.0, int csign = 1) {
    const int ph = place(d, true);                                              // gpq_he_lin_const: out may be a term in the same position
    if (ph < 0 || !Book::lin(d, t, K, lv_out, has_c, re, csign)) return false;
    const uint64_t *x0[3] = {nullptr, nullptr, nullptr}, *x1[3] = {nullptr, nullptr, nullptr};
    int sg[3] = {1, 1, 1};
    for (unsigned k = 0; k < K; ++k) { x0[k] = r0(at[t[k].slot]); x1[k] = r1(at[t[k].slot]); sg[k] = t[k].sign; }
    const int e = gpq_he_lin_const(c, w0(ph), w1(ph), x0, x1, sg, K, ca, 0, W, logql(lv_out), batch, stream);
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

}  // namespace

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
