// bridge_tail.hpp -- host fragment of bridge.hip: the relinearisation tail of he_mul / he_swk (src/he-mult.c:67-77, src/he-automorphism.c:68-76)
// for q_l = 2^logql.  relin_tail() routes a call to one of three flows; tail_prescale_mode() tells the key switch before it which weights to leave on.
#pragma once
namespace {

struct TailPlan { unsigned Wr, cnt; size_t words, bytes; };

int tail_plan(gpq_ctx *c, unsigned W, unsigned dimP, unsigned dimB, unsigned polys, TailPlan *p) {
  gpq_bridge_basis *bp;
  int rc = get_basis(c, 0, dimP, &bp);
  if (rc) return rc;
  if (dimB <= dimP) return gpq_fail(GPQ_ERR_INVALID, "relin: dimB=%u must exceed dimP=%u", dimB, dimP);
  p->Wr = bp->pbits / 64 + 1;
  p->cnt = dimB - dimP;
  p->words = (size_t)polys * ((size_t)(p->Wr + 2 * p->cnt + W) << c->logn);
  p->bytes = p->words * 8 + ((size_t)polys << c->logn);
  return GPQ_OK;
}

// "The one-product tables exist": the settings allow that tail, and the front's tables (its exact fall-back re-runs the front) and the product's
// matrix are there (built on first use).  Asked by tail_prescale_mode, gpq_relin_tail_overwriting and relin_tail; what else each needs stands at the call.
int tail_product_tables(gpq_ctx *c, unsigned dimP, unsigned dimB, gpq_relin_tables *rt, gpq_bridge_basis *bp, gpq_bridge_basis *bq, bool *ok) {
  *ok = false;
  if (!c->set.bridge_mfma || c->logn < 6 || !c->set.tail_direct || c->set.exact_crt) return GPQ_OK;
  int rc;
  if ((rc = get_relin_front(c, dimP, dimB, rt, bp, bq)) || (rt->d_bfrag && (rc = get_tail_direct(c, dimP, dimB, rt)))) return rc;
  *ok = rt->d_bfrag && rt->direct.d_bfrag;
  return GPQ_OK;
}

// How the key switch of gpq_he_mul / gpq_he_swk may scale its output for the tail that follows: 0 = not at all, 1 = the limbs of P by
// (P/p_d)^-1 (any tail), 2 = also the limbs above P by w_j (the matrix-core front only: its exact fallbacks read those limbs through
// the same tables), 3 = every limb by (Pi_B/p_d)^-1 for the one-product tail.  *tabs = the per-limb table the inverse pass reads.
int tail_prescale_mode(gpq_ctx *c, unsigned dimP, unsigned dimB, const LimbTab **tabs, int *mode) {
  *tabs = nullptr; *mode = 0;
  if (!can_prescale(c)) return GPQ_OK;
  gpq_bridge_basis *bp, *bq;
  gpq_relin_tables *rt;
  int rc;
  if ((rc = get_basis(c, 0, dimP, &bp)) || (rc = get_basis(c, dimP, dimB - dimP, &bq)) || (rc = get_relin(c, dimP, dimB, &rt))) return rc;
  if (c->set.bridge_mfma && c->logn >= 6 && (rc = get_relin_front(c, dimP, dimB, rt, bp, bq))) return rc;
  bool product = false;
  if ((rc = tail_product_tables(c, dimP, dimB, rt, bp, bq, &product))) return rc;
  if (product && rt->d_tabs_direct) { *tabs = rt->d_tabs_direct; *mode = 3; return GPQ_OK; }
  if (c->set.bridge_mfma && c->logn >= 6 && rt->d_bfrag && rt->d_tabs_w && c->set.prescale_upper) { *tabs = rt->d_tabs_w; *mode = 2; return GPQ_OK; }
  *mode = 1;
  return get_scaled_tabs(c, bp, tabs);
}

// The addend of the relinearisation tail as LIMBS (he_mul: d0hat | d1hat, src/he-mult.c:139,141 never leave RNS form before the tail):
// [polys][dimA][n] weighted for the CRT over bA; scratch = [polys][W][n] words for the coefficients the exact kernels redo (or for all of
// them when the streaming kernel does not cover the shape).
struct TailD { const uint64_t *hat; gpq_bridge_basis *bA; unsigned dimA; uint64_t *scratch; };

// The tail's workspace (tail_plan), carved here and nowhere else: r = x mod P as words, its residues above P, Q's residues, Q as words, a tie
// byte per coefficient.  The front's flag bytes (flags: round bits, amb: "cannot decide"; one per coefficient each) lie in rhat's place: only
// the integer-VALU flow keeps r's residues, and it has no flags.
struct TailWs {
  uint64_t *r, *rhat, *qhat, *qc;
  unsigned char *tie, *flags, *amb;
  TailWs(void *ws, const TailPlan &tp, unsigned W, size_t pn)      // pn = polys * n
      : r((uint64_t *)ws), rhat(r + pn * tp.Wr), qhat(rhat + pn * tp.cnt), qc(qhat + pn * tp.cnt), tie((unsigned char *)(qc + pn * W)),
        flags((unsigned char *)rhat), amb(flags + pn) {}
};
// one relin_tail call as its flows see it: P = bp, Pi' = bq (the limbs above P); in_place = out IS d, so Q must not be parked in `out`
struct Tail {
  gpq_ctx *c; hipStream_t s; gpq_bridge_basis *bp, *bq; gpq_relin_tables *rt; TailPlan tp; TailWs w;
  Two<uint64_t> out; const uint64_t *chat; Two<const uint64_t> dbig; unsigned W, dimP, dimB, logql, polys; bool in_place;
  const uint64_t *piq() const { return bq->d_pmult + (size_t)5 * (bq->WP + 1); }
};

// one of the small masked kernels of 256 threads (bridge_limb_scale, bridge_roundfix, bridge_addround, bridge_rescale_masked)
template <typename Args>
void launch_masked(const Tail &t, void (*kernel)(Args), const FlagScope &scope, const Args &a) {
  ProfScope prof(t.c, GPQ_K_BRIDGE_EXACT, t.s);
  hipLaunchKernelGGL(kernel, masked_grid(scope, 256, t.c->n, t.polys), dim3(256), 0, t.s, a);
}

// get_tail_direct's matrix as a stream (bridge_stream.hpp), with the addend's CRT in the same kernel when it comes as limbs.  *scope = the
// launch's per-wave words for the masked kernels behind it; *done = false: not covered (shape, settings).  The caller has sized c->d_redo.
int tail_stream(const Tail &t, const TailD *dh, FlagScope *scope, bool *done, unsigned rs) {
  gpq_ctx *c = t.c;
  const unsigned W = t.W, dimB = t.dimB, logql = t.logql, polys = t.polys;
  *done = false;
  const unsigned need = (logql + 63) / 64;
  if (!c->set.stream_bridge || W > 14 || W < need || logql > 896) return GPQ_OK;
  int KST, KSD = 0;
  if (dh) {
    if (!stream_fast_ok(c, dh->bA, logql)) return GPQ_OK;
    if (dimB <= 32 && dh->dimA <= 16) { KST = 8; KSD = 4; }
    else if (dimB <= 48 && dh->dimA <= 32) { KST = 12; KSD = 8; }
    else return GPQ_OK;
  } else {
    if (dimB <= 24) KST = 6; else if (dimB <= 48) KST = 12; else return GPQ_OK;
  }
  gpq_recon_mfma *tt, *td = nullptr;
  int rc;
  if ((rc = get_tail_direct_padded(c, t.dimP, dimB, t.rt, KST, &tt))) return rc;
  if (dh && (rc = get_addend_rows(c, dh->bA, KSD, &td))) return rc;
  if (!tt->d_bfrag || tt->KS != (unsigned)KST || (dh && (!td->d_bfrag || td->KS != (unsigned)KSD))) return GPQ_OK;
  const size_t lds = (size_t)(KST + KSD) * 5 * 1024 + (size_t)2 * 65 * kTailRow * 8;
  if (lds > kStreamLdsMax) return GPQ_OK;
  if ((rc = ensure_wave_any(c, t.s))) return rc;
  const unsigned groups = (c->n >> 6) * polys, blocks = stream_blocks(groups);
  const size_t chat_bytes = ((size_t)polys * dimB << c->logn) * 8, dhat_bytes = dh ? ((size_t)polys * dh->dimA << c->logn) * 8 : 0;
  if (chat_bytes >= 0xfffff000ull || dhat_bytes >= 0xfffff000ull) return GPQ_OK;
  TailStreamArgs a{t.chat, dh ? dh->hat : nullptr, chat_bytes, dhat_bytes, t.dbig, t.out, (const v4i *)tt->d_bfrag, tt->d_kc, tt->d_pm,
                   dh ? (const v4i *)td->d_bfrag : nullptr, dh ? td->d_kc : nullptr, dh ? td->d_pm : nullptr,
                   c->d_redo, t.w.tie, t.w.amb, c->d_wave_any, dimB, dh ? dh->dimA : 0u, c->logn, W, logql, groups, c->set.debug_force_redo,
                   rs, rs ? logql - rs : 0u};
  ProfScope prof(c, GPQ_K_TAIL_STREAM, t.s);
  if (dh && KST == 8) rc = launch_tail_stream_t<8, 4, true, 6>(a, lds, blocks, t.s);
  else if (dh) rc = launch_tail_stream_t<12, 8, true, 5>(a, lds, blocks, t.s);
  else if (KST == 6) rc = launch_tail_stream_t<6, 0, false, 3>(a, lds, blocks, t.s);
  else rc = launch_tail_stream_t<12, 0, false, 4>(a, lds, blocks, t.s);
  if (rc) return rc;
  *scope = FlagScope{c->d_wave_any, blocks * kStreamWaves, groups};
  *done = true;
  return GPQ_OK;
}

// The masked exact finish on the coefficients a fast kernel flagged: r of the ambiguous ones (amb), their round bits, Q's exact CRT of the
// flagged ones (c->d_redo) into `out`, bridge_addround.  `front` re-runs the front on the flagged groups first: Q's residues, flags and amb
// of those groups (chat's weights are off them: plain limbs).  scope: the launch that wrote the masks; fuse_post: all behind the front in
// ONE launch (bridge_fallback_tail_post).
int tail_exact_finish(const Tail &t, const RelinFrontArgs &front, const FlagScope &scope, bool fuse_post) {
  gpq_ctx *c = t.c;
  const TailWs &w = t.w;
  int rc;
  if ((rc = launch_relin_front(c, t.rt->KS, front, t.rt->lds_bytes, t.s))) return rc;
  ReconExtra only_amb;
  only_amb.only = w.amb; only_amb.scope = scope;
  RoundFixArgs rf{w.r, t.bp->d_phalf, w.amb, w.flags, t.tp.Wr, c->logn, scope};
  ReconExtra q;
  q.prescaled = true; q.exact_only = true; q.only = c->d_redo; q.big_b = t.out.b; q.split = t.out.split; q.scope = scope;
  AddRoundArgs ar{t.out, Two<const uint64_t>{t.out.a, t.out.b, t.out.split}, nullptr, t.dbig, t.bp->d_phalf, t.piq(), w.tie, t.W, t.tp.Wr, c->logn, t.logql,
                  c->d_redo, w.flags, scope};
  if (fuse_post) {
    ProfScope prof(c, GPQ_K_BRIDGE_EXACT, t.s);
    const ReconstructArgs rr = exact_args(c, t.bp, w.r, t.tp.Wr, t.chat, t.dimB, 0, 0, false, nullptr, c->logn, only_amb);
    const ReconstructArgs qq = exact_args(c, t.bq, t.out.a, t.W, w.qhat, t.tp.cnt, 0, t.logql, true, w.tie, c->logn, q);
    const dim3 grid = masked_grid(scope, 128, c->n, t.polys);
    if (t.bp->WP == 16) hipLaunchKernelGGL((bridge_fallback_tail_post<16, 32>), grid, dim3(128), 0, t.s, rr, rf, qq, ar);
    else hipLaunchKernelGGL((bridge_fallback_tail_post<8, 16>), grid, dim3(128), 0, t.s, rr, rf, qq, ar);
    return GPQ_OK;
  }
  if ((rc = launch_reconstruct(c, t.bp, w.r, t.tp.Wr, t.chat, t.dimB, 0, t.polys, 0, false, nullptr, t.s, -1, only_amb))) return rc;
  launch_masked(t, bridge_roundfix, scope, rf);
  if ((rc = launch_reconstruct(c, t.bq, t.out.a, t.W, w.qhat, t.tp.cnt, 0, t.polys, t.logql, true, w.tie, t.s, -1, q))) return rc;
  launch_masked(t, bridge_addround, scope, ar);
  return GPQ_OK;
}

// where he_mul's addend lies as words once its CRT has run into dh->scratch
Two<const uint64_t> addend_words(const Tail &t, const TailD *dh) { return {dh->scratch, dh->scratch + (size_t)t.out.split * t.W * t.c->n, t.out.split}; }

// Flow 1, the one-product tail.  The limbs carry the CRT weights of the whole basis (gpq_keyswitch_scaled with get_tail_direct's table): ONE
// product gives floor(x/P), the rounding decision and the centring of x -- as a stream (tail_stream) or as bridge_reconstruct_low_mfma<16>.
// `chat` is the caller's scratch here (c0hat | c1hat of the workspace): the groups of 64 coefficients the product cannot decide get their
// weights taken off in place and go through the exact finish.  Behind the streaming kernel the chains whose hand-overs stay inside a thread
// are ONE launch each (bridge_fallback_tail_pre / _post): pre = the addend's exact CRT + the weights off; the front re-run; post.  Three
// launches where there were seven.  rs / rs_done (gpq_he_mul_rs): the streaming kernel rescales what it decides; what it flagged is
// written unrescaled by the exact kernels and rescaled here (same flags, same scope).
int tail_product(Tail t, const TailD *dh, unsigned rs, bool *rs_done) {
  gpq_ctx *c = t.c;
  const unsigned gpp = c->n >> 6;
  int rc;
  FlagScope scope = kNoScope;
  bool streamed = false;
  if ((rc = tail_stream(t, dh, &scope, &streamed, rs_done ? rs : 0u))) return rc;
  const bool fuse_pre = streamed && dh && (dh->bA->WP == 32 || dh->bA->WP == 16);
  const bool fuse_post = streamed && ((t.bp->WP == 16 && t.bq->WP == 32) || (t.bp->WP == 8 && t.bq->WP == 16));
  LimbScaleArgs un{c->d_tabs, const_cast<uint64_t *>(t.chat), t.rt->d_unscale, c->d_redo, t.dimB, c->logn, scope};
  if (dh) {
    // the addend as words: for the flagged coefficients only behind the streaming kernel (exact CRT), for all of them otherwise
    ReconExtra dx;
    dx.prescaled = true;
    if (streamed) { dx.exact_only = true; dx.only = c->d_redo; dx.scope = scope; }
    if (fuse_pre) {
      ProfScope prof(c, GPQ_K_BRIDGE_EXACT, t.s);
      const ReconstructArgs dd = exact_args(c, dh->bA, dh->scratch, t.W, dh->hat, dh->dimA, 0, t.logql, true, nullptr, c->logn, dx);
      const dim3 grid = masked_grid(scope, 128, c->n, t.polys);
      if (dh->bA->WP == 32) hipLaunchKernelGGL((bridge_fallback_tail_pre<32>), grid, dim3(128), 0, t.s, dd, un);
      else hipLaunchKernelGGL((bridge_fallback_tail_pre<16>), grid, dim3(128), 0, t.s, dd, un);
    } else if ((rc = launch_reconstruct(c, dh->bA, dh->scratch, t.W, dh->hat, dh->dimA, 0, t.polys, t.logql, true, nullptr, t.s, -1, dx))) return rc;
    t.dbig = addend_words(t, dh);
  }
  if (!streamed) {
    ReconMfmaArgs m{t.chat, t.out, (const v4i *)t.rt->direct.d_bfrag, t.rt->direct.d_lk, t.rt->direct.d_kc, t.rt->direct.d_pm, c->d_redo, t.w.tie, t.dimB,
                    t.rt->direct.KS, c->logn, t.W, t.logql, t.dimB, 0, gpp, gpp * t.polys, t.dbig, nullptr, 1u, 104u, t.w.amb};
    ProfScope prof(c, GPQ_K_RELIN_TAIL_DIRECT, t.s);
    if ((rc = launch_low_mfma<16>(m, t.rt->direct.lds_bytes, t.s))) return rc;
  }
  if (!fuse_pre) launch_masked(t, bridge_limb_scale, scope, un);      // weights off the flagged groups
  // the exact sequence on the flagged groups: front (re-run, writing its flags), r for its ambiguous ones, round bits, Q, finish
  RelinFrontArgs f{t.chat, t.w.qhat, (const v4i *)t.rt->d_bfrag, t.rt->d_lk, t.rt->d_pk, t.rt->d_tkp, t.rt->d_kf, t.w.flags, t.w.amb,
                   t.dimB, t.dimP, t.tp.cnt, c->logn, t.rt->NT, gpp, gpp * t.polys, c->d_redo, 0u, 0u, scope};
  if ((rc = tail_exact_finish(t, f, scope, fuse_post))) return rc;
  if (rs && rs_done && streamed) {
    launch_masked(t, bridge_rescale_masked, scope, RescaleMaskedArgs{t.out, c->d_redo, t.W, c->logn, rs, t.logql - rs, scope});
    *rs_done = true;
  }
  return GPQ_OK;
}

// Flow 2, the matrix-core front as two kernels: the exact kernels only see the coefficients whose rounding the fixed-point estimates cannot
// decide.  The one finish that is NOT tail_exact_finish: Q's CRT may take the fast path, which then finishes the tail itself.
int tail_front(const Tail &t, const RelinFrontArgs &f, bool prescaled) {
  gpq_ctx *c = t.c;
  const TailWs &w = t.w;
  int rc;
  if ((rc = launch_relin_front(c, t.rt->KS, f, t.rt->lds_bytes, t.s))) return rc;
  ReconExtra only_amb;
  only_amb.only = w.amb; only_amb.prescaled = prescaled;
  if ((rc = launch_reconstruct(c, t.bp, w.r, t.tp.Wr, t.chat, t.dimB, 0, t.polys, 0, false, nullptr, t.s, -1, only_amb))) return rc;
  launch_masked(t, bridge_roundfix, kNoScope, RoundFixArgs{w.r, t.bp->d_phalf, w.amb, w.flags, t.tp.Wr, c->logn});
  bool fused = false;
  ReconExtra q;
  q.prescaled = true; q.fused = &fused;
  // Fused finish straight into `out` (the exact kernel parks Q of its few coefficients there before bridge_addround
  // adds d, so `out` must not BE d); otherwise Q goes to qc and bridge_addround finishes every coefficient.
  const bool direct = !t.in_place;
  if (direct) { q.addend = t.dbig; q.rflags = w.flags; q.big_b = t.out.b; q.split = t.out.split; }
  if ((rc = launch_reconstruct(c, t.bq, direct ? t.out.a : w.qc, t.W, w.qhat, t.tp.cnt, 0, t.polys, t.logql, true, w.tie, t.s, -1, q))) return rc;
  launch_masked(t, bridge_addround, kNoScope,
                AddRoundArgs{t.out, direct ? Two<const uint64_t>{t.out.a, t.out.b, t.out.split} : Two<const uint64_t>{w.qc, nullptr, ~0u}, nullptr, t.dbig,
                             t.bp->d_phalf, t.piq(), w.tie, t.W, t.tp.Wr, c->logn, t.logql, fused ? c->d_redo : nullptr, w.flags});
  return GPQ_OK;
}

// Flow 3, the integer-VALU exact tail: r = x mod P as words, its residues over the limbs above P, the exact division, Q's CRT, the finish
int tail_exact(const Tail &t, bool prescaled) {
  gpq_ctx *c = t.c;
  const TailWs &w = t.w;
  int rc;
  ReconExtra rx;
  rx.prescaled = prescaled;
  // r = x mod P from the first dimP limbs, unsigned
  if ((rc = launch_reconstruct(c, t.bp, w.r, t.tp.Wr, t.chat, t.dimB, 0, t.polys, 0, false, nullptr, t.s, -1, rx))) return rc;
  if ((rc = launch_decompose(c, w.rhat, w.r, t.tp.Wr, t.dimP, t.tp.cnt, t.polys, t.s))) return rc;
  ExactDivArgs e{c->d_tabs, t.chat, w.rhat, w.qhat, t.rt->d_pinv, t.dimB, t.dimP, t.tp.cnt, c->logn};
  { ProfScope prof(c, GPQ_K_BRIDGE_EXACT, t.s); hipLaunchKernelGGL(bridge_exactdiv, dim3((c->n + 255) / 256, t.polys, t.tp.cnt), dim3(256), 0, t.s, e); }
  // Q = (x - r)/P over the remaining limbs, centred, already reduced smod 2^logql
  if ((rc = launch_reconstruct(c, t.bq, w.qc, t.W, w.qhat, t.tp.cnt, 0, t.polys, t.logql, true, w.tie, t.s))) return rc;
  launch_masked(t, bridge_addround, kNoScope,
                AddRoundArgs{t.out, Two<const uint64_t>{w.qc, nullptr, ~0u}, w.r, t.dbig, t.bp->d_phalf, t.piq(), w.tie, t.W, t.tp.Wr, c->logn, t.logql, nullptr, nullptr});
  return GPQ_OK;
}

// src/he-mult.c:67-77 (d != null: c = rdiv(c,P) + d) and src/he-automorphism.c:68-76, for q_l = 2^logql.
// `polys` polynomials of chat; the first `split` of them go to out.a (+ addend d.a), the rest to out.b (+ d.b): c0 and c1 of a
// launch group are one batch (their chat slabs are adjacent in the workspace), half the launches and twice their size.
// chat_prescaled: tail_prescale_mode's answer to the key switch (0: plain limbs; 3 makes `chat` scratch).  rs / rs_done (gpq_he_mul_rs):
// log2(Delta) of the he_rs the tail applies where its streaming kernel runs (1 <= rs <= 63), and whether it did; explicit parameters that reach
// the one-product flow only -- gpq_he_swk and gpq_relin_tail share this function and pass neither
int relin_tail(gpq_ctx *c, Two<uint64_t> out, const uint64_t *chat, Two<const uint64_t> dbig, unsigned W, unsigned dimP, unsigned dimB,
               unsigned logql, unsigned polys, void *ws, hipStream_t s, int chat_prescaled = 0, const TailD *dh = nullptr,
               unsigned rs = 0, bool *rs_done = nullptr) {
  if (rs_done) *rs_done = false;
  TailPlan tp;
  int rc = tail_plan(c, W, dimP, dimB, polys, &tp);
  if (rc) return rc;
  gpq_bridge_basis *bp, *bq;
  gpq_relin_tables *rt;
  if ((rc = get_basis(c, 0, dimP, &bp)) || (rc = get_basis(c, dimP, tp.cnt, &bq)) || (rc = get_relin(c, dimP, dimB, &rt))) return rc;
  if (W > (unsigned)bq->WP + 1) return gpq_fail(GPQ_ERR_UNSUPPORTED, "relin: W=%u words exceed the quotient basis", W);
  Tail t{c, s, bp, bq, rt, tp, TailWs(ws, tp, W, (size_t)polys << c->logn), out, chat, dbig, W, dimP, dimB, logql, polys,
         (dbig.a && dbig.a == out.a) || (dbig.b && dbig.b == out.b)};
  // The flag bytes (c->d_redo) get their final size HERE, before a flow runs: the flow that copies the pointer into argument blocks (the one-product
  // tail) never grows it; the others reach it only through launch_reconstruct, which sizes it before reading it.  A growth after
  // such a copy once left bridge_limb_scale with the outgrown buffer -- stale flags, reads past its end (tools/soak_bridge.py, seed 23).
  const size_t flag_bytes = (size_t)polys << c->logn;
  if (chat_prescaled == 3) {
    bool product = false;
    if ((rc = tail_product_tables(c, dimP, dimB, rt, bp, bq, &product))) return rc;
    if (product && !t.in_place && W <= 14 && logql <= 896) {
      if ((rc = ensure_redo(c, flag_bytes, s)) || (rc = tail_product(t, dh, rs, rs_done))) return rc;
      return launched("relin_tail");
    }
    // The product cannot run (in place, W > 14, logql > 896, no tables; gpq_he_swk called in place): the addend as words, the weights off
    // EVERY coefficient, then the flows below on plain limbs (no rs: the caller rescales)
    if (dh) {
      ReconExtra dx;
      dx.prescaled = true;
      if ((rc = launch_reconstruct(c, dh->bA, dh->scratch, W, dh->hat, dh->dimA, 0, polys, logql, true, nullptr, s, -1, dx))) return rc;
      t.dbig = addend_words(t, dh);
    }
    launch_masked(t, bridge_limb_scale, kNoScope, LimbScaleArgs{c->d_tabs, const_cast<uint64_t *>(chat), rt->d_unscale, nullptr, dimB, c->logn, kNoScope});
    chat_prescaled = 0;
  }
  if (c->set.bridge_mfma && c->logn >= 6 && (rc = get_relin_front(c, dimP, dimB, rt, bp, bq))) return rc;
  if (c->set.bridge_mfma && c->logn >= 6 && rt->d_bfrag) {
    // the front makes Q's (pre-scaled) residues and the round bits from chat; wsc: the limbs above P arrive multiplied by w_j -- the w-scaled tables
    const unsigned gpp = c->n >> 6;
    const bool wsc = chat_prescaled == 2;
    const RelinFrontArgs f{chat, t.w.qhat, (const v4i *)(wsc ? rt->d_bfrag_w : rt->d_bfrag), rt->d_lk, wsc ? rt->d_pk_w : rt->d_pk, wsc ? rt->d_tkp_w : rt->d_tkp, rt->d_kf,
                           t.w.flags, t.w.amb, dimB, dimP, tp.cnt, c->logn, rt->NT, gpp, gpp * polys, nullptr, chat_prescaled ? 1u : 0u, wsc ? 1u : 0u};
    rc = tail_front(t, f, chat_prescaled != 0);
  } else {
    if (chat_prescaled == 2) return gpq_fail(GPQ_ERR_INVALID, "relin_tail: w-scaled limbs need the matrix-core front");
    rc = tail_exact(t, chat_prescaled != 0);
  }
  return rc ? rc : launched("relin_tail");
}

}  // namespace
