// shim_call.hpp -- the staged call: the one protocol every MPI-typed entry point with polynomial operands runs around Operands (shim_polys.hpp),
// the width ladder of the entry points that measure their operands, and the key of he_mul / he_rot / he_conj as such a call sees it.
// Part of the MPI-typed surface: one translation unit (mpi_shim.hip includes these fragments in order).
#pragma once

namespace {

void need_hectx() {
  need_gcrypt();
  if (&hectx == nullptr || !hectx.q) die("`hectx` is not initialised (hectx_init first)");
}

// q_l = 1 (logq a multiple of logDelta, e.g. 850 = 17 x 50): mpi_smod (src/types.c:108-113) takes r = x mod 1 = 0, finds 0 >= floor(1/2) and
// subtracts q -- every coefficient of the reference's result is -1, whatever the operands were.  No device work in that.
void fill_minus_one(poly_mpi_t *p, unsigned n) {
  for (unsigned i = 0; i < n; ++i) { G.mpi_set_ui(p->coeffs[i], 1); G.mpi_neg(p->coeffs[i], p->coeffs[i]); }
}

// One call: `nin` operands and `nout` results of n coefficients at W words, each with its page-locked staging rows and its device slab.
//   prepare   operands with a trusted resident copy are taken from it, the others converted and uploaded (Operands::prepare)
//   queue     work(x, o) -- x[i]: operand i as the device sees it now, o[k]: result k -- then download_issue of the low Wdown words
//   recheck   while the device works the host threads convert and fingerprint the operands taken from their copies (Operands::recheck)
//   queue     again, if an operand had changed or `again` says so
//   deliver   download_convert into the caller's integers with fingerprints, remember_results
// What differs between the entry points is stated below as policy, set between construction and run().  The buffers live across both runs
// of `work`, and the resident slabs the call reads from stay pinned until it ends (~Operands).
struct StagedCall {
  enum Verdict { Done, Misfit /* report_misfits: an operand is wider than W */, Aborted /* *abort was set: nothing was written */ };
  bool speculate = true;         // Operands::prepare's may_speculate
  bool report_misfits = false;   // an operand that outgrew its kept copy ends the program, or (true) ends the call with Misfit: the caller widens
  unsigned Wdown;                // words per coefficient that come down and are remembered, <= W
  // `side`: tasks for the host threads, with the conversions of prepare, or (`side_later`) while the device works: inside the recheck when
  // an operand is resident, on their own behind the first queue otherwise
  unsigned side_parts = 0;
  const std::function<void(unsigned)> *side = nullptr;
  bool side_later = false;
  const std::atomic<bool> *abort = nullptr;   // looked at after prepare and after the recheck
  std::function<bool()> again;                // asked after the recheck: true queues the work once more
  double queued_ms = 0;                       // wall clock behind the first queue (he_mul's timing)
  const unsigned n, W;
  const int nin, nout;

  // in_place: the results are written over the call's own operand slabs (an operand lent from its resident copy is copied there by `work`)
  StagedCall(unsigned n_, unsigned W_, int nin_, const poly_mpi_t *const in[], int nout_, bool in_place = false)
      : Wdown(W_), n(n_), W(W_), nin(nin_), nout(nout_), ops(nin_, in, dd, ss, n_, W_) {
    const size_t bytes = (size_t)W * n * 8;
    for (int i = 0; i < nin; ++i) ss[i] = &host[i].emplace(bytes);
    for (int k = 0; k < nout; ++k) ts[k] = &host[nin + k].emplace(bytes);   // results come back into rows of their own: ss may still be filling (recheck)
    for (int i = 0; i < nin; ++i) dd[i] = &dev[i].emplace(bytes);
    for (int k = 0; k < nout; ++k) {
      oo[k] = in_place ? dd[k] : &dev[nin + k].emplace(bytes);
      o[k] = oo[k]->u64();
    }
  }
  // The copies queued into / out of this call's page-locked buffers must land before the buffers return to the pool: on every way out
  // that is not a delivery, the stream is drained first.  (Page-locked buffers of the caller's own are declared before the call, so
  // that they outlive it.)
  ~StagedCall() { if (in_flight) (void)gpq_stream_sync(nullptr); }
  StagedCall(const StagedCall &) = delete;
  StagedCall &operator=(const StagedCall &) = delete;

  void prepare() {
    in_flight = prepared = true;
    const bool now = side && !side_later;
    ops.prepare(speculate, now ? side_parts : 0, now ? side : nullptr);
  }
  // everything up to the delivery (prepare included, unless the caller ran it)
  template <class Work> Verdict run(Work &&work) {
    if (!prepared) prepare();
    if (abort && abort->load()) return Aborted;
    auto queue = [&]() {
      work(ops.x, o);
      if (nout) download_issue(ts, oo, nout, n, Wdown);       // the low Wdown words of every coefficient (word-major: the first rows)
    };
    queue();
    queued_ms = wall_ms();
    const bool later = side && side_later;
    bool redo = false;
    if (ops.resident) redo = ops.recheck(later ? side_parts : 0, later ? side : nullptr);
    else if (later) { if (side_parts < 2) (*side)(0); else workers().run(side_parts, *side); }
    if (abort && abort->load()) return Aborted;
    if (ops.misfits) {
      if (report_misfits) return Misfit;
      die("coefficient does not fit the big slab");
    }
    if (again && again()) redo = true;
    if (redo) queue();
    return Done;
  }
  void deliver(poly_mpi_t *const out[]) {
    std::vector<uint64_t> prints((size_t)nout * ops.nt, 0);
    download_convert(out, ts, nout, n, Wdown, prints.data());
    in_flight = false;                                        // every range waited for its copy, and the stream is in order
    remember_results(out, oo, nout, n, Wdown, prints);
  }
  template <class Work> Verdict run(Work &&work, poly_mpi_t *const out[]) {
    const Verdict v = run(work);
    if (v == Done) deliver(out);
    return v;
  }
  // a tail of the caller's own instead of deliver()
  int sync() { in_flight = false; return gpq_stream_sync(nullptr); }

 private:
  // arrays: the buffers go back to their pools last taken, first returned, so the next call of the same shape finds every buffer in the
  // role it had (the staging rows a host thread wrote last time are the ones it writes now)
  std::optional<HostBuf> host[6];
  std::optional<DevBuf> dev[6];
  const DevBuf *dd[4], *oo[2];
  const HostBuf *ss[4], *ts[2];
  uint64_t *o[2];
  Operands ops;
  bool in_flight = false, prepared = false;
};

// The evaluation key of he_mul / he_rot / he_conj in a staged call.  A resident copy is used at once and verified while the device works
// (a mismatch -- edited in place since the upload: the reference reads its key on every call -- uploads the key and asks for a second
// run); for any other key the operands do not speculate either, the fingerprint rides with their conversions and settle() uploads it.
struct CallKey {
  KeyPrint kp;
  KeySlot *spec;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  CallKey(const he_evk_t *key, unsigned limbs, unsigned n) : kp(key, limbs, n), spec(resident_key(kp)) {
    if (spec) { k0 = (uint64_t *)spec->d0; k1 = (uint64_t *)spec->d1; }
  }
  CallKey(const CallKey &) = delete;
  CallKey &operator=(const CallKey &) = delete;
  void ride(StagedCall &call) {
    call.speculate = call.side_later = spec != nullptr;
    call.side_parts = kp.parts; call.side = &kp.task;
    call.again = [this] { return changed(); };
  }
  void settle() { if (!spec) key_on_device(kp, &k0, &k1); }   // after prepare
  bool changed() {
    if (!spec || kp.matches(*spec)) return false;
    spec = nullptr;
    key_on_device(kp, &k0, &k1);
    return true;
  }
};

// The width of a call that measures its operands.  If every operand is resident and trusted at one width of at least Wmin (and
// `try_resident`), pass(W, true) runs from the copies at that width; if that is not so, or the pass returns false (an operand has outgrown
// its copy), the integers are measured and pass(W', false) runs at what holds them, `floor_bits` and `headroom` more bits.
template <class Pass>
void width_ladder(const poly_mpi_t *const in[], int count, unsigned n, bool try_resident, unsigned Wmin, unsigned floor_bits, unsigned headroom, Pass &&pass) {
  if (try_resident && poly_cache_on(n)) {
    unsigned W = 0;
    bool all = true;
    for (int i = 0; i < count && all; ++i) {
      const PolySlot *k = resident_poly(in[i], n, 0);
      if (!k || !k->trusted || (W && k->W != W)) all = false; else W = k->W;
    }
    if (all && W >= Wmin && pass(W, true)) return;
  }
  unsigned bits = floor_bits;
  for (int i = 0; i < count; ++i) { const unsigned bi = max_bits(in[i], n); if (bi > bits) bits = bi; }
  pass((bits + headroom) / 64 + 1, false);
}

}  // namespace
