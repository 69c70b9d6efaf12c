// bridge_launch.hpp -- host fragment of bridge.hip: one launcher per bridge kernel family.  Each keeps its own block-count policy; kernels
// with raised dynamic LDS go through gpq_launch_lds (engine_internal.hpp); the ladders over instantiated widths are written once each.
#pragma once
namespace {

// grid of a masked kernel of `threads` threads: over the waves of the launch that wrote its mask (FlagScope), or over (n, polys)
inline dim3 masked_grid(const FlagScope &sc, unsigned threads, unsigned n, unsigned polys) {
  if (sc.wave_any) return dim3((sc.waves + threads / 64 - 1) / (threads / 64));
  return dim3((n + threads - 1) / threads, polys);
}

// smallest of the instantiated widths (ascending) that holds `need` words; the last one when none does
inline int width_for(unsigned need, std::initializer_list<int> widths) {
  for (int w : widths) if (need <= (unsigned)w) return w;
  return *(widths.end() - 1);
}
// result widths WL of the low-word CRT kernels (7: q up to 2^448, the reference's default 2^438; 14: q up to 2^896, the headline 2^850) and the
// one switch over them: f(std::integral_constant<int, WL>())
inline int recon_wl(unsigned need) { return width_for(need, {1, 2, 4, 7, 10, 14, 16}); }
template <typename F>
int with_recon_wl(int WL, F f) {
  switch (WL) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 7: return f(std::integral_constant<int, 7>());
    case 10: return f(std::integral_constant<int, 10>());
    case 14: return f(std::integral_constant<int, 14>());
    default: return f(std::integral_constant<int, 16>());
  }
}

template <int WL>
int launch_low_mfma(const ReconMfmaArgs &a, size_t lds, hipStream_t s) {
  unsigned blocks = 256;                                   // one 8-wave workgroup per CU (LDS), persistent over the groups
  if (blocks > (a.total_groups + 7) / 8) blocks = (a.total_groups + 7) / 8;
  return gpq_launch_lds<&bridge_reconstruct_low_mfma<WL>>(156 * 1024, dim3(blocks), dim3(512), lds, s, a);
}

// Options of the relinearisation tail: `only` restricts the exact kernel to flagged coefficients; `prescaled` says the slab
// already holds y_d; `addend`/`rflags` ask the matrix-core fast path to finish the tail itself (then *fused is set and the
// coefficients it handed to the exact kernel -- c->d_redo -- still need bridge_addround).
struct ReconExtra {
  const unsigned char *only = nullptr;
  bool prescaled = false;
  Two<const uint64_t> addend{nullptr, nullptr, ~0u};
  const unsigned char *rflags = nullptr;
  bool *fused = nullptr;
  uint64_t *big_b = nullptr;      // the polynomials from `split` on are written here instead (Two<>, bridge_kernels.hpp)
  unsigned split = ~0u;
  bool exact_only = false;        // skip the fast paths: the exact kernel alone (restricted by `only`)
  FlagScope scope = kNoScope;     // with `only` and exact_only: the bridge_stream.hpp launch that wrote the mask
};

// per-coefficient "redo exactly" flags of the fast CRT paths
int ensure_redo(gpq_ctx *c, size_t flags, hipStream_t s) {
  if (flags <= c->d_redo.bytes) return GPQ_OK;
  return c->d_redo.grow(c, s, flags, false, "the first call at a new batch size allocates scratch: run it once outside stream capture");
}

// arguments of the exact kernel bridge_reconstruct<b->WP> for one call (launch_reconstruct, and the fused fallback kernels behind bridge_stream.hpp)
ReconstructArgs exact_args(const gpq_ctx *c, const gpq_bridge_basis *b, uint64_t *big, unsigned Wout, const uint64_t *slab, unsigned slab_dim,
                           unsigned slab_first, unsigned logq, bool centre, unsigned char *tie, unsigned logn, const ReconExtra &x) {
  return ReconstructArgs{c->d_tabs, slab, Two<uint64_t>{big, x.big_b, x.split}, b->d_phat, b->d_phat_inv, b->d_pmult, b->d_phalf, tie, x.only, b->d_inv128,
                         b->dim, logn, Wout, logq, b->first, slab_dim, slab_first, centre ? 1u : 0u, x.prescaled ? 1u : 0u, x.scope};
}

int launch_reconstruct(gpq_ctx *c, const gpq_bridge_basis *b, uint64_t *big, unsigned Wout, const uint64_t *slab, unsigned slab_dim,
                       unsigned slab_first, unsigned batch, unsigned logq, bool centre, unsigned char *tie, hipStream_t s, int logn_override = -1,
                       const ReconExtra &x = ReconExtra()) {
  const unsigned logn = logn_override < 0 ? c->logn : (unsigned)logn_override, n = 1u << logn;
  const Two<uint64_t> bigs{big, x.big_b, x.split};
  ReconstructArgs a = exact_args(c, b, big, Wout, slab, slab_dim, slab_first, logq, centre, tie, logn, x);
  if (x.fused) *x.fused = false;
  // fast path: centred result modulo a power of two that needs fewer words than P has
  const unsigned need = (logq + 63) / 64;
  // (the centring threshold floor(P/2)/P differs from 1/2 by 1/(2P): negligible against the 2^-61 slack only for large P)
  const bool fast = logq && centre && !c->set.exact_crt && need + 1 < (unsigned)b->WP && need <= 16 && b->pbits >= 160;
  if (fast && !x.exact_only) {
    if (int rc = ensure_redo(c, (size_t)batch << logn, s)) return rc;
    ProfScope prof(c, GPQ_K_RECONSTRUCT, s);
    const int WL = recon_wl(need);
    bool done = false;
    if (c->set.bridge_mfma && logn >= 6 && b->dim >= 4) {      // CRT sum as bytes x constant matrix on the matrix cores
      gpq_recon_mfma *t;
      int rc = get_recon_mfma(c, const_cast<gpq_bridge_basis *>(b), WL, &t);
      if (rc) return rc;
      if (t->d_bfrag) {
        const unsigned gpp = n >> 6;
        ReconMfmaArgs m{slab, bigs, (const v4i *)t->d_bfrag, t->d_lk, t->d_kc, t->d_pm, c->d_redo, tie, b->dim, t->KS, logn, Wout, logq,
                        slab_dim, slab_first, gpp, gpp * batch, x.addend, x.rflags, x.prescaled ? 1u : 0u, 0u, nullptr};
        if (x.fused && x.rflags) *x.fused = true;
        if ((rc = with_recon_wl(WL, [&](auto wl) { return launch_low_mfma<decltype(wl)::value>(m, t->lds_bytes, s); }))) return rc;
        done = true;
      }
    }
    if (!done) with_recon_wl(WL, [&](auto wl) {
      hipLaunchKernelGGL((bridge_reconstruct_low<decltype(wl)::value>), dim3((n + 255) / 256, batch), dim3(256), 0, s, a, (unsigned)b->WP, c->d_redo);
      return (int)GPQ_OK;
    });
    a.only = c->d_redo;   // exact kernel below redoes only the flagged coefficients
    a.scope = kNoScope;   // (the fast kernels above leave no per-wave words)
  }
  ProfScope prof(c, GPQ_K_BRIDGE_EXACT, s);
  const dim3 grid = masked_grid(a.scope, 128, n, batch), block(128);
  switch (b->WP) {
    case 8: hipLaunchKernelGGL((bridge_reconstruct<8>), grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL((bridge_reconstruct<16>), grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL((bridge_reconstruct<32>), grid, block, 0, s, a); break;
    case 48: hipLaunchKernelGGL((bridge_reconstruct<48>), grid, block, 0, s, a); break;
    case 56: hipLaunchKernelGGL((bridge_reconstruct<56>), grid, block, 0, s, a); break;
    default: return gpq_fail(GPQ_ERR_UNSUPPORTED, "reconstruct: WP=%d", b->WP);
  }
  return GPQ_OK;
}

template <int KS>
int launch_decompose_mfma_t(const DecomposeMfmaArgs &a, size_t lds, hipStream_t s) {
  unsigned per_cu = (unsigned)((160 * 1024) / lds);     // workgroups a CU's LDS holds; the registers allow 3
  if (per_cu > 4) per_cu = 4;
  if (per_cu < 1) per_cu = 1;
  unsigned blocks = 256 * per_cu;
  if (blocks > (a.total_groups + 3) / 4) blocks = (a.total_groups + 3) / 4;
  return gpq_launch_lds<&bridge_decompose_mfma<KS>>((int)kMfmaLdsMax, dim3(blocks), dim3(256), lds, s, a);
}
// the integer-VALU rns_decompose: one instantiation per word count
int launch_decompose_valu(const DecomposeArgs &a, unsigned W, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  if (W <= 4) hipLaunchKernelGGL((bridge_decompose<4>), grid, block, 0, s, a);
  else if (W <= 7) hipLaunchKernelGGL((bridge_decompose<7>), grid, block, 0, s, a);
  else if (W <= 14) hipLaunchKernelGGL((bridge_decompose<14>), grid, block, 0, s, a);
  else if (W <= 16) hipLaunchKernelGGL((bridge_decompose<16>), grid, block, 0, s, a);
  else if (W <= 32) hipLaunchKernelGGL((bridge_decompose<32>), grid, block, 0, s, a);
  else return gpq_fail(GPQ_ERR_UNSUPPORTED, "decompose: W=%u words (max 32)", W);
  return GPQ_OK;
}

// `batch` polynomials in all, `big.per` from each source slab in turn, written one after another to `slab`.  lazy: the residues may stay in
// (0, 3p) (matrix-core kernel only; for slabs that go straight into a two-pass forward transform: gpq_he_mul's own decompositions)
int launch_decompose(gpq_ctx *c, uint64_t *slab, const BigSources &big, unsigned W, unsigned limb0, unsigned dim, unsigned batch, hipStream_t s, bool lazy = false) {
  ProfScope prof(c, GPQ_K_DECOMPOSE, s);
  if (c->set.bridge_mfma && c->logn >= 6 && W <= 32 && dim >= 4) {
    gpq_decomp_mfma *t;
    int rc = get_decomp_mfma(c, limb0, dim, W, &t);
    if (rc) return rc;
    if (t->d_bfrag) {
      const unsigned gpp = c->n >> 6;
      DecomposeMfmaArgs m{big, slab, (const v4i *)t->d_bfrag, t->d_pk, W, dim, c->logn, t->NT, gpp, gpp * batch, lazy ? 1u : 0u};
      switch (t->KS) {
        case 1: return launch_decompose_mfma_t<1>(m, t->lds_bytes, s);
        case 2: return launch_decompose_mfma_t<2>(m, t->lds_bytes, s);
        case 4: return launch_decompose_mfma_t<4>(m, t->lds_bytes, s);
        default: return launch_decompose_mfma_t<8>(m, t->lds_bytes, s);
      }
    }
  }
  return launch_decompose_valu(DecomposeArgs{c->d_tabs, big, slab, W, dim, c->logn, limb0}, W, dim3((c->n + 255) / 256, batch), s);
}
int launch_decompose(gpq_ctx *c, uint64_t *slab, const uint64_t *big, unsigned W, unsigned limb0, unsigned dim, unsigned batch, hipStream_t s, bool lazy = false) {
  return launch_decompose(c, slab, one_source(big), W, limb0, dim, batch, s, lazy);
}

// rns_decompose of the coefficients marked in `only` alone (integer-VALU kernel; the exact fallback behind bridge_crt_decompose)
int launch_decompose_masked(gpq_ctx *c, uint64_t *slab, const uint64_t *big, unsigned W, unsigned limb0, unsigned dim, unsigned batch,
                            const unsigned char *only, const FlagScope &scope, hipStream_t s) {
  ProfScope prof(c, GPQ_K_BRIDGE_EXACT, s);
  return launch_decompose_valu(DecomposeArgs{c->d_tabs, one_source(big), slab, W, dim, c->logn, limb0, only, scope}, W, masked_grid(scope, 256, c->n, batch), s);
}

// ---- bridge_stream.hpp: launchers ----
constexpr unsigned kStreamBlocks = 256, kStreamWaves = 8;          // one 8-wave workgroup per CU, persistent over the groups
constexpr size_t kStreamLdsMax = 156 * 1024;

int ensure_wave_any(gpq_ctx *c, hipStream_t s) {
  if (c->d_wave_any) return GPQ_OK;
  // (zeroed on the launch stream: tests/test_stream_bridge_gpu.py, a fresh peer lane)
  return c->d_wave_any.grow(c, s, kStreamBlocks * kStreamWaves * sizeof(unsigned), true, "the first call allocates scratch: run it once outside stream capture");
}
inline unsigned stream_blocks(unsigned total_groups) {
  const unsigned need = (total_groups + kStreamWaves - 1) / kStreamWaves;
  return need < kStreamBlocks ? need : kStreamBlocks;
}
inline bool stream_fast_ok(const gpq_ctx *c, const gpq_bridge_basis *b, unsigned logq) {   // launch_reconstruct's conditions for the fast CRT path
  const unsigned need = (logq + 63) / 64;
  return logq && !c->set.exact_crt && c->set.bridge_mfma && c->logn >= 6 && b->dim >= 4 && need + 1 < (unsigned)b->WP && b->pbits >= 160;
}

template <int WL, int KS, int KSD, int R>
int launch_crt_decompose_t(const CrtDecomposeArgs &a, size_t lds, unsigned blocks, hipStream_t s) {
  return gpq_launch_lds<&bridge_crt_decompose<WL, KS, KSD, R>>((int)kStreamLdsMax, dim3(blocks), dim3(512), lds, s, a);
}

// src/he-mult.c:140 + :59 -- poly_rns2mpi(d2hat) mod 2^logq and rns_decompose of it over dimB limbs in one kernel; `scratch` = W words per
// coefficient for the coefficients the exact kernels redo.  *done = false: shape or settings outside the instantiations (caller runs the two kernels).
int crt_decompose_stream(gpq_ctx *c, gpq_bridge_basis *bA, uint64_t *out, const uint64_t *slab, uint64_t *scratch, unsigned W, unsigned dimA,
                         unsigned dimB, unsigned logq, unsigned polys, hipStream_t s, bool *done) {
  *done = false;
  const unsigned need = (logq + 63) / 64;
  if (!c->set.stream_bridge || !stream_fast_ok(c, bA, logq) || W < need || dimB < 4) return GPQ_OK;
  int WL, KS, KSD;
  if (W <= 7 && dimA <= 16) { WL = 7; KS = 4; KSD = 2; }
  else if (W <= 14 && dimA <= 32) { WL = 14; KS = 8; KSD = 4; }
  else return GPQ_OK;
  gpq_recon_mfma *tr;
  gpq_decomp_mfma *td;
  int rc;
  if ((rc = get_recon_mfma(c, bA, WL, &tr, KS)) || (rc = get_decomp_mfma(c, 0, dimB, W, &td, KSD))) return rc;
  if (!tr->d_bfrag || !td->d_bfrag || tr->KS != (unsigned)KS || td->KS != (unsigned)KSD) return GPQ_OK;
  const unsigned NT = (8 * WL + 14 + 31) / 32;
  const size_t lds = (size_t)KS * NT * 1024 + (size_t)td->NT * KSD * 1024 + (size_t)65 * WL * 8;
  if (lds > kStreamLdsMax) return GPQ_OK;
  if ((rc = ensure_redo(c, (size_t)polys << c->logn, s)) || (rc = ensure_wave_any(c, s))) return rc;
  const unsigned groups = (c->n >> 6) * polys, blocks = stream_blocks(groups);
  const size_t slab_bytes = ((size_t)polys * dimA << c->logn) * 8;
  if (slab_bytes >= 0xfffff000ull) return GPQ_OK;
  CrtDecomposeArgs a{slab, slab_bytes, out, (const v4i *)tr->d_bfrag, tr->d_kc, tr->d_pm, (const v4i *)td->d_bfrag, td->d_pk, c->d_redo, c->d_wave_any,
                     dimA, dimB, td->NT, c->logn, logq, W, groups, dimB, c->set.debug_force_redo, (c->set.lazy_decompose && c->logn > 12) ? 1u : 0u};
  {
    ProfScope prof(c, GPQ_K_CRT_DECOMPOSE, s);
    if (WL == 7) rc = launch_crt_decompose_t<7, 4, 2, 4>(a, lds, blocks, s);
    else rc = launch_crt_decompose_t<14, 8, 4, 4>(a, lds, blocks, s);
    if (rc) return rc;
  }
  // the coefficients in the CRT's window: exact CRT into the scratch words, integer-VALU decompose of those
  const FlagScope scope{c->d_wave_any, blocks * kStreamWaves, groups};
  ReconExtra ex;
  ex.prescaled = true; ex.exact_only = true; ex.only = c->d_redo; ex.scope = scope;
  const bool f32 = bA->WP == 32 && W > 7 && W <= 14, f16 = bA->WP == 16 && W <= 7;
  if (f32 || f16) {                                        // one launch: a thread decomposes the words it has just reconstructed
    ProfScope prof(c, GPQ_K_BRIDGE_EXACT, s);
    const ReconstructArgs ra = exact_args(c, bA, scratch, W, slab, dimA, 0, logq, true, nullptr, c->logn, ex);
    const DecomposeArgs da{c->d_tabs, one_source(scratch), out, W, dimB, c->logn, 0, c->d_redo, scope};
    const dim3 grid = masked_grid(scope, 128, c->n, polys);
    if (f32) hipLaunchKernelGGL((bridge_fallback_crt_decompose<32, 14>), grid, dim3(128), 0, s, ra, da);
    else hipLaunchKernelGGL((bridge_fallback_crt_decompose<16, 7>), grid, dim3(128), 0, s, ra, da);
  } else {
    if ((rc = launch_reconstruct(c, bA, scratch, W, slab, dimA, 0, polys, logq, true, nullptr, s, -1, ex))) return rc;
    if ((rc = launch_decompose_masked(c, out, scratch, W, 0, dimB, polys, c->d_redo, scope, s))) return rc;
  }
  *done = true;
  return GPQ_OK;
}

template <int KS>
int launch_relin_front_t(const RelinFrontArgs &a, size_t lds, hipStream_t s) {
  unsigned per_cu = (unsigned)((160 * 1024) / lds);
  if (per_cu > 3) per_cu = 3;
  if (per_cu < 1) per_cu = 1;
  unsigned blocks = 256 * per_cu;
  if (blocks > (a.total_groups + 3) / 4) blocks = (a.total_groups + 3) / 4;
  if (a.scope.wave_any) blocks = (a.scope.waves + 3) / 4;     // wave w of this launch = wave w of the launch that wrote the mask
  return gpq_launch_lds<&bridge_relin_front_mfma<KS>>((int)kMfmaLdsMax, dim3(blocks), dim3(256), lds, s, a);
}
int launch_relin_front(const gpq_ctx *c, unsigned KS, const RelinFrontArgs &f, size_t lds, hipStream_t s) {
  ProfScope prof(c, f.only ? GPQ_K_BRIDGE_EXACT : GPQ_K_RELIN_FRONT, s);
  switch (KS) {
    case 2: return launch_relin_front_t<2>(f, lds, s);
    case 4: return launch_relin_front_t<4>(f, lds, s);
    default: return launch_relin_front_t<8>(f, lds, s);
  }
}

template <int KST, int KSD, bool DCRT, int R>
int launch_tail_stream_t(const TailStreamArgs &a, size_t lds, unsigned blocks, hipStream_t s) {
  return gpq_launch_lds<&bridge_tail_stream<KST, KSD, DCRT, R>>((int)kStreamLdsMax, dim3(blocks), dim3(512), lds, s, a);
}

int check(const gpq_ctx *c, unsigned dim, unsigned batch, const char *who) {
  if (!c) return gpq_fail(GPQ_ERR_INVALID, "%s: null context", who);
  if (dim < 1 || dim > c->nprimes) return gpq_fail(GPQ_ERR_INVALID, "%s: dim=%u outside 1..%u", who, dim, c->nprimes);
  if (batch < 1) return gpq_fail(GPQ_ERR_INVALID, "%s: empty batch", who);
  // kernels launch on the calling thread's current device: it must be the one the context (its tables, the caller's slabs) lives on
  int dev = -1;
  if (hipGetDevice(&dev) == hipSuccess && dev != c->device)
    return gpq_fail(GPQ_ERR_INVALID, "%s: the context lives on device %d but the calling thread's current device is %d (gpq_set_device(gpq_ctx_device(ctx)) first)", who, c->device, dev);
  return GPQ_OK;
}
// [a, a + na) and [b, b + nb) share a word
bool ranges_overlap(const uint64_t *a, size_t na, const uint64_t *b, size_t nb) { return a < b + nb && b < a + na; }
int launched(const char *who) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GPQ_OK : gpq_fail(GPQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

}  // namespace
