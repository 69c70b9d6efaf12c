// bridge_tables.hpp -- host fragment of bridge.hip: host big integers, and the builders / caches of the constant tables the bridge kernels read
// (CRT constants per basis, the matrix-core matrices, the scaled per-limb tables of the key switch's inverse pass), built on first use.
#pragma once
namespace {

typedef unsigned __int128 u128h;
typedef std::vector<uint64_t> Big;  // little-endian words, unsigned

void mul_small(Big &a, uint64_t m) {
  uint64_t carry = 0;
  for (auto &w : a) { u128h t = (u128h)w * m + carry; w = (uint64_t)t; carry = (uint64_t)(t >> 64); }
  if (carry) a.push_back(carry);
}
uint64_t divmod_small(Big &a, uint64_t m) {  // a <- floor(a/m), returns a mod m
  uint64_t rem = 0;
  for (size_t i = a.size(); i-- > 0;) { u128h t = ((u128h)rem << 64) | a[i]; a[i] = (uint64_t)(t / m); rem = (uint64_t)(t % m); }
  while (a.size() > 1 && a.back() == 0) a.pop_back();
  return rem;
}
uint64_t mod_small(const Big &a, uint64_t m) { Big t = a; return divmod_small(t, m); }
void shr1(Big &a) {
  for (size_t i = 0; i < a.size(); ++i) a[i] = (a[i] >> 1) | (i + 1 < a.size() ? a[i + 1] << 63 : 0);
}
uint64_t powm(uint64_t b, uint64_t e, uint64_t m) {
  uint64_t r = 1;
  while (e) { if (e & 1) r = (uint64_t)((u128h)r * b % m); b = (uint64_t)((u128h)b * b % m); e >>= 1; }
  return r;
}
void put(std::vector<uint64_t> &dst, size_t off, const Big &v, size_t words) {
  for (size_t j = 0; j < words; ++j) dst[off + j] = j < v.size() ? v[j] : 0;
}

const int kWP[] = {8, 16, 32, 48, 56};

// ---- host big integers for the general-modulus path (sizes of a few thousand bits) ----
int cmp_big(const Big &a, const Big &b) {
  size_t na = a.size(), nb = b.size();
  while (na > 1 && a[na - 1] == 0) --na;
  while (nb > 1 && b[nb - 1] == 0) --nb;
  if (na != nb) return na < nb ? -1 : 1;
  for (size_t i = na; i-- > 0;) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
void sub_big(Big &a, const Big &b) {  // a -= b, a >= b
  uint64_t bor = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    const u128h d = (u128h)a[i] - (i < b.size() ? b[i] : 0) - bor;
    a[i] = (uint64_t)d; bor = (uint64_t)(d >> 64) & 1;
  }
}
Big floor_pow2_div(unsigned bits, const Big &m) {  // floor(2^bits / m), restoring division bit by bit
  Big q((bits + 64) / 64, 0), rem(m.size() + 1, 0);
  for (int b = (int)bits; b >= 0; --b) {
    uint64_t c = b == (int)bits ? 1 : 0;           // shift rem left by one, bring in the next dividend bit
    for (size_t i = 0; i < rem.size(); ++i) { const uint64_t n = rem[i] >> 63; rem[i] = (rem[i] << 1) | c; c = n; }
    if (cmp_big(rem, m) >= 0) { sub_big(rem, m); q[b >> 6] |= 1ull << (b & 63); }
  }
  return q;
}

// CRT constants of primes first .. first+dim-1: what struct rns_ctx node dim-1 holds for first = 0
// (src/poly.h:35-38); sub-ranges serve the exact division of he_relin.
int get_basis(gpq_ctx *c, unsigned first, unsigned dim, gpq_bridge_basis **out) {
  const auto key = std::make_pair(first, dim);
  auto it = c->cache->bases.find(key);
  if (it != c->cache->bases.end()) { *out = &it->second; return GPQ_OK; }
  if (dim < 1 || first + dim > c->nprimes || dim > 63)
    return gpq_fail(GPQ_ERR_INVALID, "bridge: limbs %u..%u outside the chain of %u (at most 63 per basis)", first, first + dim, c->nprimes);
  Big P{1};
  for (unsigned d = 0; d < dim; ++d) mul_small(P, c->p[first + d]);  // src/precomp.c:274-277
  int WP = 0;
  for (int w : kWP) if ((size_t)w >= P.size()) { WP = w; break; }
  if (!WP) return gpq_fail(GPQ_ERR_UNSUPPORTED, "bridge: P of %u limbs needs %zu words", dim, P.size());
  gpq_bridge_basis b;
  b.first = first; b.dim = dim; b.WP = WP; b.pbits = 64 * (unsigned)(P.size() - 1) + (64 - __builtin_clzll(P.back()));
  std::vector<uint64_t> phat((size_t)dim * WP), pinv(dim), pmult((size_t)6 * (WP + 1)), phalf(WP + 1);
  for (unsigned d = 0; d < dim; ++d) {
    const uint64_t pd = c->p[first + d];
    Big q = P;
    divmod_small(q, pd);                                             // phat_d = P / p_d   :287
    put(phat, (size_t)d * WP, q, WP);
    pinv[d] = powm(mod_small(q, pd), pd - 2, pd);                    // :288-289
  }
  Big h = P; shr1(h);                                                // P_2 = floor(P/2)   :278
  put(phalf, 0, h, WP + 1);
  Big m = P;
  for (int k = 5; k >= 0; --k) { put(pmult, (size_t)k * (WP + 1), m, WP + 1); mul_small(m, 2); }  // P,2P,..,32P at rows 5..0
  std::vector<uint64_t> inv128(2 * (size_t)dim);
  for (unsigned d = 0; d < dim; ++d) {
    const u128h q = ~(u128h)0 / c->p[first + d];                     // floor(2^128 / p_d): p_d does not divide 2^128
    inv128[2 * d] = (uint64_t)q; inv128[2 * d + 1] = (uint64_t)(q >> 64);
  }
  int rc;
  if ((rc = b.d_phat.upload(c, phat)) || (rc = b.d_phat_inv.upload(c, pinv)) || (rc = b.d_pmult.upload(c, pmult)) ||
      (rc = b.d_phalf.upload(c, phalf)) || (rc = b.d_inv128.upload(c, inv128))) return rc;
  b.h_phat_inv = pinv;
  b.h_P = P;
  b.h_phat = phat;
  *out = &c->cache->bases.emplace(key, std::move(b)).first->second;
  return GPQ_OK;
}

int get_relin(gpq_ctx *c, unsigned dimP, unsigned dimB, gpq_relin_tables **out) {
  const auto key = std::make_pair(dimP, dimB);
  auto it = c->cache->relins.find(key);
  if (it != c->cache->relins.end()) { *out = &it->second; return GPQ_OK; }
  gpq_bridge_basis *bp;
  int rc = get_basis(c, 0, dimP, &bp);
  if (rc) return rc;
  std::vector<uint64_t> pinv(dimB - dimP);
  for (unsigned d = dimP; d < dimB; ++d) pinv[d - dimP] = powm(mod_small(bp->h_P, c->p[d]), c->p[d] - 2, c->p[d]);
  gpq_relin_tables t;
  if ((rc = t.d_pinv.upload(c, pinv))) return rc;
  *out = &c->cache->relins.emplace(key, std::move(t)).first->second;
  return GPQ_OK;
}

// The context's per-limb table with the constants of the LAST inverse stage -- n^-1 and winv[1] n^-1 (src/ntt.c:71-72 folded into the
// stage, ntt_kernels.hpp gs_last) -- multiplied by (P/p_d)^-1 mod p_d for the limbs d of basis b: an inverse transform that reads it
// hands out y_d = ahat_d * phat_invmp_d, the first product of rns_reconstruct (src/rns.c:66-68), for free -- one modular multiply
// and a canonicalisation per (coefficient, limb) less in the CRT kernels that follow (`prescaled`).  Limbs outside the basis keep n^-1.
// The scaled constants are NEW split pairs that gs_last of the wide class reads with multiplicands up to 8p - 1: they pass the same check as
// every other entry of a wide limb (engine.hip: upload_tables).  Returns the first limb below nwide_max whose pair fails, or ~0u.
static unsigned first_unfit_wide_limb(const gpq_ctx *c, const std::vector<LimbTab> &t, unsigned first, unsigned count) {
  for (unsigned d = first; d < first + count && d < c->nwide_max; ++d)
    if (!split_entry_fits_wide(t[d].k.p, t[d].ninv_s.x, t[d].ninv_s.y) || !split_entry_fits_wide(t[d].k.p, t[d].winv1_ninv_s.x, t[d].winv1_ninv_s.y)) return d;
  return ~0u;
}
int get_scaled_tabs(gpq_ctx *c, gpq_bridge_basis *b, const LimbTab **out) {
  if (!b->d_tabs_scaled) {
    std::vector<LimbTab> t = c->cache->h_tabs;
    for (unsigned d = 0; d < b->dim; ++d) {
      LimbTab &e = t[b->first + d];
      const uint64_t p = e.k.p, s = b->h_phat_inv[d];
      e.ninv = (uint64_t)((u128h)e.ninv * s % p);
      e.winv1_ninv = (uint64_t)((u128h)e.winv1_ninv * s % p);
      if (b->first + d < c->nsplit_tables) { e.ninv_s = split_pair_of(e.ninv, p); e.winv1_ninv_s = split_pair_of(e.winv1_ninv, p); }
    }
    const unsigned unfit = first_unfit_wide_limb(c, t, b->first, b->dim);
    if (int rc = b->d_tabs_scaled.upload(c, t)) return rc;
    if (unfit != ~0u) c->cache->scaled_wide_limit[b->d_tabs_scaled] = unfit;
  }
  *out = b->d_tabs_scaled;
  return GPQ_OK;
}
// A context that is about to hand such a table to an inverse pass (gpq_he_mul_tensor_scaled / gpq_keyswitch_scaled / gpq_keyswitch_rotated): a table
// with a pair that does not fit the wide class ends the context's wide range at that limb, FOR GOOD (the calls between which this happens hand
// over canonical residues: any class reads them).  Called where the table is chosen, by the callers of get_scaled_tabs / tail_prescale_mode.
void apply_scaled_wide_limit(gpq_ctx *c, const LimbTab *tabs) {
  if (!tabs || c->cache->scaled_wide_limit.empty()) return;
  const auto it = c->cache->scaled_wide_limit.find(tabs);
  if (it == c->cache->scaled_wide_limit.end()) return;
  if (c->nwide_max > it->second) c->nwide_max = it->second;
  if (c->set.nwide > it->second) c->set.nwide = it->second;
}
inline bool can_prescale(const gpq_ctx *c) { return c->set.prescale && c->logn > 12 && !c->cache->h_tabs.empty(); }   // the two-pass transforms only (small rings: gpq_invntt)

// balanced base-256 digits of a little-endian multiword value, `nd` digits (the final carry is dropped: mod 256^nd)
void balanced_digits(const uint64_t *words, size_t nwords, int8_t *out, size_t nd) {
  unsigned carry = 0;
  for (size_t i = 0; i < nd; ++i) {
    const unsigned byte = i / 8 < nwords ? (unsigned)((words[i / 8] >> (8 * (i % 8))) & 0xff) : 0;
    const unsigned t = byte + carry;
    if (t >= 128) { out[i] = (int8_t)((int)t - 256); carry = 1; } else { out[i] = (int8_t)t; carry = 0; }
  }
}

// Constant matrix, offsets and multiples of `Pw` for bridge_reconstruct_low_mfma<WL>: the contraction sum_d y_d * weight_d mod 2^(64 WL)
// plus the fixed-point columns F = sum_d y_d floor(2^104 / p_d).  For a CRT, weight_d = P/p_d and Pw = P (get_recon_mfma); for the
// one-product relinearisation tail, weight_d = floor(Pi' 2^104 / p_d) and Pw = Pi' 2^104 (get_tail_direct).
int build_recon_mfma(gpq_ctx *c, const std::vector<uint64_t> &primes, const std::vector<uint64_t> &weight_inv, const std::vector<Big> &weight,
                     const Big &Pw, int WL, gpq_recon_mfma *tp, unsigned KSpad = 0, unsigned fcol0 = 0) {
  gpq_recon_mfma &t = *tp;
  const unsigned dim = (unsigned)primes.size(), NT = (8 * WL + 14 + 31) / 32, ncol = 32 * NT;
  t.KS = std::max((dim + 3) / 4, KSpad);                 // (KSpad: zero rows up to the k steps a bridge_stream.hpp instantiation runs)
  if (!fcol0) fcol0 = 8u * WL;                           // first of the 14 fixed-point columns (the addend's rows inside the tail's product: 144)
  t.lds_bytes = (size_t)t.KS * NT * 1024 + (size_t)t.KS * 64;
  if (t.lds_bytes <= 156 * 1024) {
    std::vector<int8_t> bf((size_t)t.KS * NT * 1024, 0);
    std::vector<uint64_t> lk((size_t)t.KS * 8, 0), kc(WL + 2, 0), pm((size_t)65 * WL, 0);
    std::vector<int8_t> beta(8 * (size_t)WL), phi(8);
    Big sum_phat(WL, 0);
    u128h sum_inv = 0;
    for (unsigned d = 0; d < dim; ++d) {
      const uint64_t pd = primes[d];
      lk[2 * (size_t)d] = pd;
      lk[2 * (size_t)d + 1] = weight_inv[d];
      const Big &ph = weight[d];
      balanced_digits(ph.data(), ph.size() < (size_t)WL ? ph.size() : (size_t)WL, beta.data(), beta.size());
      const uint64_t inv = (uint64_t)((((u128h)1) << 104) / pd);                       // < 2^46
      balanced_digits(&inv, 1, phi.data(), 8);
      uint64_t cy = 0;                                                                   // sum_phat += weight_d mod 2^(64 WL)
      for (int j = 0; j < WL; ++j) {
        const u128h s2 = (u128h)sum_phat[j] + ((size_t)j < ph.size() ? ph[j] : 0) + cy;
        sum_phat[j] = (uint64_t)s2; cy = (uint64_t)(s2 >> 64);
      }
      sum_inv += inv;
      for (unsigned i = 0; i < 8; ++i) {
        const unsigned k = 8 * d + i, s = k / 32, h = (k % 32) / 16, tt = k % 16;
        for (unsigned col = 0; col < ncol; ++col) {
          int8_t v = 0;
          if (col < 8u * WL) { if (col >= i) v = beta[col - i]; }
          else if (col >= fcol0) { const unsigned m = col - fcol0; if (m >= i && m - i < 8 && m < 14) v = phi[m - i]; }
          if (!v) continue;
          const unsigned nt = col / 32, lane = 32 * h + col % 32;
          bf[(((size_t)s * NT + nt) * 64 + lane) * 16 + tt] = v;
        }
      }
    }
    // offsets of the signed bytes: 0x8080..80 * sum weight_d (mod 2^(64 WL)) and 0x8080..80 * sum inv_d
    Big kcS = sum_phat;
    mul_small(kcS, 0x8080808080808080ull);
    for (int j = 0; j < WL; ++j) kc[j] = (size_t)j < kcS.size() ? kcS[j] : 0;
    const u128h lo = (u128h)(uint64_t)sum_inv * 0x8080808080808080ull;
    const u128h hi = (u128h)(uint64_t)(sum_inv >> 64) * 0x8080808080808080ull;
    const u128h kf = lo + (hi << 64);
    kc[WL] = (uint64_t)kf; kc[WL + 1] = (uint64_t)(kf >> 64);
    Big mP{0};
    for (unsigned m = 0; m <= 64; ++m) {
      uint64_t bw = 0;                                                                   // (m Pw - Kc) mod 2^(64 WL)
      for (int j = 0; j < WL; ++j) {
        const u128h d2 = (u128h)((size_t)j < mP.size() ? mP[j] : 0) - kc[j] - bw;
        pm[(size_t)m * WL + j] = (uint64_t)d2; bw = (uint64_t)(d2 >> 64) & 1;
      }
      Big nxt(std::max(mP.size(), Pw.size()) + 1, 0);                                    // mP += Pw
      uint64_t cy = 0;
      for (size_t j = 0; j < nxt.size(); ++j) {
        const u128h s2 = (u128h)(j < mP.size() ? mP[j] : 0) + (j < Pw.size() ? Pw[j] : 0) + cy;
        nxt[j] = (uint64_t)s2; cy = (uint64_t)(s2 >> 64);
      }
      mP = nxt;
    }
    int rc;
    if ((rc = t.d_bfrag.upload(c, bf)) || (rc = t.d_lk.upload(c, lk)) || (rc = t.d_kc.upload(c, kc)) || (rc = t.d_pm.upload(c, pm))) { t = gpq_recon_mfma(); return rc; }
  }
  return GPQ_OK;
}

// ... for the CRT over basis b
int get_recon_mfma(gpq_ctx *c, gpq_bridge_basis *b, int WL, gpq_recon_mfma **out, unsigned KSpad = 0) {
  if (KSpad <= (b->dim + 3) / 4) KSpad = 0;
  const int key = WL + 1000 * (int)KSpad;
  auto it = b->mfma.find(key);
  if (it != b->mfma.end()) { *out = &it->second; return GPQ_OK; }
  gpq_recon_mfma t;
  const std::vector<uint64_t> primes(c->p.begin() + b->first, c->p.begin() + b->first + b->dim);
  std::vector<Big> weight(b->dim);
  for (unsigned d = 0; d < b->dim; ++d) {
    weight[d].assign(b->h_phat.begin() + (size_t)d * b->WP, b->h_phat.begin() + (size_t)(d + 1) * b->WP);
  }
  if (int rc = build_recon_mfma(c, primes, b->h_phat_inv, weight, b->h_P, WL, &t, KSpad)) return rc;
  *out = &b->mfma.emplace(key, std::move(t)).first->second;
  return GPQ_OK;
}

// Rows that put poly_rns2mpi(dhat) INSIDE the one-product relinearisation tail (bridge_stream.hpp, DCRT): the CRT over basis b with every
// weight shifted up by the tail's 104 fraction bits -- weight_d = (P/p_d) 2^104, P_w = P 2^104, all modulo 2^1024 -- and the fixed-point
// columns for its own multiple of P at 144 .. 157 (the tail's are 128 .. 141).  Padded to KSpad k steps.
int get_addend_rows(gpq_ctx *c, gpq_bridge_basis *b, unsigned KSpad, gpq_recon_mfma **out) {
  const int key = 100016 + 1000 * (int)KSpad;
  auto it = b->mfma.find(key);
  if (it != b->mfma.end()) { *out = &it->second; return GPQ_OK; }
  auto shifted = [](const Big &v) {                      // v * 2^104
    Big r = v;
    r.insert(r.begin(), 0);
    mul_small(r, 1ull << 40);
    return r;
  };
  const std::vector<uint64_t> primes(c->p.begin() + b->first, c->p.begin() + b->first + b->dim);
  std::vector<Big> weight(b->dim);
  for (unsigned d = 0; d < b->dim; ++d) {
    weight[d] = shifted(Big(b->h_phat.begin() + (size_t)d * b->WP, b->h_phat.begin() + (size_t)(d + 1) * b->WP));
    weight[d].resize(weight[d].size() < 16 ? 16 : weight[d].size(), 0);
  }
  gpq_recon_mfma t;
  if (int rc = build_recon_mfma(c, primes, b->h_phat_inv, weight, shifted(b->h_P), 16, &t, KSpad, 144)) return rc;
  *out = &b->mfma.emplace(key, std::move(t)).first->second;
  return GPQ_OK;
}

// balanced base-256 digits of v < 2^63: v = sum_b d_b 256^b, d_b in [-128, 127] (top digit small and positive)
void balanced8(uint64_t v, int8_t out[8]) {
  const uint64_t t = v + 0x0080808080808080ull;
  for (int b = 0; b < 7; ++b) out[b] = (int8_t)(((t >> (8 * b)) & 0xff) ^ 0x80);
  out[7] = (int8_t)(t >> 56);
}

constexpr size_t kMfmaLdsMax = 96 * 1024;   // of the CU's 160 KB: one workgroup always fits, two when the tables are small

// constant matrix of bridge_decompose_mfma for the primes limb0 .. limb0+dim-1 and W-word inputs
int get_decomp_mfma(gpq_ctx *c, unsigned limb0, unsigned dim, unsigned W, gpq_decomp_mfma **out, unsigned KSforce = 0) {
  const unsigned KSnat = W <= 4 ? 1 : W <= 8 ? 2 : W <= 16 ? 4 : 8;
  if (KSforce <= KSnat) KSforce = 0;
  const auto key = std::make_pair(std::make_pair(limb0, dim), W + 1000 * KSforce);
  auto it = c->cache->decomps.find(key);
  if (it != c->cache->decomps.end()) { *out = &it->second; return GPQ_OK; }
  gpq_decomp_mfma t;
  const unsigned KB = 8 * W;
  t.KS = KSforce ? KSforce : KSnat;                      // (KSforce: zero columns up to the k steps a bridge_stream.hpp instantiation runs)
  t.NT = (dim + 3) / 4;
  t.lds_bytes = (size_t)t.NT * t.KS * 1024 + (size_t)t.NT * 96;
  if (t.lds_bytes <= kMfmaLdsMax) {
    std::vector<int8_t> bf((size_t)t.NT * t.KS * 1024, 0);
    std::vector<uint64_t> pk((size_t)t.NT * 12, 0);
    std::vector<int8_t> dig((size_t)KB * 8);
    for (unsigned j = 0; j < dim; ++j) {
      const uint64_t p = c->p[limb0 + j];
      uint64_t T = 1, K = 0;                               // 256^k mod p ; sum_{k < KB-1} 256^k mod p
      for (unsigned k = 0; k < KB; ++k) {
        balanced8(T, &dig[(size_t)k * 8]);
        if (k + 1 < KB) K = (K + T) % p;
        T = (uint64_t)(((u128h)T << 8) % p);
      }
      K = (uint64_t)(((u128h)K << 7) % p);                 // 128 * sum
      const uint64_t off = 1ull << 50;
      pk[3 * (size_t)j] = p;
      pk[3 * (size_t)j + 1] = off + (K + p - off % p) % p;
      pk[3 * (size_t)j + 2] = p - (1ull << 59);
      const unsigned nt = j / 4, pq = j % 4;
      for (unsigned k = 0; k < KB; ++k) {
        const unsigned s = k / 32, h = (k % 32) / 16, tt = k % 16;
        for (unsigned b = 0; b < 8; ++b) {
          const unsigned lane = 32 * h + 8 * pq + b;       // B[k][col]: lane = (col, h), byte tt
          bf[(((size_t)nt * t.KS + s) * 64 + lane) * 16 + tt] = dig[(size_t)k * 8 + b];
        }
      }
    }
    int rc;
    if ((rc = t.d_bfrag.upload(c, bf)) || (rc = t.d_pk.upload(c, pk))) return rc;
  }
  *out = &c->cache->decomps.emplace(key, std::move(t)).first->second;
  return GPQ_OK;
}

// tables of bridge_relin_front_mfma for P = p_0..p_{dimP-1} and the limbs dimP..dimB-1
int get_relin_front(gpq_ctx *c, unsigned dimP, unsigned dimB, gpq_relin_tables *rt, gpq_bridge_basis *bp, gpq_bridge_basis *bq) {
  if (rt->front_tried) return GPQ_OK;
  rt->front_tried = true;
  const unsigned cnt = dimB - dimP;
  if (dimP < 4 || dimP > 32 || cnt < 4 || bp->pbits < 160) return GPQ_OK;
  const unsigned KS = dimP <= 8 ? 2 : dimP <= 16 ? 4 : 8, NTp = (cnt + 3) / 4, NT = NTp + 1;
  const size_t lds = (size_t)NT * KS * 1024 + (size_t)(8 * KS + 12 * NTp) * 8;
  if (lds > kMfmaLdsMax) return GPQ_OK;
  std::vector<int8_t> bf((size_t)NT * KS * 1024, 0);
  std::vector<uint64_t> lk((size_t)8 * KS, 0), pk((size_t)12 * NTp, 0), tkp((size_t)cnt * 64, 0), kf(2, 0);
  // The same tables with every constant of limb j multiplied by w_j = P^-1 (Pi'/p_j)^-1 mod p_j: with the limbs above P arriving
  // already multiplied by w_j (the key switch's inverse pass reads d_tabs_w) Q's scaled residue is x'_j - (r w_j mod p_j), a
  // subtraction where the plain tables need a modular multiplication per (coefficient, limb).
  std::vector<int8_t> bfw;
  std::vector<uint64_t> pkw((size_t)12 * NTp, 0), tkpw((size_t)cnt * 64, 0), wscale(cnt, 1);
  u128h sum_inv = 0;
  for (unsigned d = 0; d < dimP; ++d) {
    const uint64_t pd = c->p[d];
    lk[2 * (size_t)d] = pd;
    lk[2 * (size_t)d + 1] = bp->h_phat_inv[d];
    const uint64_t inv = (uint64_t)((((u128h)1) << 104) / pd);
    sum_inv += inv;
    int8_t phi[8];
    balanced_digits(&inv, 1, phi, 8);
    for (unsigned i = 0; i < 8; ++i) {
      const unsigned k = 8 * d + i, s = k / 32, h = (k % 32) / 16, tt = k % 16;
      for (unsigned m = i; m < 14 && m - i < 8; ++m)
        bf[(((size_t)(NT - 1) * KS + s) * 64 + 32 * h + m) * 16 + tt] = phi[m - i];
    }
  }
  const u128h kfv = (u128h)(uint64_t)sum_inv * 0x8080808080808080ull;
  kf[0] = (uint64_t)kfv; kf[1] = (uint64_t)(kfv >> 64);
  bfw = bf;                                                                // the F columns (row tile NT-1) are the same
  for (int scaled = 0; scaled < 2; ++scaled) {
    std::vector<int8_t> &B = scaled ? bfw : bf;
    std::vector<uint64_t> &PK = scaled ? pkw : pk, &TK = scaled ? tkpw : tkp;
    for (unsigned j = 0; j < cnt; ++j) {
      const uint64_t pj = c->p[dimP + j];
      const uint64_t Pm0 = mod_small(bp->h_P, pj);
      const uint64_t Pinv = powm(Pm0, pj - 2, pj);
      const uint64_t wj = (uint64_t)((u128h)Pinv * bq->h_phat_inv[j] % pj);
      const uint64_t mulw = scaled ? wj : 1;
      const uint64_t Pm = (uint64_t)((u128h)Pm0 * mulw % pj);
      wscale[j] = wj;
      uint64_t sum_ph = 0;
      const unsigned nt = j / 4, pq = j % 4;
      for (unsigned d = 0; d < dimP; ++d) {
        Big ph(bp->h_phat.begin() + (size_t)d * bp->WP, bp->h_phat.begin() + (size_t)(d + 1) * bp->WP);
        uint64_t T = (uint64_t)((u128h)mod_small(ph, pj) * mulw % pj);   // (P/p_d) [w_j] mod p_j
        sum_ph = (uint64_t)(((u128h)sum_ph + T) % pj);
        for (unsigned i = 0; i < 8; ++i) {
          int8_t dig[8];
          balanced8(T, dig);
          const unsigned k = 8 * d + i, s = k / 32, h = (k % 32) / 16, tt = k % 16;
          for (unsigned b = 0; b < 8; ++b) B[(((size_t)nt * KS + s) * 64 + 32 * h + 8 * pq + b) * 16 + tt] = dig[b];
          T = (uint64_t)(((u128h)T << 8) % pj);
        }
      }
      const uint64_t K = (uint64_t)((u128h)(0x8080808080808080ull % pj) * sum_ph % pj);
      const uint64_t off = 1ull << 50;
      PK[3 * (size_t)j] = pj;
      PK[3 * (size_t)j + 1] = off + (K + pj - off % pj) % pj;
      PK[3 * (size_t)j + 2] = wj;
      for (unsigned k = 0; k < 64; ++k) TK[(size_t)j * 64 + k] = (pj - (uint64_t)((u128h)k * Pm % pj)) % pj;
    }
  }
  // the context's per-limb table for the key switch's inverse pass: (P/p_d)^-1 on the limbs of P, w_j above
  std::vector<LimbTab> tw = c->cache->h_tabs;
  if (!tw.empty()) {
    for (unsigned d = 0; d < dimB; ++d) {
      LimbTab &e = tw[d];
      const uint64_t p = e.k.p, sc = d < dimP ? bp->h_phat_inv[d] : wscale[d - dimP];
      e.ninv = (uint64_t)((u128h)e.ninv * sc % p);
      e.winv1_ninv = (uint64_t)((u128h)e.winv1_ninv * sc % p);
      if (d < c->nsplit_tables) { e.ninv_s = split_pair_of(e.ninv, p); e.winv1_ninv_s = split_pair_of(e.winv1_ninv, p); }
    }
  }
  // (in place: rt is the cache's entry.  d_bfrag and d_tabs_w are what the callers test, so a build that fails half way takes them back:
  // the tables count as absent, what was uploaded stays owned and accounted)
  int rc;
  if ((rc = rt->d_lk.upload(c, lk)) || (rc = rt->d_pk.upload(c, pk)) || (rc = rt->d_tkp.upload(c, tkp)) || (rc = rt->d_kf.upload(c, kf)) ||
      (rc = rt->d_bfrag.upload(c, bf))) { rt->d_bfrag.reset(); return rc; }
  if (!tw.empty()) {
    if ((rc = rt->d_bfrag_w.upload(c, bfw)) || (rc = rt->d_pk_w.upload(c, pkw)) || (rc = rt->d_tkp_w.upload(c, tkpw)) ||
        (rc = rt->d_tabs_w.upload(c, tw))) { rt->d_bfrag.reset(); rt->d_tabs_w.reset(); return rc; }
    const unsigned unfit = first_unfit_wide_limb(c, tw, 0, dimB);
    if (unfit != ~0u) c->cache->scaled_wide_limit[rt->d_tabs_w] = unfit;
  }
  rt->NT = NT; rt->KS = KS; rt->lds_bytes = lds;
  return GPQ_OK;
}

// The one-product tail's matrix over all dimB limbs, zero-padded to KSpad k steps (get_tail_direct): weight_d = floor(Pi' 2^104 / p_d) in at
// least 16 words -- exact for the limbs above P -- with P_w = Pi' 2^104 and the CRT scale (Pi_B/p_d)^-1 mod p_d
int build_tail_direct(gpq_ctx *c, unsigned dimP, unsigned dimB, unsigned KSpad, gpq_recon_mfma *t) {
  gpq_bridge_basis *bB, *bq;
  int rc;
  if ((rc = get_basis(c, 0, dimB, &bB)) || (rc = get_basis(c, dimP, dimB - dimP, &bq))) return rc;
  Big num = bq->h_P;
  num.insert(num.begin(), 0);                               // << 64
  mul_small(num, 1ull << 40);                               // << 40
  const std::vector<uint64_t> primes(c->p.begin(), c->p.begin() + dimB);
  std::vector<Big> weight(dimB, num);
  for (unsigned d = 0; d < dimB; ++d) {
    (void)divmod_small(weight[d], primes[d]);
    weight[d].resize(std::max<size_t>(16, weight[d].size()), 0);
  }
  return build_recon_mfma(c, primes, bB->h_phat_inv, weight, num, 16, t, KSpad);
}

// Tables of the ONE-PRODUCT relinearisation tail (bridge_reconstruct_low_mfma<16> with frac_bits = 104, bridge_mfma.hpp).  With y_d the
// residues scaled for the CRT over ALL dimB limbs (Pi_B = P Pi'), x = sum_d y_d Pi_B/p_d - kappa Pi_B and
//     2^104 x / P = sum_d y_d (Pi' 2^104 / p_d) - kappa Pi' 2^104 :
// exact integers for the limbs above P (p_j divides Pi'), floors for the limbs of P -- an underestimate by less than dimP 2^60 units of
// 2^-104.  The low 104 bits of the 16-word sum are the fraction (x mod P)/P that mpi_rdiv rounds on, the bits above floor(x/P); kappa
// (the multiples of Pi_B the centring of x takes off) comes from the same F columns as in any CRT.  Also: the per-limb table that makes
// the key switch's inverse pass deliver y_d (gpq_keyswitch_scaled), and the weights Pi_B/p_d mod p_d that take the scaling off again
// (bridge_limb_scale) for the few groups the exact kernels re-run.
int get_tail_direct(gpq_ctx *c, unsigned dimP, unsigned dimB, gpq_relin_tables *rt) {
  if (rt->direct_tried) return GPQ_OK;
  rt->direct_tried = true;
  gpq_bridge_basis *bB;
  int rc;
  if (dimB > 60 || dimB - dimP < 4) return GPQ_OK;
  if ((rc = get_basis(c, 0, dimB, &bB)) || c->cache->h_tabs.empty()) return rc;
  if ((rc = build_tail_direct(c, dimP, dimB, 0, &rt->direct)) || !rt->direct.d_bfrag) return rc;
  std::vector<uint64_t> unscale(dimB);
  for (unsigned d = 0; d < dimB; ++d) {
    Big ph(bB->h_phat.begin() + (size_t)d * bB->WP, bB->h_phat.begin() + (size_t)(d + 1) * bB->WP);
    unscale[d] = mod_small(ph, c->p[d]);                    // Pi_B/p_d mod p_d
  }
  const LimbTab *tabs;
  if ((rc = get_scaled_tabs(c, bB, &tabs)) || (rc = rt->d_scale.upload(c, bB->h_phat_inv)) ||   // (Pi_B/p_d)^-1 mod p_d
      (rc = rt->d_unscale.upload(c, unscale))) { rt->direct = gpq_recon_mfma(); return rc; }   // (in place too: no half-built one-product tail)
  rt->d_tabs_direct = tabs;
  return GPQ_OK;
}

// get_tail_direct's matrix zero-padded to KST k steps
int get_tail_direct_padded(gpq_ctx *c, unsigned dimP, unsigned dimB, gpq_relin_tables *rt, unsigned KST, gpq_recon_mfma **out) {
  if (KST <= (dimB + 3) / 4) { *out = &rt->direct; return GPQ_OK; }
  auto it = rt->direct_padded.find(KST);
  if (it != rt->direct_padded.end()) { *out = &it->second; return GPQ_OK; }
  gpq_recon_mfma t;
  if (int rc = build_tail_direct(c, dimP, dimB, KST, &t)) return rc;
  *out = &rt->direct_padded.emplace(KST, std::move(t)).first->second;
  return GPQ_OK;
}

}  // namespace
