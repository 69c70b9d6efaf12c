// bridge_genswk.hpp -- host fragment of bridge.hip: gpq_he_genswk_batch, `count` switching keys per call.  The reduction modulo
// M = P 2^k splits by CRT into the value mod P (the CRT of the first dimP limbs of the product slab), the value mod 2^k
// (gpq_rns_reconstruct's low-word path) and the recombination kernel genswk_crt_tail (genswk_kernels.hpp): no general Barrett pass,
// no host synchronisation, the secret transformed by the caller once for all keys.
#pragma once
namespace {

Big shl_big(const Big &v, unsigned bits) {
  const unsigned wsh = bits / 64, bsh = bits % 64;
  Big r(v.size() + wsh + 1, 0);
  for (size_t j = 0; j < v.size(); ++j) {
    r[j + wsh] |= v[j] << bsh;
    if (bsh) r[j + wsh + 1] |= v[j] >> (64 - bsh);
  }
  while (r.size() > 1 && r.back() == 0) r.pop_back();
  return r;
}
unsigned bits_big(const Big &v) { return 64 * (unsigned)(v.size() - 1) + (64 - __builtin_clzll(v.back())); }
// a * b mod 2^(64 words)
Big mul_low(const Big &a, const Big &b, size_t words) {
  Big r(words, 0);
  for (size_t i = 0; i < words && i < a.size(); ++i) {
    uint64_t carry = 0;
    for (size_t j = 0; i + j < words; ++j) {
      const u128h t = (u128h)a[i] * (j < b.size() ? b[j] : 0) + r[i + j] + carry;
      r[i + j] = (uint64_t)t; carry = (uint64_t)(t >> 64);
    }
  }
  return r;
}
// v^-1 mod 2^(64 words) for odd v: x <- x (2 - v x) doubles the correct low bits (v itself is right to 3)
Big inv_pow2(const Big &v, size_t words) {
  Big x(words, 0);
  x[0] = v[0];
  for (unsigned bits = 3; bits < 64 * words; bits *= 2) {
    Big t = mul_low(v, x, words);                   // 2 - v x
    uint64_t carry = 1;
    for (size_t j = 0; j < words; ++j) { t[j] = ~t[j] + carry; carry = carry && t[j] == 0; }
    uint64_t c2 = 2;
    for (size_t j = 0; j < words && c2; ++j) { const u128h s = (u128h)t[j] + c2; t[j] = (uint64_t)s; c2 = (uint64_t)(s >> 64); }
    x = mul_low(x, t, words);
  }
  return x;
}

int get_genswk(gpq_ctx *c, unsigned dimP, unsigned logqL, gpq_genswk_tables **out) {
  const auto key = std::make_pair(dimP, logqL);
  auto it = c->cache->genswk.find(key);
  if (it != c->cache->genswk.end()) { *out = &it->second; return GPQ_OK; }
  gpq_bridge_basis *bp;
  int rc = get_basis(c, 0, dimP, &bp);
  if (rc) return rc;
  gpq_genswk_tables t;
  const Big &P = bp->h_P;
  const Big M = shl_big(P, logqL), Mh = shl_big(P, logqL - 1);
  Big P3 = P;
  mul_small(P3, 3);
  const Big M3h = shl_big(P3, logqL - 1);
  t.WPw = (unsigned)P.size(); t.W2 = (logqL + 63) / 64; t.LM = (unsigned)M3h.size(); t.nbits = bits_big(M);
  t.dimmul = (t.nbits + c->logn) / 59 + 1;                      // src/he-kem.c:83
  const Big Pinv = inv_pow2(P, t.W2);
  std::vector<uint64_t> h((size_t)t.WPw + t.W2 + 3 * (size_t)t.LM, 0);
  size_t at = 0;
  const size_t oP = at; put(h, at, P, t.WPw); at += t.WPw;
  const size_t oI = at; put(h, at, Pinv, t.W2); at += t.W2;
  const size_t oM = at; put(h, at, M, t.LM); at += t.LM;
  const size_t oH = at; put(h, at, Mh, t.LM); at += t.LM;
  const size_t o3 = at; put(h, at, M3h, t.LM);
  if ((rc = t.d_const.upload(c, h))) return rc;
  t.P = t.d_const + oP; t.Pinv = t.d_const + oI; t.M = t.d_const + oM; t.Mh = t.d_const + oH; t.M3h = t.d_const + o3;
  *out = &c->cache->genswk.emplace(key, std::move(t)).first->second;
  return GPQ_OK;
}

// what both entry points check about the shape; *t on success
int genswk_batch_plan(gpq_ctx *c, unsigned W, unsigned dimP, unsigned logqL, unsigned dimevk, unsigned count, gpq_genswk_tables **t) {
  const char *who = "gpq_he_genswk_batch";
  int rc = check(c, dimevk, count, who);
  if (rc) return rc;
  if (!logqL) return gpq_fail(GPQ_ERR_INVALID, "%s: q_L must be 2^logqL with logqL > 0", who);
  if (dimP < 1 || dimP > c->nprimes) return gpq_fail(GPQ_ERR_INVALID, "%s: dimP=%u outside 1..%u", who, dimP, c->nprimes);
  if ((rc = get_genswk(c, dimP, logqL, t))) return rc;
  if (W < 1 || 64ull * W <= (*t)->nbits) return gpq_fail(GPQ_ERR_INVALID, "%s: %u words cannot hold the raw sample of %u bits (64 W > bits of P q_L)", who, W, (*t)->nbits);
  if ((*t)->dimmul > c->nprimes) return gpq_fail(GPQ_ERR_INVALID, "%s: the product needs %u limbs, the context has %u", who, (*t)->dimmul, c->nprimes);
  if (W > 32 || (*t)->WPw > (unsigned)GENSWK_MAXP) return gpq_fail(GPQ_ERR_UNSUPPORTED, "%s: W=%u, P of %u words", who, W, (*t)->WPw);
  return GPQ_OK;
}
// words of workspace per key of a launch group: product slab | X mod P | X mod 2^k | p0 | p1 centred
size_t genswk_words_per_key(const gpq_ctx *c, const gpq_genswk_tables *t, unsigned W) {
  return ((size_t)t->dimmul + t->WPw + t->W2 + 2 * (size_t)W) << c->logn;
}

template <bool GATHER>
int launch_genswk_tail(gpq_ctx *c, const GenswkTailArgs &a, unsigned keys, hipStream_t s) {
  ProfScope prof(c, GPQ_K_GENSWK_TAIL, s);
  const size_t per_wave = (size_t)(a.WP + 3 * a.W2 + a.W) * 64 * 8;       // at most (32 + 96 + 32) * 512 = 80 KiB: one workgroup's LDS holds a wave
  unsigned waves = (unsigned)((64 * 1024) / per_wave);
  waves = waves > 4 ? 4 : waves < 1 ? 1 : waves;
  if (c->n < 64 * waves) waves = (c->n + 63) / 64;
  const dim3 grid((c->n + 64 * waves - 1) / (64 * waves), keys), block(64 * waves);
  if (per_wave * waves > 64 * 1024) return gpq_launch_lds<&genswk_crt_tail<GATHER>>(96 * 1024, grid, block, per_wave * waves, s, a);
  hipLaunchKernelGGL(genswk_crt_tail<GATHER>, grid, block, per_wave * waves, s, a);
  return GPQ_OK;
}

}  // namespace

extern "C" unsigned gpq_he_genswk_dimmul(gpq_ctx *c, unsigned dimP, unsigned logqL) {
  gpq_genswk_tables *t;
  if (!c || !logqL || dimP < 1 || dimP > c->nprimes || get_genswk(c, dimP, logqL, &t) != GPQ_OK) return 0;
  return t->dimmul;
}

extern "C" size_t gpq_he_genswk_batch_workspace_bytes(gpq_ctx *c, unsigned W, unsigned dimP, unsigned logqL, unsigned dimevk, unsigned count) {
  gpq_genswk_tables *t;
  if (genswk_batch_plan(c, W, dimP, logqL, dimevk, count, &t) != GPQ_OK) return 0;
  return genswk_words_per_key(c, t, W) * gpq_group_size(c, count) * 8;
}

extern "C" int gpq_he_genswk_batch(gpq_ctx *c, uint64_t *evk0, uint64_t *evk1, const uint64_t *p1, const int8_t *e, const uint64_t *sk_ntt,
                                   const int8_t *sk_small, const uint64_t *galois, const uint64_t *sp, unsigned Wsp, unsigned W, unsigned dimP,
                                   unsigned logqL, unsigned dimevk, unsigned count, void *workspace, void *stream) {
  const char *who = "gpq_he_genswk_batch";
  gpq_genswk_tables *t;
  int rc = genswk_batch_plan(c, W, dimP, logqL, dimevk, count, &t);
  if (rc) return rc;
  if (!evk0 || !evk1 || !p1 || !e || !sk_ntt || !workspace) return gpq_fail(GPQ_ERR_INVALID, "%s: null argument", who);
  if (galois ? !sk_small : (!sp || Wsp < 1)) return gpq_fail(GPQ_ERR_INVALID, "%s: galois needs sk_small; without galois the hidden polynomials sp of Wsp >= 1 words", who);
  const size_t n = c->n;
  std::vector<unsigned> ginv(galois ? count : 0);
  for (unsigned j = 0; j < ginv.size(); ++j) {
    const uint64_t g = galois[j];
    if (!(g & 1)) return gpq_fail(GPQ_ERR_INVALID, "%s: galois[%u] is even", who, j);
    uint64_t x = g;                                             // g^-1 mod 2^64, then mod 2n
    for (int r = 0; r < 5; ++r) x *= 2 - g * x;
    ginv[j] = (unsigned)(x & (2 * n - 1));
  }
  const unsigned group = gpq_group_size(c, count);
  const size_t evk = (size_t)count * dimevk * n * 8, big = (size_t)count * W * n * 8, small = (size_t)count * n, key = (size_t)t->dimmul * n * 8,
               wsb = genswk_words_per_key(c, t, W) * group * 8, hidden = galois ? n : (size_t)count * Wsp * n * 8;
  const void *hid = galois ? (const void *)sk_small : (const void *)sp;
  auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return x < y + nb && y < x + na;
  };
  for (uint64_t *o : {evk0, evk1})
    if (overlap(o, evk, p1, big) || overlap(o, evk, e, small) || overlap(o, evk, sk_ntt, key) || overlap(o, evk, hid, hidden))
      return gpq_fail(GPQ_ERR_INVALID, "%s: an output overlaps an input", who);
  if (overlap(evk0, evk, evk1, evk)) return gpq_fail(GPQ_ERR_INVALID, "%s: the outputs overlap", who);
  if (overlap(workspace, wsb, evk0, evk) || overlap(workspace, wsb, evk1, evk) || overlap(workspace, wsb, p1, big) || overlap(workspace, wsb, e, small) ||
      overlap(workspace, wsb, sk_ntt, key) || overlap(workspace, wsb, hid, hidden))
    return gpq_fail(GPQ_ERR_INVALID, "%s: the workspace overlaps an output or an input", who);
  gpq_bridge_basis *bP, *bM;
  if ((rc = get_basis(c, 0, dimP, &bP)) || (rc = get_basis(c, 0, t->dimmul, &bM))) return rc;
  StageRange stage(who);
  hipStream_t s = (hipStream_t)stream;
  const unsigned dimmul = t->dimmul, WPw = t->WPw, W2 = t->W2;
  for (unsigned k0 = 0; k0 < count; k0 += group) {
    const unsigned keys = count - k0 < group ? count - k0 : group;
    uint64_t *x = (uint64_t *)workspace, *aX = x + (size_t)keys * dimmul * n, *c2 = aX + (size_t)keys * WPw * n, *p0 = c2 + (size_t)keys * W2 * n,
             *p1c = p0 + (size_t)keys * W * n;
    const uint64_t *p1g = p1 + (size_t)k0 * W * n;
    if ((rc = gpq_rns_decompose(c, x, p1g, W, dimmul, keys, stream))) return rc;           // src/poly.c:96-103 with the secret's limbs already transformed
    if ((rc = gpq_ntt(c, x, dimmul, keys, stream))) return rc;
    if ((rc = gpq_rns_mul_shared(c, x, x, sk_ntt, dimmul, keys, s))) return rc;
    if ((rc = gpq_invntt(c, x, dimmul, keys, stream))) return rc;
    if ((rc = launch_reconstruct(c, bP, aX, WPw, x, dimmul, 0, keys, 0, false, nullptr, s))) return rc;        // X mod P in [0, P): exact, P | P'
    if ((rc = launch_reconstruct(c, bM, c2, W2, x, dimmul, 0, keys, logqL, true, nullptr, s))) return rc;      // smod(X, 2^k), X centred mod P'
    GenswkTailArgs a{aX, c2, e + (size_t)k0 * n, p1g, sk_small, galois ? nullptr : sp + (size_t)k0 * Wsp * n, p0, p1c, t->P, t->Pinv, t->M, t->Mh, t->M3h,
                     WPw, W2, W, Wsp, t->LM, c->logn, logqL, {}};
    if (galois) {
      for (unsigned j0 = 0; j0 < keys; j0 += kGenswkKeysPerLaunch) {
        const unsigned cnt = keys - j0 < kGenswkKeysPerLaunch ? keys - j0 : kGenswkKeysPerLaunch;
        GenswkTailArgs b = a;
        b.aX += (size_t)j0 * WPw * n; b.c2 += (size_t)j0 * W2 * n; b.e += (size_t)j0 * n; b.p1 += (size_t)j0 * W * n;
        b.p0 += (size_t)j0 * W * n; b.p1c += (size_t)j0 * W * n;
        for (unsigned j = 0; j < cnt; ++j) b.ginv[j] = ginv[k0 + j0 + j];
        if ((rc = launch_genswk_tail<true>(c, b, cnt, s))) return rc;
      }
    } else if ((rc = launch_genswk_tail<false>(c, a, keys, s))) return rc;
    if ((rc = launched("genswk_crt_tail"))) return rc;
    if ((rc = gpq_evk_pack(c, evk0 + (size_t)k0 * dimevk * n, p0, W, dimevk, keys, stream)) ||
        (rc = gpq_evk_pack(c, evk1 + (size_t)k0 * dimevk * n, p1c, W, dimevk, keys, stream))) return rc;       // :103-110
  }
  return launched(who);
}
