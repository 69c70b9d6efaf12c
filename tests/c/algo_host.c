/* algo_host.c -- gpq_shim_he_inv / _sqrt / _sigmoid / _log / _exp (include/gpqhe_hip_compat.h) with real libgcrypt MPIs: each result is compared,
 * in every integer, in l and in the bits of nu and B, with the reference's loop (src/he-algo.c:131-458) written over this library's own per-call
 * symbols (he_mul, he_rs, he_mulpt, he_addpt, ...) in the same program.
 *
 *   algo_host check <logn> <logq> <all>   q = 2^logq, Delta = 2^30; all = 0: he_inv and he_sqrt with one iteration, 1: all five
 *   algo_host check_at <logn> <logq> <logDelta> <down> <all>   the same with Delta = 2^logDelta on a source brought `down` levels below the top
 *                                         by this program's own he_moddown (centred mod q_l, l < L), and he_sigmoid once more in place
 *   algo_host refuse <logn> <logq>        the 0 returns: a depth that does not fit, a source that is not centred
 *   algo_host odd <logn> <logq>           ... and q = 2^logq - 1: no modulus on the way is a power of two
 *   algo_host time <logn> <logq> <logDelta> <rounds>   he_inv's call sequence over the per-call symbols against ONE gpq_shim_he_inv, wall time
 * he_ecd is the host program's; here a deterministic stand-in that both sides call on the same vector. */
#include <complex.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "gpqhe_hip.h"
#include "gpqhe_hip_compat.h"
#include "gpqhe_hip_ctx.h"

typedef void *MPI;
MPI gcry_mpi_new(unsigned int nbits);
void gcry_mpi_release(MPI a);
MPI gcry_mpi_set(MPI w, const MPI u);
MPI gcry_mpi_set_ui(MPI w, unsigned long u);
void gcry_mpi_lshift(MPI x, MPI a, unsigned int n);
void gcry_mpi_sub_ui(MPI w, MPI u, unsigned long v);
void gcry_mpi_sub(MPI w, MPI u, MPI v);
void gcry_mpi_neg(MPI w, MPI u);
void gcry_mpi_mod(MPI r, MPI dividend, MPI divisor);
int gcry_mpi_cmp(const MPI u, const MPI v);
unsigned int gcry_mpi_get_nbits(MPI a);
unsigned int gcry_mpi_scan(MPI *ret, int format, const void *buffer, size_t buflen, size_t *nscanned);

static uint64_t splitmix64(uint64_t *s)
{
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

/* key generation draws from these */
static uint64_t err_state = 111, uni_state = 222;
static void set_si(MPI m, long v)
{
  gcry_mpi_set_ui(m, (unsigned long)(v < 0 ? -v : v));
  if (v < 0) gcry_mpi_neg(m, m);
}
void sample_error(poly_mpi_t *r)
{
  for (unsigned i = 0; i < polyctx.n; i++) set_si(r->coeffs[i], (long)(splitmix64(&err_state) % 17) - 8);
}
static void uniform_mod(MPI out, const MPI q, uint64_t *st)
{
  const unsigned nb = (gcry_mpi_get_nbits(q) + 7) / 8 + 8;
  unsigned char buf[1024];
  for (unsigned b = 0; b < nb; b += 8) { const uint64_t v = splitmix64(st); memcpy(buf + b, &v, 8); }
  MPI t = NULL;
  gcry_mpi_scan(&t, 5, buf, nb, NULL);
  gcry_mpi_mod(out, t, q);
  gcry_mpi_release(t);
}
void sample_uniform(poly_mpi_t *r, const MPI q)
{
  for (unsigned i = 0; i < polyctx.n; i++) uniform_mod(r->coeffs[i], q, &uni_state);
}

/* the stand-in encoder: a dense plaintext below Delta in magnitude that depends on the first slot alone (he_exp encodes a constant vector) */
static unsigned ecd_calls;
void he_ecd(struct he_pt *pt, const _Complex double *m)
{
  ecd_calls++;
  pt->nu = hectx.Delta;
  for (unsigned i = 0; i < polyctx.n; i++) {
    const double v = (creal(m[0]) * (double)(1 + i % 5) - cimag(m[0]) * (double)(i % 3)) * hectx.Delta / (double)(2 + i % 7);
    set_si(pt->m.coeffs[i], (i & 1 ? -1 : 1) * lround(v));
  }
}
/* he_const_pt, src/he-encode.c:119-125 */
static void const_pt(he_pt_t *pt, double re)
{
  for (unsigned i = 0; i < polyctx.n; i++) gcry_mpi_set_ui(pt->m.coeffs[i], 0);
  set_si(pt->m.coeffs[0], (long)roundl((long double)re * hectx.Delta));
  pt->nu = hectx.Delta;
}

static void ct_alloc(he_ct_t *ct) { poly_mpi_alloc(&ct->c0); poly_mpi_alloc(&ct->c1); ct->l = 0; ct->nu = ct->B = 0; }
static void ct_set(he_ct_t *d, const he_ct_t *s)
{
  for (unsigned i = 0; i < polyctx.n; i++) { gcry_mpi_set(d->c0.coeffs[i], s->c0.coeffs[i]); gcry_mpi_set(d->c1.coeffs[i], s->c1.coeffs[i]); }
  d->l = s->l; d->nu = s->nu; d->B = s->B;
}
static int same(const he_ct_t *a, const he_ct_t *b, const char *what)
{
  unsigned bad = 0;
  for (unsigned i = 0; i < polyctx.n; i++) bad += gcry_mpi_cmp(a->c0.coeffs[i], b->c0.coeffs[i]) != 0, bad += gcry_mpi_cmp(a->c1.coeffs[i], b->c1.coeffs[i]) != 0;
  if (bad || a->l != b->l || memcmp(&a->nu, &b->nu, 8) || memcmp(&a->B, &b->B, 8)) {
    printf("MISMATCH %s: %u coefficients, l %u/%u, nu %.17g/%.17g, B %.17g/%.17g\n", what, bad, a->l, b->l, a->nu, b->nu, a->B, b->B);
    return 1;
  }
  printf("ok %s\n", what);
  return 0;
}

/* ---- the reference's loops over the library's per-call symbols ---------------------------------------------------------------------- */
#define NTMP 10
static he_ct_t T[NTMP];
static he_pt_t P1;
static const he_evk_t *RLK;
static void mul_rs(he_ct_t *d, const he_ct_t *a, const he_ct_t *b) { he_mul(d, a, b, RLK); he_rs(d); }
static void mulc_rs(he_ct_t *d, const he_ct_t *a, double re) { const_pt(&P1, re); he_mulpt(d, a, &P1); he_rs(d); }
static void addc(he_ct_t *d, const he_ct_t *a, double re) { const_pt(&P1, re); he_addpt(d, a, &P1); }
static void subc(he_ct_t *d, const he_ct_t *a, double re) { const_pt(&P1, re); he_subpt(d, a, &P1); }

static void loop_inv(he_ct_t *out, const he_ct_t *ct, unsigned iter)                 /* src/he-algo.c:131-164 */
{
  he_ct_t *tmp = &T[0], *an = &T[1], *bn = &T[2];
  he_copy_ct(tmp, ct);
  he_neg(tmp);
  addc(an, tmp, 2);
  he_moddown(an);
  addc(bn, tmp, 1);
  for (unsigned i = 0; i < iter; i++) {
    mul_rs(bn, bn, bn);
    addc(tmp, bn, 1);
    mul_rs(an, an, tmp);
  }
  he_copy_ct(out, an);
}
static void loop_sqrt(he_ct_t *out, const he_ct_t *ct, unsigned iter)                /* :166-206 */
{
  he_ct_t *tmp = &T[0], *an = &T[1], *bn = &T[2];
  he_copy_ct(an, ct);
  subc(bn, ct, 1);
  for (unsigned i = 0; i < iter; i++) {
    mulc_rs(tmp, bn, 0.5);
    subc(tmp, tmp, 1);
    he_neg(tmp);
    he_moddown(an);
    mul_rs(an, an, tmp);
    subc(tmp, bn, 3);
    mulc_rs(tmp, tmp, 0.25);
    mul_rs(bn, bn, bn);
    mul_rs(bn, bn, tmp);
  }
  he_copy_ct(out, an);
}
static void loop_sigmoid(he_ct_t *out, const he_ct_t *ct)                            /* :208-277 */
{
  he_ct_t *ct2 = &T[0], *ct4 = &T[1], *ct8 = &T[2], *ct3x = &T[3], *ct13 = &T[4], *ct7x = &T[5], *ct57 = &T[6], *ct9x = &T[7];
  mul_rs(ct2, ct, ct);
  mul_rs(ct4, ct2, ct2);
  mul_rs(ct8, ct4, ct4);
  mulc_rs(ct3x, ct, -1. / 48);
  addc(ct13, ct2, (1. / 4) / (-1. / 48));
  mul_rs(ct13, ct3x, ct13);
  he_moddown(ct13); he_moddown(ct13);
  mulc_rs(ct7x, ct, -17. / 80640);
  addc(ct57, ct2, (1. / 480) / (-17. / 80640));
  mul_rs(ct57, ct7x, ct57);
  mul_rs(ct57, ct4, ct57);
  he_moddown(ct57);
  mulc_rs(ct9x, ct, 31. / 1451520);
  he_moddown(ct9x); he_moddown(ct9x);
  mul_rs(ct9x, ct9x, ct8);
  he_add(out, ct13, ct57);
  he_add(out, out, ct9x);
  addc(out, out, 1. / 2);
}
static void log_half(he_ct_t *acc, const he_ct_t *x, unsigned downs, double k6, double k4, double k2, double k0, double kx)
{
  he_ct_t *ct2 = &T[0], *ct4 = &T[1], *ct8 = &T[2], *tmp = &T[5];
  he_copy_ct(acc, ct8);
  mulc_rs(tmp, ct2, k6);
  mul_rs(tmp, tmp, ct4);
  he_add(acc, acc, tmp);
  mulc_rs(tmp, ct4, k4);
  he_add(acc, acc, tmp);
  mulc_rs(tmp, ct2, k2);
  he_moddown(tmp);
  he_add(acc, acc, tmp);
  addc(acc, acc, k0);
  mulc_rs(tmp, x, kx);
  for (unsigned i = 0; i < downs; i++) he_moddown(tmp);
  mul_rs(acc, tmp, acc);
}
static void loop_log(he_ct_t *out, const he_ct_t *ct)                                /* :279-361 */
{
  he_ct_t *ct2 = &T[0], *ct4 = &T[1], *ct8 = &T[2], *ctodd = &T[3], *cteven = &T[4];
  mul_rs(ct2, ct, ct);
  mul_rs(ct4, ct2, ct2);
  mul_rs(ct8, ct4, ct4);
  log_half(ctodd, ct, 2, 9. / 7., 9. / 5., 9. / 3., 9, 1. / 9.);
  log_half(cteven, ct2, 1, 10. / 8., 10. / 6., 10. / 4., 10. / 2, -1. / 10.);
  he_add(out, ctodd, cteven);
}
static void loop_exp(he_ct_t *out, _Complex double a, const he_ct_t *ct, unsigned iter)   /* :364-458 */
{
  he_ct_t *act = &T[0], *ct2 = &T[1], *ct4 = &T[2], *ct01 = &T[3], *ct23 = &T[4], *ct0123 = &T[5], *ct45 = &T[6], *ct67 = &T[7], *ct4567 = &T[8];
  he_pt_t pt;
  poly_mpi_alloc(&pt.m);
  _Complex double coeff[64];
  a /= (1 << iter);
  for (unsigned i = 0; i < hectx.slots; i++) coeff[i] = a;
  he_ecd(&pt, coeff);
  he_mulpt(act, ct, &pt);
  he_rs(act);
  mul_rs(ct2, act, act);
  mul_rs(ct4, ct2, ct2);
  addc(ct01, act, 1.0);
  mulc_rs(ct01, ct01, 1.0);
  he_moddown(ct01);
  addc(ct23, act, 3.0);
  mulc_rs(ct23, ct23, 1.0 / 6);
  mul_rs(ct23, ct2, ct23);
  he_add(ct0123, ct01, ct23);
  he_moddown(ct0123);
  addc(ct45, act, 5.0);
  mulc_rs(ct45, ct45, 1.0 / 120);
  he_moddown(ct45);
  addc(ct67, act, 7.0);
  mulc_rs(ct67, ct67, 1.0 / 5040);
  mul_rs(ct67, ct2, ct67);
  he_add(ct4567, ct45, ct67);
  mul_rs(ct4567, ct4, ct4567);
  he_add(out, ct0123, ct4567);
  for (unsigned i = 0; i < iter; i++) mul_rs(out, out, out);
  poly_mpi_free(&pt.m);
}

/* ---- the context, a centred ciphertext at the top level, a relinearisation key -------------------------------------------------------- */
static he_evk_t rlk;
static unsigned LOGDELTA = 30;
static void setup(unsigned logn, unsigned logq, int odd, he_ct_t *ct)
{
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  if (odd) gcry_mpi_sub_ui(q, q, 1);
  hectx_init(logn, q, 4, 1ull << LOGDELTA);
  hectx.bnd.Brs = 11.5;
  for (unsigned l = 0; l <= hectx.L; l++) hectx.bnd.Bmult[l] = 100.0 + l;
  ct_alloc(ct);
  ct->l = hectx.L; ct->nu = hectx.Delta * 3.5; ct->B = 17.25;
  MPI qh = gcry_mpi_new(0);
  gcry_mpi_set_ui(qh, 1);
  gcry_mpi_lshift(qh, qh, logq - 1);
  uint64_t s2 = 444;
  for (unsigned i = 0; i < polyctx.n; i++) {                  /* centred uniform mod q_L */
    uniform_mod(ct->c0.coeffs[i], hectx.q[ct->l], &s2);
    uniform_mod(ct->c1.coeffs[i], hectx.q[ct->l], &s2);
    if (gcry_mpi_cmp(ct->c0.coeffs[i], qh) >= 0) gcry_mpi_sub(ct->c0.coeffs[i], ct->c0.coeffs[i], hectx.q[ct->l]);
    if (gcry_mpi_cmp(ct->c1.coeffs[i], qh) >= 0) gcry_mpi_sub(ct->c1.coeffs[i], ct->c1.coeffs[i], hectx.q[ct->l]);
  }
  for (int k = 0; k < NTMP; k++) ct_alloc(&T[k]);
  poly_mpi_alloc(&P1.m);
  poly_mpi_t sk;
  poly_mpi_alloc(&sk);
  uint64_t st = 333;
  for (unsigned i = 0; i < polyctx.n; i++) { const unsigned v = (unsigned)(splitmix64(&st) % 3); set_si(sk.coeffs[i], v == 2 ? -1 : (long)v); }
  rlk.p0.coeffs = calloc((size_t)hectx.dimevk * polyctx.n, 8); rlk.p1.coeffs = calloc((size_t)hectx.dimevk * polyctx.n, 8);
  if (!odd) he_genrlk(&rlk, &sk);                             /* (key generation takes a power of two; at an odd modulus no evaluator gets as far as its key) */
  RLK = &rlk;
}

static void stats(const char *what, const char *when)
{
  uint64_t confirmed = 0, changed = 0;
  gpq_mpi_shim_poly_stats(&confirmed, &changed);
  printf("poly stats %s %s: resident %u confirmed %llu changed %llu\n", what, when, gpq_mpi_shim_resident_polys(), (unsigned long long)confirmed, (unsigned long long)changed);
}

static const char *NAMES[5] = {"he_inv", "he_sqrt", "he_sigmoid", "he_log", "he_exp"};
static const _Complex double EXP_A = 0.75 - 0.25 * I;
static int call(int kind, he_ct_t *dst, const he_ct_t *src, unsigned iter)
{
  switch (kind) {
    case 0: return gpq_shim_he_inv(dst, src, &rlk, iter);
    case 1: return gpq_shim_he_sqrt(dst, src, &rlk, iter);
    case 2: return gpq_shim_he_sigmoid(dst, src, &rlk);
    case 3: return gpq_shim_he_log(dst, src, &rlk);
    default: return gpq_shim_he_exp(dst, EXP_A, src, &rlk, iter);
  }
}
static void loop(int kind, he_ct_t *dst, const he_ct_t *src, unsigned iter)
{
  switch (kind) {
    case 0: loop_inv(dst, src, iter); break;
    case 1: loop_sqrt(dst, src, iter); break;
    case 2: loop_sigmoid(dst, src); break;
    case 3: loop_log(dst, src); break;
    default: loop_exp(dst, EXP_A, src, iter); break;
  }
}

static int run_check(unsigned logn, unsigned logq, unsigned logdelta, unsigned down, int all)
{
  he_ct_t ct, x, y, keep;
  LOGDELTA = logdelta;
  setup(logn, logq, 0, &ct);
  if (down >= hectx.L) { printf("FAIL %u levels down from L = %u\n", down, hectx.L); return 1; }
  for (unsigned d = 0; d < down; d++) he_moddown(&ct);          /* l < L: Bmult[l], q_l and the limb counts are no longer the top's */
  printf("source at l %u of L %u\n", ct.l, hectx.L);
  ct_alloc(&x); ct_alloc(&y); ct_alloc(&keep);
  int bad = 0;
  he_copy_ct(&keep, &ct);                                     /* a first call on ct: where polynomials are kept resident, ct is from here on */
  he_mul(&x, &ct, &ct, &rlk);                                 /* ... and a first product: the key is on the device (a call with a key that is not takes no operand from its copy) */
  for (int kind = 0; kind < (all ? 5 : 2); kind++) {
    unsigned iter = kind == 2 || kind == 3 ? 0 : 1;
    if (kind == 4 && (ct.l < 5 || gcry_mpi_get_nbits(hectx.q[ct.l - 5]) < 2)) iter = 0;   /* he_exp takes 4 + iter levels, and q = 1 is no level */
    char what[64];
    stats(NAMES[kind], "before");
    const unsigned e0 = ecd_calls;
    const int took = call(kind, &x, &ct, iter);
    stats(NAMES[kind], "after");
    printf("%s returned %d, he_ecd calls %u\n", NAMES[kind], took, ecd_calls - e0);
    if (took != 1) { printf("FAIL %s did not run\n", NAMES[kind]); bad = 1; continue; }
    loop(kind, &y, &ct, iter);
    bad |= same(&x, &y, NAMES[kind]);
    snprintf(what, sizeof what, "%s leaves its source", NAMES[kind]);
    bad |= same(&ct, &keep, what);
    if (kind == 0) {                                          /* in place, and a second iteration count */
      ct_set(&x, &ct);
      if (gpq_shim_he_inv(&x, &x, &rlk, 2) != 1) { printf("FAIL he_inv in place did not run\n"); bad = 1; continue; }
      loop_inv(&y, &ct, 2);
      bad |= same(&x, &y, "he_inv in place, two iterations");
    }
    if (kind == 2 && down) {                                  /* in place once more, below the top */
      ct_set(&x, &ct);
      if (gpq_shim_he_sigmoid(&x, &x, &rlk) != 1) { printf("FAIL he_sigmoid in place did not run\n"); bad = 1; continue; }
      bad |= same(&x, &y, "he_sigmoid in place");
    }
  }
  return bad;
}

static int run_refuse(unsigned logn, unsigned logq)
{
  he_ct_t ct, x, keep;
  int bad = 0;
  /* a source that is not centred, and a depth that does not fit, at q = 2^logq */
  setup(logn, logq, 0, &ct);
  ct_alloc(&x); ct_alloc(&keep);
  for (unsigned i = 0; i < polyctx.n; i++) { set_si(x.c0.coeffs[i], 1000 + i); set_si(x.c1.coeffs[i], -7 - (long)i); }
  x.l = 3; x.nu = 5.5; x.B = 6.5;
  ct_set(&keep, &x);
  for (int kind = 0; kind < 5; kind++) {
    char what[96];
    const int r = call(kind, &x, &ct, hectx.L);              /* he_inv: L + 1 levels; he_sqrt: 2 L; he_exp: 4 + L */
    if (kind != 2 && kind != 3) {
      printf("%s with a depth that does not fit returned %d\n", NAMES[kind], r);
      if (r != 0) { printf("FAIL %s ran beyond the chain\n", NAMES[kind]); bad = 1; }
      snprintf(what, sizeof what, "%s beyond the chain leaves dst", NAMES[kind]);
      bad |= same(&x, &keep, what);
    }
  }
  MPI half = gcry_mpi_new(0);
  gcry_mpi_set_ui(half, 1);
  gcry_mpi_lshift(half, half, logq - 1);                      /* q_L / 2: one past the largest centred value */
  gcry_mpi_set(ct.c1.coeffs[polyctx.n / 2 + 3], half);
  for (int kind = 0; kind < 5; kind++) {
    char what[96];
    const int r = call(kind, &x, &ct, kind == 2 || kind == 3 ? 0 : 1);
    printf("%s of a source that is not centred returned %d\n", NAMES[kind], r);
    if (r != 0) { printf("FAIL %s ran on a source that is not centred\n", NAMES[kind]); bad = 1; }
    snprintf(what, sizeof what, "%s of a source that is not centred leaves dst", NAMES[kind]);
    bad |= same(&x, &keep, what);
  }
  return bad;
}

static int run_odd(unsigned logn, unsigned logq)
{
  he_ct_t ct, x, keep;
  int bad = 0;
  setup(logn, logq, 1, &ct);
  ct_alloc(&x); ct_alloc(&keep);
  for (unsigned i = 0; i < polyctx.n; i++) { set_si(x.c0.coeffs[i], 1000 + i); set_si(x.c1.coeffs[i], -7 - (long)i); }
  x.l = 3; x.nu = 5.5; x.B = 6.5;
  ct_set(&keep, &x);
  for (int kind = 0; kind < 5; kind++) {
    char what[96];
    const int r = call(kind, &x, &ct, kind == 2 || kind == 3 ? 0 : 1);
    printf("%s at an odd modulus returned %d\n", NAMES[kind], r);
    if (r != 0) { printf("FAIL %s ran at an odd modulus\n", NAMES[kind]); bad = 1; }
    snprintf(what, sizeof what, "%s at an odd modulus leaves dst", NAMES[kind]);
    bad |= same(&x, &keep, what);
  }
  return bad;
}

/* he_inv's call sequence over the per-call symbols on resident operands against ONE gpq_shim_he_inv, alternating; per side the third pass of
 * every round is timed (the first two warm tables, buffers and resident copies), p50 over the rounds */
static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
static int cmp_double(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }
static int run_time(unsigned logn, unsigned logq, unsigned logdelta, int rounds)
{
  he_ct_t ct, x, y;
  LOGDELTA = logdelta;
  setup(logn, logq, 0, &ct);
  ct_alloc(&x); ct_alloc(&y);
  if (rounds < 1 || rounds > 64) rounds = 7;
  const unsigned iters = hectx.L > 8 ? 8 : hectx.L - 1;
  double tl[64], tc[64];
  for (int r = 0; r < rounds; r++) {
    for (int pass = 0; pass < 3; pass++) { const double t0 = now_ms(); loop_inv(&y, &ct, iters); tl[r] = now_ms() - t0; }
    for (int pass = 0; pass < 3; pass++) {
      const double t0 = now_ms();
      if (gpq_shim_he_inv(&x, &ct, &rlk, iters) != 1) { printf("FAIL gpq_shim_he_inv did not run\n"); return 1; }
      tc[r] = now_ms() - t0;
    }
  }
  const int bad = same(&x, &y, "he_inv");
  qsort(tl, rounds, sizeof *tl, cmp_double);
  qsort(tc, rounds, sizeof *tc, cmp_double);
  printf("time logn %u logq %u Delta 2^%u he_inv %u iterations, %d alternating rounds: per-call sequence p50 %.2f ms (%.2f .. %.2f), gpq_shim_he_inv p50 %.2f ms (%.2f .. %.2f), ratio %.2f\n",
         logn, logq, logdelta, iters, rounds, tl[rounds / 2], tl[0], tl[rounds - 1], tc[rounds / 2], tc[0], tc[rounds - 1], tl[rounds / 2] / tc[rounds / 2]);
  return bad;
}

int main(int argc, char **argv)
{
  if (argc >= 6 && !strcmp(argv[1], "time")) return run_time(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
  if (argc >= 5 && !strcmp(argv[1], "check")) return run_check(atoi(argv[2]), atoi(argv[3]), 30, 0, atoi(argv[4]));
  if (argc >= 7 && !strcmp(argv[1], "check_at")) return run_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
  if (argc >= 4 && !strcmp(argv[1], "refuse")) return run_refuse(atoi(argv[2]), atoi(argv[3]));
  if (argc >= 4 && !strcmp(argv[1], "odd")) return run_odd(atoi(argv[2]), atoi(argv[3]));
  fprintf(stderr, "usage: algo_host check <logn> <logq> <all> | check_at <logn> <logq> <logDelta> <down> <all> | refuse <logn> <logq> | odd <logn> <logq> | time <logn> <logq> <logDelta> <rounds>\n");
  return 2;
}
