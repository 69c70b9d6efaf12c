/* cmp_host.c -- gpq_shim_he_cmp / gpq_shim_he_cmppt (include/gpqhe_hip_compat.h) with real libgcrypt MPIs: each result is compared, in every
 * integer, in l and in the bits of nu and B, with the reference's loop (src/he-algo.c:460-548, he_inv's :131-164 nested) written over this
 * library's own per-call symbols (he_mul, he_rs, he_mulpt, he_add, he_addpt, ...) in the same program.
 *
 *   cmp_host check <logn> <logq> <logDelta> <iter> <alpha> <iterpt> <tpt>
 *                                          q = 2^logq, Delta = 2^logDelta: he_cmp(iter, alpha), once more with dst == ct1 and once with both
 *                                          sources one ciphertext; he_cmppt(iterpt, tpt) by a dense plaintext of about logq bits
 *   cmp_host refuse <logn> <logq> <logDelta>   the 0 returns: unequal levels, alpha 0 and 53, a depth beyond l, a source that is not centred
 *   cmp_host time <logn> <logq> <logDelta> <iter> <t> <rounds>   he_cmppt's call sequence over the per-call symbols on resident operands
 *                                          against ONE gpq_shim_he_cmppt, wall time (he_cmppt: it takes t, so any depth can be timed) */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "gpqhe_hip.h"
#include "gpqhe_hip_algo.h"
#include "gpqhe_hip_compat.h"
#include "gpqhe_hip_ctx.h"

typedef void *MPI;
MPI gcry_mpi_new(unsigned int nbits);
void gcry_mpi_release(MPI a);
MPI gcry_mpi_set(MPI w, const MPI u);
MPI gcry_mpi_set_ui(MPI w, unsigned long u);
void gcry_mpi_lshift(MPI x, MPI a, unsigned int n);
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
/* centred uniform mod q */
static void centred_poly(poly_mpi_t *p, const MPI q, uint64_t *st)
{
  MPI qh = gcry_mpi_new(0);
  gcry_mpi_set_ui(qh, 1);
  gcry_mpi_lshift(qh, qh, gcry_mpi_get_nbits(q) - 2);
  for (unsigned i = 0; i < polyctx.n; i++) {
    uniform_mod(p->coeffs[i], q, st);
    if (gcry_mpi_cmp(p->coeffs[i], qh) >= 0) gcry_mpi_sub(p->coeffs[i], p->coeffs[i], q);
  }
  gcry_mpi_release(qh);
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
#define NTMP 6
static he_ct_t T[NTMP];
static he_pt_t P1;
static he_evk_t rlk;
static void mul_rs(he_ct_t *d, const he_ct_t *a, const he_ct_t *b) { he_mul(d, a, b, &rlk); he_rs(d); }
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
static void loop_cmp_core(he_ct_t *an, const he_ct_t *ct, unsigned iter, unsigned t)  /* :460-507 */
{
  he_ct_t *bn = &T[3], *inv = &T[4];
  he_copy_ct(inv, an);
  mulc_rs(inv, inv, 0.5);
  loop_inv(inv, inv, iter);
  mulc_rs(an, ct, 0.5);
  for (unsigned i = 0; i < iter + 1; i++) he_moddown(an);
  mul_rs(an, an, inv);
  subc(bn, an, 1);
  he_neg(bn);
  for (unsigned r = 0; r < t; r++) {
    mul_rs(an, an, an);
    mul_rs(bn, bn, bn);
    he_add(inv, an, bn);
    loop_inv(inv, inv, iter);
    for (unsigned i = 0; i < iter + 1; i++) he_moddown(an);
    mul_rs(an, an, inv);
    subc(bn, an, 1);
    he_neg(bn);
  }
}
static void loop_cmp(he_ct_t *out, const he_ct_t *ct1, const he_ct_t *ct2, unsigned iter, unsigned t)   /* :514-530, t by gpq_he_cmp_rounds */
{
  he_ct_t *an = &T[5];
  he_add(an, ct1, ct2);
  loop_cmp_core(an, ct1, iter, t);
  he_copy_ct(out, an);
}
static void loop_cmppt(he_ct_t *out, const he_ct_t *ct, const he_pt_t *pt, unsigned iter, unsigned t)   /* :532-548 */
{
  he_ct_t *an = &T[5];
  he_addpt(an, ct, pt);
  loop_cmp_core(an, ct, iter, t);
  he_copy_ct(out, an);
}

/* ---- the context, two centred ciphertexts at the top level, a dense plaintext, a relinearisation key ----------------------------------- */
static he_ct_t CT1, CT2;
static he_pt_t PT;
static void setup(unsigned logn, unsigned logq, unsigned logdelta)
{
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  hectx_init(logn, q, 4, 1ull << logdelta);
  hectx.bnd.Brs = 11.5;
  for (unsigned l = 0; l <= hectx.L; l++) hectx.bnd.Bmult[l] = 100.0 + l;
  uint64_t st = 444;
  ct_alloc(&CT1); ct_alloc(&CT2);
  CT1.l = CT2.l = hectx.L;
  CT1.nu = hectx.Delta * 3.5; CT1.B = 17.25;
  CT2.nu = hectx.Delta * 5.25; CT2.B = 3.125;
  centred_poly(&CT1.c0, hectx.q[hectx.L], &st); centred_poly(&CT1.c1, hectx.q[hectx.L], &st);
  centred_poly(&CT2.c0, hectx.q[hectx.L], &st); centred_poly(&CT2.c1, hectx.q[hectx.L], &st);
  poly_mpi_alloc(&PT.m);
  centred_poly(&PT.m, hectx.q[hectx.L], &st);
  PT.nu = hectx.Delta * 7.0;                                  /* above both sources': pt->nu decides he_addpt's maximum */
  for (int k = 0; k < NTMP; k++) ct_alloc(&T[k]);
  poly_mpi_alloc(&P1.m);
  poly_mpi_t sk;
  poly_mpi_alloc(&sk);
  uint64_t ss = 333;
  for (unsigned i = 0; i < polyctx.n; i++) { const unsigned v = (unsigned)(splitmix64(&ss) % 3); set_si(sk.coeffs[i], v == 2 ? -1 : (long)v); }
  rlk.p0.coeffs = calloc((size_t)hectx.dimevk * polyctx.n, 8); rlk.p1.coeffs = calloc((size_t)hectx.dimevk * polyctx.n, 8);
  he_genrlk(&rlk, &sk);
}

static void stats(const char *what, const char *when)
{
  uint64_t confirmed = 0, changed = 0;
  gpq_mpi_shim_poly_stats(&confirmed, &changed);
  printf("poly stats %s %s: resident %u confirmed %llu changed %llu\n", what, when, gpq_mpi_shim_resident_polys(), (unsigned long long)confirmed, (unsigned long long)changed);
}

static int run_check(unsigned logn, unsigned logq, unsigned logdelta, unsigned iter, unsigned alpha, unsigned iterpt, unsigned tpt)
{
  he_ct_t x, y, keep1, keep2;
  setup(logn, logq, logdelta);
  ct_alloc(&x); ct_alloc(&y); ct_alloc(&keep1); ct_alloc(&keep2);
  int bad = 0;
  const int t = gpq_he_cmp_rounds(alpha);
  printf("L %u, he_cmp iter %u alpha %u: t %d, depth %d; he_cmppt iter %u t %u: depth %d\n", hectx.L, iter, alpha, t, gpq_he_cmp_depth(iter, (unsigned)t), iterpt,
         tpt, gpq_he_cmp_depth(iterpt, tpt));
  if (t < 0) { printf("FAIL alpha %u has no round count\n", alpha); return 1; }
  he_copy_ct(&keep1, &CT1);                                   /* first calls on both: where polynomials are kept resident, they are from here on */
  he_copy_ct(&keep2, &CT2);
  he_mul(&x, &CT1, &CT2, &rlk);                               /* ... and the key is on the device */
  stats("he_cmp", "before");
  int took = gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, iter, alpha);
  stats("he_cmp", "after");
  printf("he_cmp returned %d\n", took);
  if (took != 1) { printf("FAIL he_cmp did not run\n"); bad = 1; }
  else {
    loop_cmp(&y, &CT1, &CT2, iter, (unsigned)t);
    bad |= same(&x, &y, "he_cmp");
    bad |= same(&CT1, &keep1, "he_cmp leaves its first source");
    bad |= same(&CT2, &keep2, "he_cmp leaves its second source");
    ct_set(&x, &CT1);                                         /* dst == ct1 */
    if (gpq_shim_he_cmp(&x, &x, &CT2, &rlk, iter, alpha) != 1) { printf("FAIL he_cmp in place did not run\n"); bad = 1; }
    else bad |= same(&x, &y, "he_cmp with dst == ct1");
    ct_set(&x, &CT2);                                         /* dst == ct2 */
    if (gpq_shim_he_cmp(&x, &CT1, &x, &rlk, iter, alpha) != 1) { printf("FAIL he_cmp onto ct2 did not run\n"); bad = 1; }
    else bad |= same(&x, &y, "he_cmp with dst == ct2");
    if (gpq_shim_he_cmp(&x, &CT1, &CT1, &rlk, iter, alpha) != 1) { printf("FAIL he_cmp of one ciphertext with itself did not run\n"); bad = 1; }
    else { loop_cmp(&y, &CT1, &CT1, iter, (unsigned)t); bad |= same(&x, &y, "he_cmp of one ciphertext with itself"); }
  }
  stats("he_cmppt", "before");
  took = gpq_shim_he_cmppt(&x, &CT1, &PT, &rlk, iterpt, tpt);
  stats("he_cmppt", "after");
  printf("he_cmppt returned %d\n", took);
  if (took != 1) { printf("FAIL he_cmppt did not run\n"); bad = 1; }
  else {
    loop_cmppt(&y, &CT1, &PT, iterpt, tpt);
    bad |= same(&x, &y, "he_cmppt");
    bad |= same(&CT1, &keep1, "he_cmppt leaves its source");
    const_pt(&P1, 1);                                         /* ... and by he_const_pt(1), nu = Delta */
    he_pt_t one;
    poly_mpi_alloc(&one.m);
    for (unsigned i = 0; i < polyctx.n; i++) gcry_mpi_set(one.m.coeffs[i], P1.m.coeffs[i]);
    one.nu = P1.nu;
    if (gpq_shim_he_cmppt(&x, &CT1, &one, &rlk, iterpt, tpt) != 1) { printf("FAIL he_cmppt by a constant did not run\n"); bad = 1; }
    else { loop_cmppt(&y, &CT1, &one, iterpt, tpt); bad |= same(&x, &y, "he_cmppt by he_const_pt(1)"); }
  }
  return bad;
}

static int refused(int r, const he_ct_t *x, const he_ct_t *keep, const char *what)
{
  char line[128];
  printf("%s returned %d\n", what, r);
  if (r != 0) printf("FAIL %s ran\n", what);
  snprintf(line, sizeof line, "%s leaves dst", what);
  return (r != 0) | same(x, keep, line);
}
static int run_refuse(unsigned logn, unsigned logq, unsigned logdelta)
{
  he_ct_t x, keep, low;
  int bad = 0;
  setup(logn, logq, logdelta);
  ct_alloc(&x); ct_alloc(&keep); ct_alloc(&low);
  for (unsigned i = 0; i < polyctx.n; i++) { set_si(x.c0.coeffs[i], 1000 + i); set_si(x.c1.coeffs[i], -7 - (long)i); }
  x.l = 3; x.nu = 5.5; x.B = 6.5;
  ct_set(&keep, &x);
  he_copy_ct(&low, &CT2);
  he_moddown(&low);
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &low, &rlk, 0, 1), &x, &keep, "he_cmp of unequal levels");
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, 0, 0), &x, &keep, "he_cmp with alpha 0");
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, 0, 53), &x, &keep, "he_cmp with alpha 53");
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, hectx.L - 2, 1), &x, &keep, "he_cmp with a depth beyond l");        /* 3 + iter = L + 1 */
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, 0, 8), &x, &keep, "he_cmp with rounds beyond l");                  /* t = 10 */
  bad |= refused(gpq_shim_he_cmppt(&x, &CT1, &PT, &rlk, hectx.L - 2, 0), &x, &keep, "he_cmppt with a depth beyond l");
  bad |= refused(gpq_shim_he_cmppt(&x, &CT1, &PT, &rlk, 0, 0xFFFFFFFFu), &x, &keep, "he_cmppt with a depth that overflows");
  MPI half = gcry_mpi_new(0);
  gcry_mpi_set_ui(half, 1);
  gcry_mpi_lshift(half, half, logq - 1);                      /* q_L / 2: one past the largest centred value */
  MPI was = gcry_mpi_new(0);
  gcry_mpi_set(was, CT2.c1.coeffs[polyctx.n / 2 + 3]);
  gcry_mpi_set(CT2.c1.coeffs[polyctx.n / 2 + 3], half);
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, 0, 1), &x, &keep, "he_cmp of a second source that is not centred");
  gcry_mpi_set(CT2.c1.coeffs[polyctx.n / 2 + 3], was);
  if (gpq_shim_he_cmp(&low, &CT1, &CT2, &rlk, 0, 1) != 1) { printf("FAIL he_cmp did not run once the source was centred again\n"); bad = 1; }
  gcry_mpi_set(CT1.c0.coeffs[5], half);
  bad |= refused(gpq_shim_he_cmp(&x, &CT1, &CT2, &rlk, 0, 1), &x, &keep, "he_cmp of a first source that is not centred");
  bad |= refused(gpq_shim_he_cmppt(&x, &CT1, &PT, &rlk, 0, 0), &x, &keep, "he_cmppt of a source that is not centred");
  return bad;
}

/* he_cmppt's call sequence over the per-call symbols on resident operands against ONE gpq_shim_he_cmppt, alternating; per side the third pass
 * of every round is timed (the first two warm tables, buffers and resident copies), p50 over the rounds */
static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
static int cmp_double(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }
static int run_time(unsigned logn, unsigned logq, unsigned logdelta, unsigned iter, unsigned t, int rounds)
{
  he_ct_t x, y;
  setup(logn, logq, logdelta);
  ct_alloc(&x); ct_alloc(&y);
  if (rounds < 1 || rounds > 64) rounds = 7;
  double tl[64], tc[64];
  for (int r = 0; r < rounds; r++) {
    for (int pass = 0; pass < 3; pass++) { const double t0 = now_ms(); loop_cmppt(&y, &CT1, &PT, iter, t); tl[r] = now_ms() - t0; }
    for (int pass = 0; pass < 3; pass++) {
      const double t0 = now_ms();
      if (gpq_shim_he_cmppt(&x, &CT1, &PT, &rlk, iter, t) != 1) { printf("FAIL gpq_shim_he_cmppt did not run\n"); return 1; }
      tc[r] = now_ms() - t0;
    }
  }
  const int bad = same(&x, &y, "he_cmppt");
  qsort(tl, rounds, sizeof *tl, cmp_double);
  qsort(tc, rounds, sizeof *tc, cmp_double);
  printf("time logn %u logq %u Delta 2^%u he_cmppt iter %u t %u (%d levels), %d alternating rounds: per-call sequence p50 %.2f ms (%.2f .. %.2f), gpq_shim_he_cmppt p50 %.2f ms (%.2f .. %.2f), ratio %.2f\n",
         logn, logq, logdelta, iter, t, gpq_he_cmp_depth(iter, t), rounds, tl[rounds / 2], tl[0], tl[rounds - 1], tc[rounds / 2], tc[0], tc[rounds - 1],
         tl[rounds / 2] / tc[rounds / 2]);
  return bad;
}

int main(int argc, char **argv)
{
  if (argc >= 9 && !strcmp(argv[1], "check"))
    return run_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]));
  if (argc >= 5 && !strcmp(argv[1], "refuse")) return run_refuse(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
  if (argc >= 8 && !strcmp(argv[1], "time")) return run_time(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]));
  fprintf(stderr, "usage: cmp_host check <logn> <logq> <logDelta> <iter> <alpha> <iterpt> <tpt> | refuse <logn> <logq> <logDelta> | time <logn> <logq> <logDelta> <iter> <t> <rounds>\n");
  return 2;
}
