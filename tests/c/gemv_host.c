/* gemv_host.c -- he_gemv / he_sum / he_idx (src/he-algo.c:47-113) through the reference's signatures with real libgcrypt MPIs, against the
 * reference's loop spelled here over the library's per-call he_copy_ct / he_rot / he_mulpt / he_add / he_rs.
 *
 *   gemv_host check <logn> <logq> <slots> <odd>   every coefficient, l, and the bits of nu and B equal; odd = 1: q = 2^logq - 1 (the fallback)
 *   gemv_host gemvtime <logn> <logq> <slots>      wall time of he_gemv against the loop (conversions and copies included)
 *
 * he_ecd is the host program's (src/he-encode.c:107-111); here a deterministic stand-in: both sides call it on the same vectors. */
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

static uint64_t err_state = 111, uni_state = 222;
void sample_error(poly_mpi_t *r)
{
  for (unsigned i = 0; i < polyctx.n; i++) {
    const long v = (long)(splitmix64(&err_state) % 17) - 8;
    gcry_mpi_set_ui(r->coeffs[i], (unsigned long)(v < 0 ? -v : v));
    if (v < 0) gcry_mpi_neg(r->coeffs[i], r->coeffs[i]);
  }
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

/* the stand-in encoder: any deterministic function of the slot vector */
void he_ecd(struct he_pt *pt, const _Complex double *m)
{
  pt->nu = hectx.Delta;
  const unsigned s = hectx.slots;
  for (unsigned i = 0; i < polyctx.n; i++) {
    const long v = lround(creal(m[i % s]) * 977.0 + cimag(m[i % s]) * 31.0) * (long)(i % 7 + 1) - (long)(i % 3);
    gcry_mpi_set_ui(pt->m.coeffs[i], (unsigned long)(v < 0 ? -v : v));
    if (v < 0) gcry_mpi_neg(pt->m.coeffs[i], pt->m.coeffs[i]);
  }
}

static void ct_alloc(he_ct_t *ct) { poly_mpi_alloc(&ct->c0); poly_mpi_alloc(&ct->c1); }

/* src/he-algo.c:47-93, call by call, over the library's per-call symbols */
static void ref_gemv(he_ct_t *ct_dest, const _Complex double *A, const he_ct_t *ct, const he_evk_t *rk)
{
  const unsigned slots = hectx.slots;
  unsigned n1 = (unsigned)sqrt(slots);
  if (slots != n1 * n1) n1 = (unsigned)sqrt(2 * slots);
  const unsigned n2 = slots / n1;
  he_pt_t pt;
  poly_mpi_alloc(&pt.m);
  he_ct_t inner, outer, ct_rot;
  ct_alloc(&inner); ct_alloc(&outer); ct_alloc(&ct_rot);
  _Complex double *diag = malloc(slots * sizeof *diag), *rd = malloc(slots * sizeof *rd);
  for (unsigned i = 0; i < n2; i++) {
    const int shift = (int)(i * n1);
    for (unsigned j = 0; j < n1; j++) {
      he_copy_ct(&ct_rot, ct);
      he_rot(&ct_rot, (int)j, rk);
      for (unsigned k = 0; k < slots; k++) diag[k] = A[(k % slots) * slots + (shift + j + k) % slots];   /* zrotdiag, :29-42 */
      for (unsigned k = 0; k < slots; k++) { int r = ((int)k - shift) % (int)slots; if (r < 0) r += (int)slots; rd[k] = diag[r]; }
      he_ecd(&pt, rd);
      he_mulpt(&ct_rot, &ct_rot, &pt);
      if (!j) he_copy_ct(&inner, &ct_rot); else he_add(&inner, &inner, &ct_rot);
    }
    he_rot(&inner, shift, rk);
    if (!i) he_copy_ct(&outer, &inner); else he_add(&outer, &outer, &inner);
  }
  he_copy_ct(ct_dest, &outer);
  he_rs(ct_dest);
  free(diag); free(rd);
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

static he_evk_t *rk, rlk, ck;
static he_ct_t ct;

static void setup(unsigned logn, unsigned logq, unsigned slots, int odd)
{
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  hectx_init(logn, q, slots, 1ull << 30);
  hectx.bnd.Brs = 11.5;
  for (unsigned l = 0; l <= hectx.L; l++) hectx.bnd.Bmult[l] = 100.0 + l;
  poly_mpi_t sk;
  poly_mpi_alloc(&sk);
  uint64_t st = 333;
  for (unsigned i = 0; i < polyctx.n; i++) {
    const unsigned v = (unsigned)(splitmix64(&st) % 3);
    gcry_mpi_set_ui(sk.coeffs[i], v == 2 ? 1 : v);
    if (v == 2) gcry_mpi_neg(sk.coeffs[i], sk.coeffs[i]);
  }
  const size_t words = (size_t)hectx.dimevk * polyctx.n;
  rk = calloc(slots, sizeof *rk);
  for (unsigned k = 0; k < slots; k++) { rk[k].p0.coeffs = malloc(words * 8); rk[k].p1.coeffs = malloc(words * 8); }
  rlk.p0.coeffs = malloc(words * 8); rlk.p1.coeffs = malloc(words * 8);
  ck.p0.coeffs = malloc(words * 8); ck.p1.coeffs = malloc(words * 8);
  he_genrk(rk, &sk);
  he_genrlk(&rlk, &sk);
  he_genck(&ck, &sk);
  if (odd) {            /* the library's key generation takes power-of-two q_L only: the keys above, then the same shapes over q = 2^logq - 1 */
    hectx_exit();
    gcry_mpi_sub_ui(q, q, 1);
    hectx_init(logn, q, slots, 1ull << 30);
    hectx.bnd.Brs = 11.5;
    for (unsigned l = 0; l <= hectx.L; l++) hectx.bnd.Bmult[l] = 100.0 + l;
  }
  ct_alloc(&ct);
  ct.l = hectx.L; ct.nu = hectx.Delta * 3.5; ct.B = 17.25;
  MPI qh = gcry_mpi_new(0);
  gcry_mpi_set_ui(qh, 1);
  gcry_mpi_lshift(qh, qh, logq - 1);
  uint64_t s2 = 444;
  for (unsigned i = 0; i < polyctx.n; i++) {                  /* centred uniform mod q_L */
    uniform_mod(ct.c0.coeffs[i], hectx.q[ct.l], &s2);
    uniform_mod(ct.c1.coeffs[i], hectx.q[ct.l], &s2);
    if (gcry_mpi_cmp(ct.c0.coeffs[i], qh) >= 0) gcry_mpi_sub(ct.c0.coeffs[i], ct.c0.coeffs[i], hectx.q[ct.l]);
    if (gcry_mpi_cmp(ct.c1.coeffs[i], qh) >= 0) gcry_mpi_sub(ct.c1.coeffs[i], ct.c1.coeffs[i], hectx.q[ct.l]);
  }
}

static _Complex double *matrix(unsigned slots, uint64_t seed)
{
  _Complex double *A = malloc((size_t)slots * slots * sizeof *A);
  for (size_t i = 0; i < (size_t)slots * slots; i++) A[i] = (double)(splitmix64(&seed) % 9) - 4.0 + ((double)(splitmix64(&seed) % 5) - 2.0) * I;
  return A;
}

static int check(unsigned slots)
{
  int bad = 0;
  he_ct_t got, want;
  ct_alloc(&got); ct_alloc(&want);
  _Complex double *A = matrix(slots, 5), *S = calloc((size_t)slots * slots, sizeof *S);
  he_gemv(&got, A, &ct, rk);
  ref_gemv(&want, A, &ct, rk);
  bad |= same(&got, &want, "he_gemv");
  for (unsigned i = 0; i < slots; i++) S[i] = 1;
  he_sum(&got, &ct, rk);
  ref_gemv(&want, S, &ct, rk);
  bad |= same(&got, &want, "he_sum");
  const unsigned idxs[3] = {0, 5 % slots, slots - 1};
  for (int t = 0; t < 3; t++) {
    memset(S, 0, (size_t)slots * slots * sizeof *S);
    S[idxs[t] * slots + idxs[t]] = 1;
    he_idx(&got, &ct, idxs[t], rk);
    ref_gemv(&want, S, &ct, rk);
    char name[32];
    snprintf(name, sizeof name, "he_idx %u", idxs[t]);
    bad |= same(&got, &want, name);
  }
  /* ct_dest == ct */
  he_ct_t x, y;
  ct_alloc(&x); ct_alloc(&y);
  he_copy_ct(&x, &ct); he_copy_ct(&y, &ct);
  he_gemv(&x, A, &x, rk);
  ref_gemv(&want, A, &y, rk);
  bad |= same(&x, &want, "he_gemv in place");
  /* he_nrm2's sequence, src/he-algo.c:114-127: he_conj, he_mul, he_rs, he_sum(ct, ct) */
  if (ct.l >= 2) {
    he_ct_t cj, m1, m2;
    ct_alloc(&cj); ct_alloc(&m1); ct_alloc(&m2);
    he_copy_ct(&cj, &ct); he_conj(&cj, &ck);
    he_mul(&m1, &ct, &cj, &rlk); he_rs(&m1);
    he_copy_ct(&m2, &m1);
    for (unsigned i = 0; i < slots * slots; i++) S[i] = i < slots ? 1 : 0;
    he_sum(&m1, &m1, rk);
    ref_gemv(&want, S, &m2, rk);
    bad |= same(&m1, &want, "he_nrm2 sequence");
  }
  return bad;
}

static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }

static int gemvtime(unsigned slots)
{
  he_ct_t got, want;
  ct_alloc(&got); ct_alloc(&want);
  _Complex double *A = matrix(slots, 5);
  he_gemv(&got, A, &ct, rk);                                /* warm-up: tables, keys, buffers */
  ref_gemv(&want, A, &ct, rk);
  for (int rep = 0; rep < 3; rep++) {
    double t0 = now_ms();
    he_gemv(&got, A, &ct, rk);
    double t1 = now_ms();
    ref_gemv(&want, A, &ct, rk);
    double t2 = now_ms();
    printf("gemvtime logn %u slots %u: he_gemv %.2f ms, reference loop over the library's symbols %.2f ms, ratio %.3f\n", polyctx.logn, slots,
           t1 - t0, t2 - t1, (t1 - t0) / (t2 - t1));
  }
  return same(&got, &want, "gemvtime words");
}

int main(int argc, char **argv)
{
  if (argc >= 6 && !strcmp(argv[1], "check")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    return check(atoi(argv[4]));
  }
  if (argc >= 5 && !strcmp(argv[1], "gemvtime")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0);
    return gemvtime(atoi(argv[4]));
  }
  fprintf(stderr, "usage: gemv_host check <logn> <logq> <slots> <odd> | gemvtime <logn> <logq> <slots>\n");
  return 2;
}
