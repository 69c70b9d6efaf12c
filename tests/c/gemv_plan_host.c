/* gemv_plan_host.c -- the plan cache behind he_gemv / he_sum / he_idx (include/gpqhe_hip_compat.h: gpq_shim_gemv_plan_cache) with real libgcrypt
 * MPIs: a repeat call with the same matrix makes NO he_ecd call (the stand-in encoder below counts), every result equals the reference's loop
 * spelled over the library's per-call symbols (words, l, nu, B), and whatever the encoded diagonals depend on misses the cache.
 *
 *   gemv_plan_host check <logn> <logq> <slots> <odd>     odd = 1: q = 2^logq - 1, every call takes the loop
 *   gemv_plan_host plantime <logn> <logq> <slots>        wall time of he_gemv on a new matrix (encodes, makes the plan), on the same matrix
 *                                                        again, and of the loop (conversions and copies included)
 *
 * Setup, encoder and reference loop as in gemv_host.c. */
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
static unsigned long ecd_calls;
void he_ecd(struct he_pt *pt, const _Complex double *m)
{
  ecd_calls++;
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

static int bad;
static he_ct_t got, want;

/* he_gemv(A, x) against the loop; returns the he_ecd calls the library's he_gemv made */
static unsigned long gemv_vs_loop(const _Complex double *A, const he_ct_t *x, const char *what)
{
  const unsigned long before = ecd_calls;
  he_gemv(&got, A, x, rk);
  const unsigned long made = ecd_calls - before;
  ref_gemv(&want, A, x, rk);
  bad |= same(&got, &want, what);
  return made;
}
static void expect(int cond, const char *what, unsigned long calls)
{
  if (cond) printf("ok %s\n", what);
  else { printf("FAIL %s (%lu he_ecd calls)\n", what, calls); bad = 1; }
}

static int check(unsigned slots, int odd)
{
  unsigned n1 = (unsigned)sqrt(slots);
  if (slots != n1 * n1) n1 = (unsigned)sqrt(2 * slots);
  const unsigned long per_call = (unsigned long)n1 * (slots / n1);
  ct_alloc(&got); ct_alloc(&want);
  _Complex double *A = matrix(slots, 5), *S = calloc((size_t)slots * slots, sizeof *S);
  he_ct_t ct2;
  ct_alloc(&ct2);
  he_copy_ct(&ct2, &ct);
  he_neg(&ct2);
  ct2.nu = ct.nu * 1.25; ct2.B = 3.5;
  unsigned long c;
  if (odd) {                                       /* not a power of two: the loop, call after call */
    c = gemv_vs_loop(A, &ct, "odd q first");
    expect(c == per_call, "odd q first call encodes", c);
    c = gemv_vs_loop(A, &ct2, "odd q second");
    expect(c == per_call, "odd q second call encodes", c);
    return bad;
  }
  c = gemv_vs_loop(A, &ct, "first call");
  expect(c == per_call, "first call encodes every diagonal", c);
  c = gemv_vs_loop(A, &ct2, "second call, another ciphertext");
  expect(c == 0, "second call makes no he_ecd call", c);
  A[slots + 1 < slots * slots ? slots + 1 : 0] += 1.0;            /* one entry, in place */
  c = gemv_vs_loop(A, &ct, "matrix changed in place");
  expect(c == per_call, "a changed entry misses", c);
  c = gemv_vs_loop(A, &ct2, "changed matrix again");
  expect(c == 0, "the changed matrix hits next time", c);
  if (ct.l < 2) { printf("FAIL the parameters leave no second level\n"); return 1; }
  he_ct_t low;
  ct_alloc(&low);
  he_copy_ct(&low, &ct);
  he_moddown(&low);
  c = gemv_vs_loop(A, &low, "another level");
  expect(c == per_call, "another ct->l misses", c);
  const double Delta = hectx.Delta;
  hectx.Delta = Delta * 2;                          /* (no longer q_l / q_(l-1): both sides run call by call) */
  c = gemv_vs_loop(A, &ct, "another Delta");
  expect(c == per_call, "another Delta misses", c);
  hectx.Delta = Delta;
  c = gemv_vs_loop(A, &ct, "Delta restored");
  expect(c == 0, "the plan made before is still there", c);
  /* five distinct matrices through four entries: the first is gone, the last is kept */
  gpq_shim_gemv_plan_cache(0);
  gpq_shim_gemv_plan_cache(4);
  _Complex double *M[5];
  for (int t = 0; t < 5; t++) {
    M[t] = matrix(slots, 100 + t);
    c = gemv_vs_loop(M[t], &ct, "distinct matrix");
    expect(c == per_call, "a new matrix encodes", c);
  }
  c = gemv_vs_loop(M[4], &ct2, "fifth matrix again");
  expect(c == 0, "the fifth matrix is kept", c);
  c = gemv_vs_loop(M[0], &ct2, "first matrix again");
  expect(c == per_call, "the first matrix was evicted", c);
  /* he_sum, he_idx: keyed by kind and idx */
  for (unsigned i = 0; i < slots * slots; i++) S[i] = i < slots ? 1 : 0;
  for (int rep = 0; rep < 2; rep++) {
    const unsigned long before = ecd_calls;
    he_sum(&got, rep ? &ct2 : &ct, rk);
    c = ecd_calls - before;
    ref_gemv(&want, S, rep ? &ct2 : &ct, rk);
    bad |= same(&got, &want, rep ? "he_sum again" : "he_sum");
    expect(rep ? c == 0 : c == per_call, rep ? "he_sum again makes no he_ecd call" : "he_sum encodes once", c);
  }
  const unsigned idxs[2] = {0, 5 % slots};
  for (int rep = 0; rep < 2; rep++)
    for (int t = 0; t < 2; t++) {
      if (t && idxs[1] == idxs[0]) continue;
      memset(S, 0, (size_t)slots * slots * sizeof *S);
      S[idxs[t] * slots + idxs[t]] = 1;
      const unsigned long before = ecd_calls;
      he_idx(&got, rep ? &ct2 : &ct, idxs[t], rk);
      c = ecd_calls - before;
      ref_gemv(&want, S, rep ? &ct2 : &ct, rk);
      char name[48];
      snprintf(name, sizeof name, "he_idx %u%s", idxs[t], rep ? " again" : "");
      bad |= same(&got, &want, name);
      expect(rep ? c == 0 : c == per_call, rep ? "he_idx again makes no he_ecd call" : "he_idx encodes once per idx", c);
    }
  /* ct_dest == ct, on a hit */
  he_ct_t x, y;
  ct_alloc(&x); ct_alloc(&y);
  he_copy_ct(&x, &ct); he_copy_ct(&y, &ct);
  he_gemv(&x, M[4], &x, rk);
  ref_gemv(&want, M[4], &y, rk);
  bad |= same(&x, &want, "he_gemv in place");
  /* he_nrm2's sequence, src/he-algo.c:114-127: he_conj, he_mul, he_rs, he_sum(ct, ct) */
  {
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
  /* without the cache: every call encodes, as before */
  gpq_shim_gemv_plan_cache(0);
  c = gemv_vs_loop(M[4], &ct, "cache off first");
  expect(c == per_call, "cache off: first call encodes", c);
  c = gemv_vs_loop(M[4], &ct2, "cache off second");
  expect(c == per_call, "cache off: second call encodes", c);
  gpq_shim_gemv_plan_cache(4);
  return bad;
}

static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }

static int plantime(unsigned slots)
{
  ct_alloc(&got); ct_alloc(&want);
  _Complex double *A = matrix(slots, 5);
  he_gemv(&got, A, &ct, rk);                                /* warm-up: tables, keys, buffers */
  ref_gemv(&want, A, &ct, rk);
  for (int rep = 0; rep < 3; rep++) {
    A = matrix(slots, 200 + rep);
    const double t0 = now_ms();
    he_gemv(&got, A, &ct, rk);
    const double t1 = now_ms();
    he_gemv(&got, A, &ct, rk);
    const double t2 = now_ms();
    ref_gemv(&want, A, &ct, rk);
    const double t3 = now_ms();
    printf("plantime logn %u slots %u: he_gemv first call %.2f ms (ratio %.3f), repeat call %.2f ms (ratio %.3f), reference loop over the library's symbols %.2f ms\n",
           polyctx.logn, slots, t1 - t0, (t1 - t0) / (t3 - t2), t2 - t1, (t2 - t1) / (t3 - t2), t3 - t2);
  }
  return same(&got, &want, "plantime words");
}

int main(int argc, char **argv)
{
  if (argc >= 5 && !strcmp(argv[1], "plantime")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0);
    return plantime(atoi(argv[4]));
  }
  if (argc >= 6 && !strcmp(argv[1], "check")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    return check(atoi(argv[4]), atoi(argv[5]));
  }
  fprintf(stderr, "usage: gemv_plan_host check <logn> <logq> <slots> <odd> | plantime <logn> <logq> <slots>\n");
  return 2;
}
