/* constpt_host.c -- he_mulpt / he_addpt / he_subpt by constant plaintexts (a + b x^(n/2), what he_const_pt writes) through the reference's
 * signatures with real libgcrypt MPIs: every step runs with gpq_mpi_shim_set_const_pt(1) and with (0) on twin ciphertexts, and the two must
 * agree in every coefficient, in l and in the bits of nu and B.  The counters of gpq_mpi_shim_const_pt_stats are printed behind every step.
 *
 *   constpt_host check <logn> <logq> <print>   the chain below at q = 2^logq, Delta = 2^30; print = 1: the first product's integers in hex
 *   constpt_host odd <logn> <logq>             q = 2^logq - 1: nothing takes the constant path
 *   constpt_host time <logn> <logq>            wall time of the calls with the switch on and off, operands resident, and of he_inv's call sequence */
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
unsigned int gcry_mpi_print(int format, unsigned char *buffer, size_t buflen, size_t *nwritten, const MPI a);

static uint64_t splitmix64(uint64_t *s)
{
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

/* key generation (time mode only) draws from these */
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

static void ct_alloc(he_ct_t *ct) { poly_mpi_alloc(&ct->c0); poly_mpi_alloc(&ct->c1); }
static void ct_set(he_ct_t *d, const he_ct_t *s)
{
  for (unsigned i = 0; i < polyctx.n; i++) { gcry_mpi_set(d->c0.coeffs[i], s->c0.coeffs[i]); gcry_mpi_set(d->c1.coeffs[i], s->c1.coeffs[i]); }
  d->l = s->l; d->nu = s->nu; d->B = s->B;
}
static void set_si(MPI m, long v)
{
  gcry_mpi_set_ui(m, (unsigned long)(v < 0 ? -v : v));
  if (v < 0) gcry_mpi_neg(m, m);
}
/* the plaintext a + b x^(n/2): every coefficient written */
static void pt_const(he_pt_t *pt, long a, long b)
{
  for (unsigned i = 0; i < polyctx.n; i++) gcry_mpi_set_ui(pt->m.coeffs[i], 0);
  set_si(pt->m.coeffs[0], a);
  set_si(pt->m.coeffs[polyctx.n / 2], b);
  pt->nu = hectx.Delta;
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

static void setup(unsigned logn, unsigned logq, int odd, he_ct_t *ct)
{
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  if (odd) gcry_mpi_sub_ui(q, q, 1);
  hectx_init(logn, q, 4, 1ull << 30);
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
}

static void print_poly(const char *name, const poly_mpi_t *p)
{
  unsigned char buf[1024];
  for (unsigned i = 0; i < polyctx.n; i++) {
    size_t nw = 0;
    if (gcry_mpi_print(4 /* GCRYMPI_FMT_HEX */, buf, sizeof buf, &nw, p->coeffs[i])) { printf("FAIL gcry_mpi_print\n"); exit(1); }
    printf("coeff %s %u %s\n", name, i, (const char *)buf);
  }
}

static int bad;
static unsigned long last_taken, last_fell;
static void counters(const char *step)
{
  unsigned long t = 0, f = 0;
  gpq_mpi_shim_const_pt_stats(&t, &f);
  printf("counters %s: taken %lu fell_back %lu\n", step, t - last_taken, f - last_fell);
  last_taken = t; last_fell = f;
}

static void poly_stats(const char *when)
{
  uint64_t confirmed = 0, changed = 0;
  gpq_mpi_shim_poly_stats(&confirmed, &changed);
  printf("poly stats %s: resident %u confirmed %llu changed %llu\n", when, gpq_mpi_shim_resident_polys(), (unsigned long long)confirmed, (unsigned long long)changed);
}

/* one step on the twins: x with the constant path on, y with it off */
#define STEP(name, onx, ony)                                         \
  do {                                                               \
    gpq_mpi_shim_set_const_pt(1); onx;                               \
    gpq_mpi_shim_set_const_pt(0); ony;                               \
    gpq_mpi_shim_set_const_pt(1);                                    \
    bad |= same(&x, &y, name);                                       \
    counters(name);                                                  \
  } while (0)

static int run_check(unsigned logn, unsigned logq, int odd, int print)
{
  he_ct_t ct, x, y;
  setup(logn, logq, odd, &ct);
  const unsigned n = polyctx.n;
  ct_alloc(&x); ct_alloc(&y);
  ct_set(&x, &ct); ct_set(&y, &ct);
  he_pt_t pt;
  poly_mpi_alloc(&pt.m);
  if (odd) {
    pt_const(&pt, 3l << 28, 0);
    STEP("odd q he_mulpt", he_mulpt(&x, &x, &pt), he_mulpt(&y, &y, &pt));
    STEP("odd q he_addpt", he_addpt(&x, &x, &pt), he_addpt(&y, &y, &pt));
    STEP("odd q he_subpt", he_subpt(&x, &x, &pt), he_subpt(&y, &y, &pt));
    return bad;
  }
  if (hectx.L < 4) { printf("FAIL the parameters leave fewer than four levels\n"); return 1; }
  /* he_mulpt by a real, a negative and a complex constant, each followed by he_rs, on one chain */
  pt_const(&pt, (13l << 28) + 12345, 0);
  if (print) { print_poly("in0", &x.c0); print_poly("in1", &x.c1); printf("constant %ld %ld level %u\n", (13l << 28) + 12345, 0l, x.l); }
  STEP("he_mulpt real", he_mulpt(&x, &x, &pt), he_mulpt(&y, &y, &pt));
  if (print) { print_poly("out0", &x.c0); print_poly("out1", &x.c1); }
  STEP("he_rs real", he_rs(&x), he_rs(&y));
  pt_const(&pt, -((1l << 30) / 48), 0);
  STEP("he_mulpt negative", he_mulpt(&x, &x, &pt), he_mulpt(&y, &y, &pt));
  STEP("he_rs negative", he_rs(&x), he_rs(&y));
  pt_const(&pt, 987654321, -(5l << 27) - 7);
  he_ct_t dx, dy;                                             /* dest != src */
  ct_alloc(&dx); ct_alloc(&dy);
  gpq_mpi_shim_set_const_pt(1); he_mulpt(&dx, &x, &pt);
  gpq_mpi_shim_set_const_pt(0); he_mulpt(&dy, &y, &pt);
  gpq_mpi_shim_set_const_pt(1);
  bad |= same(&dx, &dy, "he_mulpt complex");
  bad |= same(&x, &y, "he_mulpt complex leaves its source");
  counters("he_mulpt complex");
  ct_set(&x, &dx); ct_set(&y, &dy);
  STEP("he_rs complex", he_rs(&x), he_rs(&y));
  /* he_addpt / he_subpt */
  pt_const(&pt, 1l << 30, 0);
  STEP("he_addpt real", he_addpt(&x, &x, &pt), he_addpt(&y, &y, &pt));
  /* one coefficient of c0 edited behind the library's back, the same on both twins: where x is resident the constant path starts from the
   * kept copies, the recheck finds the edit and the one launch runs again (`poly stats` lines around that call) */
  set_si(x.c0.coeffs[n / 3], -12345); set_si(y.c0.coeffs[n / 3], -12345);   /* centred at every level */
  pt_const(&pt, (7l << 27) + 3, -5);
  STEP("he_mulpt const after a host edit", poly_stats("before the edited call"); he_mulpt(&x, &x, &pt); poly_stats("after the edited call"), he_mulpt(&y, &y, &pt));
  pt_const(&pt, -77, (1l << 62) + 5);
  STEP("he_subpt complex", he_subpt(&x, &x, &pt), he_subpt(&y, &y, &pt));
  STEP("he_addpt complex", he_addpt(&dx, &x, &pt), he_addpt(&dy, &y, &pt); ct_set(&x, &dx); ct_set(&y, &dy));
  /* a dense plaintext, and one with a single extra non-zero coefficient at index 1 */
  uint64_t st = 555;
  for (unsigned i = 0; i < n; i++) set_si(pt.m.coeffs[i], (long)(splitmix64(&st) >> 36) - (1l << 27));
  STEP("he_mulpt dense", he_mulpt(&dx, &x, &pt), he_mulpt(&dy, &y, &pt); ct_set(&x, &dx); ct_set(&y, &dy));
  STEP("he_addpt dense", he_addpt(&x, &x, &pt), he_addpt(&y, &y, &pt));
  pt_const(&pt, 12345, -678);
  gcry_mpi_set_ui(pt.m.coeffs[1], 1);
  STEP("he_mulpt nearly sparse", he_mulpt(&dx, &x, &pt), he_mulpt(&dy, &y, &pt); ct_set(&x, &dx); ct_set(&y, &dy));
  STEP("he_subpt nearly sparse", he_subpt(&x, &x, &pt), he_subpt(&y, &y, &pt));
  pt_const(&pt, 12345, -678);
  gcry_mpi_set_ui(pt.m.coeffs[n - 1], 1);
  STEP("he_mulpt nearly sparse at the end", he_mulpt(&dx, &x, &pt), he_mulpt(&dy, &y, &pt); ct_set(&x, &dx); ct_set(&y, &dy));
  /* a coefficient wider than 63 bits at n/2 */
  pt_const(&pt, 5, 0);
  gcry_mpi_set_ui(pt.m.coeffs[n / 2], 1); gcry_mpi_lshift(pt.m.coeffs[n / 2], pt.m.coeffs[n / 2], 63);
  STEP("he_addpt wide constant", he_addpt(&x, &x, &pt), he_addpt(&y, &y, &pt));
  /* a ciphertext with a coefficient that is not centred (q_l / 2, one past the largest centred value), in place */
  MPI half = gcry_mpi_new(0);
  gcry_mpi_set_ui(half, 1);
  gcry_mpi_lshift(half, half, gcry_mpi_get_nbits(hectx.q[x.l]) - 2);
  gcry_mpi_set(x.c1.coeffs[n / 2 + 3], half); gcry_mpi_set(y.c1.coeffs[n / 2 + 3], half);
  pt_const(&pt, 40961, 3);
  STEP("he_mulpt non-centred", he_mulpt(&x, &x, &pt), he_mulpt(&y, &y, &pt));
  STEP("he_mulpt centred again", he_mulpt(&x, &x, &pt), he_mulpt(&y, &y, &pt));
  return bad;
}

static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
static int cmp_double(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }
#define CALLS 31

static int run_time(unsigned logn, unsigned logq)
{
  he_ct_t ct, x, tmp, an, bn;
  setup(logn, logq, 0, &ct);
  ct_alloc(&x); ct_alloc(&tmp); ct_alloc(&an); ct_alloc(&bn);
  he_pt_t pt, one, two;
  poly_mpi_alloc(&pt.m); poly_mpi_alloc(&one.m); poly_mpi_alloc(&two.m);
  pt_const(&pt, (13l << 28) + 12345, -99);
  pt_const(&one, 1l << 30, 0);
  pt_const(&two, 2l << 30, 0);
  double t[CALLS];
  for (int round = 0; round < 4; round++) {                   /* on, off, on, off: the order is not what is measured */
    const int on = !(round & 1);
    gpq_mpi_shim_set_const_pt(on);
    he_copy_ct(&x, &ct);
    he_mulpt(&x, &x, &pt); he_addpt(&x, &x, &pt);             /* warm-up: tables, buffers, resident copies */
    for (int i = 0; i < CALLS; i++) { const double t0 = now_ms(); he_mulpt(&x, &x, &pt); t[i] = now_ms() - t0; }
    qsort(t, CALLS, sizeof *t, cmp_double);
    printf("time logn %u logq %u const_pt %d: he_mulpt by a constant, chained p50 %.3f ms p95 %.3f ms\n", logn, logq, on, t[CALLS / 2], t[CALLS * 95 / 100]);
    for (int i = 0; i < CALLS; i++) { const double t0 = now_ms(); he_addpt(&x, &x, &pt); t[i] = now_ms() - t0; }
    qsort(t, CALLS, sizeof *t, cmp_double);
    printf("time logn %u logq %u const_pt %d: he_addpt by a constant, chained p50 %.3f ms p95 %.3f ms\n", logn, logq, on, t[CALLS / 2], t[CALLS * 95 / 100]);
  }
  /* he_inv's call sequence (src/he-algo.c:130-165) over the library's symbols, as mpi_host hemultime times it */
  poly_mpi_t sk;
  poly_mpi_alloc(&sk);
  uint64_t st = 333;
  for (unsigned i = 0; i < polyctx.n; i++) { const unsigned v = (unsigned)(splitmix64(&st) % 3); set_si(sk.coeffs[i], v == 2 ? -1 : (long)v); }
  he_evk_t rlk;
  rlk.p0.coeffs = malloc((size_t)hectx.dimevk * polyctx.n * 8); rlk.p1.coeffs = malloc((size_t)hectx.dimevk * polyctx.n * 8);
  he_genrlk(&rlk, &sk);
  const int iters = hectx.L > 8 ? 8 : (int)hectx.L - 1;
  for (int round = 0; round < 4; round++) {
    const int on = !(round & 1);
    gpq_mpi_shim_set_const_pt(on);
    double total = 0;
    for (int pass = 0; pass < 3; pass++) {                    /* the last pass is timed */
      const double t0 = now_ms();
      he_copy_ct(&tmp, &ct);
      he_neg(&tmp);
      he_addpt(&an, &tmp, &two);
      he_moddown(&an);
      he_addpt(&bn, &tmp, &one);
      for (int it = 0; it < iters; it++) {
        he_mul(&bn, &bn, &bn, &rlk);
        he_rs(&bn);
        he_addpt(&tmp, &bn, &one);
        he_mul(&an, &an, &tmp, &rlk);
        he_rs(&an);
      }
      total = now_ms() - t0;
    }
    printf("time logn %u logq %u const_pt %d: he_inv's call sequence, %d iterations: %.2f ms\n", logn, logq, on, iters, total);
  }
  gpq_mpi_shim_set_const_pt(1);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 5 && !strcmp(argv[1], "check")) return run_check(atoi(argv[2]), atoi(argv[3]), 0, atoi(argv[4]));
  if (argc >= 4 && !strcmp(argv[1], "odd")) return run_check(atoi(argv[2]), atoi(argv[3]), 1, 0);
  if (argc >= 4 && !strcmp(argv[1], "time")) return run_time(atoi(argv[2]), atoi(argv[3]));
  fprintf(stderr, "usage: constpt_host check <logn> <logq> <print> | odd <logn> <logq> | time <logn> <logq>\n");
  return 2;
}
