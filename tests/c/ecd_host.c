/* ecd_host.c -- gpq_mpi_shim_set_device_ecd (include/gpqhe_hip_compat.h) with real libgcrypt MPIs: he_gemv / he_sum / he_idx on a matrix
 * they hold no plan for, once with the host program's he_ecd encoding the diagonals (switch 0, the default) and once with the device
 * encoding them from the matrix (switch 1).  Both must give the same coefficients, l and bits of nu and B; with the switch on he_ecd is
 * not called at all, with it off once per diagonal; and a matrix with a coefficient beyond 2^63 falls back to he_ecd without an error.
 *
 *   ecd_host check <logn> <logq> <slots>
 *   ecd_host firstcall <logn> <logq> <slots> <on>     tools/ecd_first_call_ab.py's worker: sets the switch (where the library has one: the
 *                                                     symbol is weak here, so the program also runs on a build without it), warms up, prints
 *                                                     "ready" and then serves one line per command on stdin -- `first`: he_gemv on a NEW matrix
 *                                                     with every plan dropped first; `repeat`: the same matrix again; `quit`
 *
 * he_ecd below is the encoder of src/he-encode.c:53-64 / src/canemb.c:62-81 stated in plain C for this test: it reads polyctx.ring
 * (cyc_group, zetas) like the reference and must be compiled without fused multiply-add (-ffp-contract=off).  Setup as gemv_plan_host.c. */
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

#pragma weak gpq_mpi_shim_set_device_ecd

typedef void *MPI;
MPI gcry_mpi_new(unsigned int nbits);
void gcry_mpi_release(MPI a);
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

/* an integer-valued double of any size, exactly */
static void set_integer(MPI r, double v)
{
  const double a = fabs(v);
  if (a < 9007199254740992.0) gcry_mpi_set_ui(r, (unsigned long)a);
  else {
    int e;
    const double m = frexp(a, &e);                        /* a = m 2^e, m 2^53 an integer */
    gcry_mpi_set_ui(r, (unsigned long)ldexp(m, 53));
    gcry_mpi_lshift(r, r, (unsigned)(e - 53));
  }
  if (v < 0) gcry_mpi_neg(r, r);
}

static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }

static unsigned long ecd_calls;
static double ecd_ms;                                     /* wall time spent inside he_ecd */
static void encode(struct he_pt *pt, const _Complex double *msg);
void he_ecd(struct he_pt *pt, const _Complex double *msg)
{
  const double t0 = now_ms();
  ecd_calls++;
  encode(pt, msg);
  ecd_ms += now_ms() - t0;
}
static void encode(struct he_pt *pt, const _Complex double *msg)
{
  pt->nu = hectx.Delta;
  const unsigned slots = hectx.slots, nh = polyctx.n / 2, gap = nh / slots;
  double *re = malloc(slots * sizeof *re), *im = malloc(slots * sizeof *im);
  for (unsigned i = 0; i < slots; i++) { re[i] = creal(msg[i]); im[i] = cimag(msg[i]); }
  for (unsigned len = slots; len >= 2; len >>= 1) {       /* invcanemb */
    const unsigned idx_mod = len << 2, step = polyctx.m / idx_mod, mid = len >> 1;
    for (unsigned i = 0; i < slots; i += len)
      for (unsigned j = 0; j < mid; j++) {
        const unsigned k = (idx_mod - polyctx.ring.cyc_group[j] % idx_mod) * step;
        const double c = creal(polyctx.ring.zetas[k]), s = cimag(polyctx.ring.zetas[k]);
        const double dr = re[i + j] - re[i + j + mid], di = im[i + j] - im[i + j + mid];
        re[i + j] = re[i + j] + re[i + j + mid];
        im[i + j] = im[i + j] + im[i + j + mid];
        const double p0 = dr * c, p1 = di * s, p2 = dr * s, p3 = di * c;
        re[i + j + mid] = p0 - p1;
        im[i + j + mid] = p2 + p3;
      }
  }
  for (unsigned i = 1, j = 0; i < slots; i++) {           /* bitrev_vec */
    unsigned bit = slots >> 1;
    for (; j >= bit; bit >>= 1) j -= bit;
    j += bit;
    if (i < j) { double t = re[i]; re[i] = re[j]; re[j] = t; t = im[i]; im[i] = im[j]; im[j] = t; }
  }
  for (unsigned i = 0; i < polyctx.n; i++) gcry_mpi_set_ui(pt->m.coeffs[i], 0);
  for (unsigned i = 0; i < slots; i++) {
    set_integer(pt->m.coeffs[i * gap], round(re[i] / slots * hectx.Delta));
    set_integer(pt->m.coeffs[i * gap + nh], round(im[i] / slots * hectx.Delta));
  }
  free(re); free(im);
}

static void ct_alloc(he_ct_t *ct) { poly_mpi_alloc(&ct->c0); poly_mpi_alloc(&ct->c1); }

static int same(const he_ct_t *a, const he_ct_t *b, const char *what)
{
  unsigned bad = 0, nonzero = 0;
  MPI zero = gcry_mpi_new(0);
  for (unsigned i = 0; i < polyctx.n; i++) {
    bad += gcry_mpi_cmp(a->c0.coeffs[i], b->c0.coeffs[i]) != 0, bad += gcry_mpi_cmp(a->c1.coeffs[i], b->c1.coeffs[i]) != 0;
    nonzero += gcry_mpi_cmp(a->c0.coeffs[i], zero) != 0;
  }
  gcry_mpi_release(zero);
  if (bad || a->l != b->l || memcmp(&a->nu, &b->nu, 8) || memcmp(&a->B, &b->B, 8) || nonzero < polyctx.n / 2) {
    printf("MISMATCH %s: %u coefficients, %u non-zero, l %u/%u, nu %.17g/%.17g, B %.17g/%.17g\n", what, bad, nonzero, a->l, b->l, a->nu, b->nu, a->B, b->B);
    return 1;
  }
  printf("ok %s\n", what);
  return 0;
}

static he_evk_t *rk;
static he_ct_t ct;

static void setup(unsigned logn, unsigned logq, unsigned slots)
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
  he_genrk(rk, &sk);
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

/* entries of magnitude up to 2^10 with all 53 bits in use: coefficients of about 40 bits at Delta = 2^30 */
static _Complex double *matrix(unsigned slots, uint64_t seed)
{
  _Complex double *A = malloc((size_t)slots * slots * sizeof *A);
  for (size_t i = 0; i < (size_t)slots * slots; i++) {
    const double x = ldexp((double)(splitmix64(&seed) >> 11), -43) - 512.0, y = ldexp((double)(splitmix64(&seed) >> 11), -43) - 512.0;
    A[i] = x + y * I;
  }
  return A;
}

static int bad;
static void expect(int cond, const char *what, unsigned long calls)
{
  if (cond) printf("ok %s\n", what);
  else { printf("FAIL %s (%lu he_ecd calls)\n", what, calls); bad = 1; }
}

/* which: 0 he_gemv(A), 1 he_sum, 2 he_idx(idx) */
static unsigned long run(he_ct_t *out, int which, const _Complex double *A, unsigned idx)
{
  const unsigned long before = ecd_calls;
  if (which == 0) he_gemv(out, A, &ct, rk);
  else if (which == 1) he_sum(out, &ct, rk);
  else he_idx(out, &ct, idx, rk);
  return ecd_calls - before;
}

static int check(unsigned slots)
{
  static const char *const names[3] = {"he_gemv", "he_sum", "he_idx"};
  _Complex double *A = matrix(slots, 5);
  he_ct_t off[3], on[3], fb_off, fb_on;
  char what[96];
  for (int w = 0; w < 3; w++) { ct_alloc(&off[w]); ct_alloc(&on[w]); }
  ct_alloc(&fb_off); ct_alloc(&fb_on);
  const unsigned idx = slots - 1;
  gpq_mpi_shim_set_device_ecd(0);
  for (int w = 0; w < 3; w++) {
    const unsigned long c = run(&off[w], w, A, idx);
    snprintf(what, sizeof what, "%s, switch off: one he_ecd call per diagonal", names[w]);
    expect(c == slots, what, c);
  }
  gpq_shim_gemv_plan_cache(0);                               /* the plans made with the host's encoder go */
  gpq_shim_gemv_plan_cache(4);
  gpq_mpi_shim_set_device_ecd(1);
  for (int w = 0; w < 3; w++) {
    const unsigned long c = run(&on[w], w, A, idx);
    snprintf(what, sizeof what, "%s, switch on: no he_ecd call", names[w]);
    expect(c == 0, what, c);
    snprintf(what, sizeof what, "%s, device encoder against host encoder", names[w]);
    bad |= same(&on[w], &off[w], what);
  }
  {                                                          /* the plan the device encoder made serves the repeat call */
    const unsigned long c = run(&on[0], 0, A, idx);
    expect(c == 0, "he_gemv again, switch on: no he_ecd call", c);
    bad |= same(&on[0], &off[0], "he_gemv again, the plan made on the device");
  }
  /* one entry of 2^40: times Delta = 2^30 and over `slots` still beyond 2^63 -- no image on the device, so he_ecd encodes after all */
  A[1 * slots + 2 % slots] = 1099511627776.0;
  gpq_shim_gemv_plan_cache(0);
  gpq_shim_gemv_plan_cache(4);
  unsigned long c = run(&fb_on, 0, A, idx);
  expect(c == slots, "out of range, switch on: falls back to he_ecd", c);
  gpq_shim_gemv_plan_cache(0);
  gpq_shim_gemv_plan_cache(4);
  gpq_mpi_shim_set_device_ecd(0);
  c = run(&fb_off, 0, A, idx);
  expect(c == slots, "out of range, switch off: he_ecd", c);
  bad |= same(&fb_on, &fb_off, "out of range: the fallback gives the host encoder's words");
  return bad;
}

static int firstcall(unsigned slots, int on)
{
  if (gpq_mpi_shim_set_device_ecd) gpq_mpi_shim_set_device_ecd(on);
  else if (on) { fprintf(stderr, "this build of the library has no gpq_mpi_shim_set_device_ecd\n"); return 2; }
  he_ct_t out;
  ct_alloc(&out);
  uint64_t seed = 1000;
  _Complex double *A = matrix(slots, seed);
  he_gemv(&out, A, &ct, rk);                                 /* warm-up: tables, keys, buffers */
  he_gemv(&out, A, &ct, rk);
  printf("ready\n");
  fflush(stdout);
  char line[64];
  while (fgets(line, sizeof line, stdin)) {
    if (!strncmp(line, "first", 5)) {
      gpq_shim_gemv_plan_cache(0);
      gpq_shim_gemv_plan_cache(4);
      free(A);
      A = matrix(slots, ++seed);
      const unsigned long c0 = ecd_calls;
      const double e0 = ecd_ms, t0 = now_ms();
      he_gemv(&out, A, &ct, rk);
      printf("first %.3f %.3f %lu\n", now_ms() - t0, ecd_ms - e0, ecd_calls - c0);
    } else if (!strncmp(line, "repeat", 6)) {
      const unsigned long c0 = ecd_calls;
      const double t0 = now_ms();
      he_gemv(&out, A, &ct, rk);
      printf("repeat %.3f 0 %lu\n", now_ms() - t0, ecd_calls - c0);
    } else break;
    fflush(stdout);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 6 && !strcmp(argv[1], "firstcall")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    return firstcall(atoi(argv[4]), atoi(argv[5]));
  }
  if (argc >= 5 && !strcmp(argv[1], "check")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    return check(atoi(argv[4]));
  }
  fprintf(stderr, "usage: ecd_host check <logn> <logq> <slots> | firstcall <logn> <logq> <slots> <on>\n");
  return 2;
}
