/* dcd_host.c -- gpq_shim_he_dec_dcd (include/gpqhe_hip_compat.h) with real libgcrypt MPIs: he_dec followed by he_dcd with the plaintext
 * staying on the device, against the shim's he_dec followed by the host program's own decoder.
 *
 *   dcd_host check <logn> <logq> <slots>      the doubles of both routes, bit for bit, twice (the second time everything is resident), a
 *                                             third time after a host-side edit of c1 (`poly stats` lines around the device route), and
 *                                             he_dec alone afterwards still gives the same integers
 *   dcd_host fallback <logn> <logq> <slots>   q = 2^logq - 159, no power of two: the call returns 0 and leaves m untouched
 *   dcd_host time <logn> <logq> <slots> <iterations>
 *                                             milliseconds per call of (A) he_dec + host decode and (B) gpq_shim_he_dec_dcd, interleaved
 *                                             after warm-up; every call ends with its result on the host
 *
 * decode below is the decoder of src/he-encode.c:66-74 with canemb (src/canemb.c:43-60) and the bit loop of mpi_to_double
 * (src/types.c:77-106), stated in plain C for this test from their semantics: it reads polyctx.ring.zetas, computes the powers of 5
 * itself and must be compiled without fused multiply-add (-ffp-contract=off).  Setup as ecd_host.c. */
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
void gcry_mpi_sub(MPI w, MPI u, MPI v);
void gcry_mpi_sub_ui(MPI w, MPI u, unsigned long v);
void gcry_mpi_add_ui(MPI w, MPI u, unsigned long v);
void gcry_mpi_neg(MPI w, MPI u);
void gcry_mpi_mod(MPI r, MPI dividend, MPI divisor);
void gcry_mpi_rshift(MPI x, MPI a, unsigned int n);
int gcry_mpi_cmp(const MPI u, const MPI v);
int gcry_mpi_cmp_ui(const MPI u, unsigned long v);
int gcry_mpi_is_neg(MPI a);
int gcry_mpi_test_bit(MPI a, unsigned int n);
unsigned int gcry_mpi_get_nbits(MPI a);
unsigned int gcry_mpi_scan(MPI *ret, int format, const void *buffer, size_t buflen, size_t *nscanned);

static uint64_t splitmix64(uint64_t *s)
{
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
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

static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }

/* the magnitude's bits from the top down, num = num * 2 + bit in double arithmetic; the sign last */
static double to_double(MPI a)
{
  unsigned length = gcry_mpi_get_nbits(a);
  if (!length) return 0;
  const int neg = gcry_mpi_is_neg(a);
  MPI b = gcry_mpi_new(0);
  gcry_mpi_set(b, a);
  if (neg) gcry_mpi_neg(b, b);
  double num = 0;
  while (length-- > 0) {
    num = num * 2.;
    num = num + gcry_mpi_test_bit(b, length);
  }
  gcry_mpi_release(b);
  return neg ? -num : num;
}

static void decode(_Complex double *z, const struct he_pt *pt)
{
  const unsigned slots = hectx.slots, nh = polyctx.n / 2, gap = nh / slots;
  double *re = malloc(slots * sizeof *re), *im = malloc(slots * sizeof *im);
  unsigned *pow5 = malloc((slots / 2 + 1) * sizeof *pow5);
  pow5[0] = 1;
  for (unsigned j = 1; j < slots / 2; j++) pow5[j] = (unsigned)((5ull * pow5[j - 1]) % polyctx.m);   /* 5^j mod m; mod 4 len below */
  for (unsigned i = 0; i < slots; i++) {
    re[i] = to_double(pt->m.coeffs[i * gap]) / pt->nu;
    im[i] = to_double(pt->m.coeffs[i * gap + nh]) / pt->nu;
  }
  for (unsigned i = 1, j = 0; i < slots; i++) {             /* bit reversal */
    unsigned bit = slots >> 1;
    for (; j >= bit; bit >>= 1) j -= bit;
    j += bit;
    if (i < j) { double t = re[i]; re[i] = re[j]; re[j] = t; t = im[i]; im[i] = im[j]; im[j] = t; }
  }
  for (unsigned len = 2; len <= slots; len <<= 1) {
    const unsigned idx_mod = len << 2, step = polyctx.m / idx_mod, mid = len >> 1;
    for (unsigned i = 0; i < slots; i += len)
      for (unsigned j = 0; j < mid; j++) {
        const unsigned k = (pow5[j] % idx_mod) * step;
        const double c = creal(polyctx.ring.zetas[k]), s = cimag(polyctx.ring.zetas[k]);
        const double ur = re[i + j], ui = im[i + j], br = re[i + j + mid], bi = im[i + j + mid];
        const double p0 = br * c, p1 = bi * s, p2 = br * s, p3 = bi * c;
        const double vr = p0 - p1, vi = p2 + p3;
        re[i + j] = ur + vr; im[i + j] = ui + vi;
        re[i + j + mid] = ur - vr; im[i + j + mid] = ui - vi;
      }
  }
  for (unsigned i = 0; i < slots; i++) { double pair[2] = {re[i], im[i]}; memcpy(&z[i], pair, sizeof pair); }
  free(re); free(im); free(pow5);
}

static poly_mpi_t sk;
static he_ct_t ct;

static void setup(unsigned logn, unsigned logq, unsigned slots, unsigned long minus)
{
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  if (minus) gcry_mpi_sub_ui(q, q, minus);
  hectx_init(logn, q, slots, 1ull << 30);
  poly_mpi_alloc(&sk);
  uint64_t st = 333;
  for (unsigned i = 0; i < polyctx.n; i++) {                 /* ternary */
    const unsigned v = (unsigned)(splitmix64(&st) % 3);
    gcry_mpi_set_ui(sk.coeffs[i], v == 2 ? 1 : v);
    if (v == 2) gcry_mpi_neg(sk.coeffs[i], sk.coeffs[i]);
  }
  poly_mpi_alloc(&ct.c0); poly_mpi_alloc(&ct.c1);
  ct.l = hectx.L; ct.nu = hectx.Delta * 3.5 + 1.0; ct.B = 17.25;     /* nu: no power of two */
  MPI qh = gcry_mpi_new(0);
  gcry_mpi_rshift(qh, hectx.q[ct.l], 1);
  uint64_t s2 = 444;
  for (unsigned i = 0; i < polyctx.n; i++) {                  /* centred uniform mod q_L */
    uniform_mod(ct.c0.coeffs[i], hectx.q[ct.l], &s2);
    uniform_mod(ct.c1.coeffs[i], hectx.q[ct.l], &s2);
    if (gcry_mpi_cmp(ct.c0.coeffs[i], qh) >= 0) gcry_mpi_sub(ct.c0.coeffs[i], ct.c0.coeffs[i], hectx.q[ct.l]);
    if (gcry_mpi_cmp(ct.c1.coeffs[i], qh) >= 0) gcry_mpi_sub(ct.c1.coeffs[i], ct.c1.coeffs[i], hectx.q[ct.l]);
  }
  gcry_mpi_release(qh);
  gcry_mpi_release(q);
}

static int bad;
static void expect(int cond, const char *what)
{
  if (cond) printf("ok %s\n", what);
  else { printf("FAIL %s\n", what); bad = 1; }
}

static int same_doubles(const _Complex double *a, const _Complex double *b, unsigned slots, const char *what)
{
  unsigned differ = 0, nonzero = 0, first = 0;
  for (unsigned i = 0; i < slots; i++) {
    if (memcmp(&a[i], &b[i], sizeof a[i])) { if (!differ) first = i; differ++; }
    nonzero += creal(a[i]) != 0 && cimag(a[i]) != 0 && isfinite(creal(a[i])) && isfinite(cimag(a[i]));
  }
  if (differ || nonzero < slots) {
    printf("MISMATCH %s: %u of %u slots differ (%u non-zero), first %u: %.17g%+.17gi vs %.17g%+.17gi\n", what, differ, slots, nonzero, first,
           creal(a[first]), cimag(a[first]), creal(b[first]), cimag(b[first]));
    return 1;
  }
  printf("ok %s\n", what);
  return 0;
}

static void poly_stats(const char *when)
{
  uint64_t confirmed = 0, changed = 0;
  gpq_mpi_shim_poly_stats(&confirmed, &changed);
  printf("poly stats %s: resident %u confirmed %llu changed %llu\n", when, gpq_mpi_shim_resident_polys(), (unsigned long long)confirmed, (unsigned long long)changed);
}

static int check(unsigned slots)
{
  struct he_pt pt, pt2;
  poly_mpi_alloc(&pt.m); poly_mpi_alloc(&pt2.m);
  _Complex double *za = malloc(slots * sizeof *za), *zb = malloc(slots * sizeof *zb);
  for (int round = 0; round < 2; round++) {
    memset(zb, 0x5a, slots * sizeof *zb);
    he_dec(&pt, &ct, &sk);
    decode(za, &pt);
    const int rc = gpq_shim_he_dec_dcd(zb, &ct, &sk);
    expect(rc == 1, round ? "again: gpq_shim_he_dec_dcd returns 1" : "gpq_shim_he_dec_dcd returns 1");
    bad |= same_doubles(zb, za, slots, round ? "again, everything resident: device decode against he_dec + host decode" : "device decode against he_dec + host decode");
  }
  /* a third round with one coefficient of c1 edited behind the library's back.  The device route goes FIRST: it starts from the kept
   * copies, its recheck finds the edit and the device work runs again (a polynomial found changed is not trusted by the call after) */
  gcry_mpi_add_ui(ct.c1.coeffs[polyctx.n / 3], ct.c1.coeffs[polyctx.n / 3], 1);
  memset(zb, 0x5a, slots * sizeof *zb);
  poly_stats("before the edited call");
  const int rc3 = gpq_shim_he_dec_dcd(zb, &ct, &sk);
  poly_stats("after the edited call");
  expect(rc3 == 1, "after a host edit: gpq_shim_he_dec_dcd returns 1");
  he_dec(&pt, &ct, &sk);
  decode(za, &pt);
  bad |= same_doubles(zb, za, slots, "after a host edit: device decode against he_dec + host decode");
  expect(memcmp(&pt.nu, &ct.nu, 8) == 0, "he_dec copies nu");
  he_dec(&pt2, &ct, &sk);
  unsigned differ = 0, nonzero = 0;
  for (unsigned i = 0; i < polyctx.n; i++) { differ += gcry_mpi_cmp(pt.m.coeffs[i], pt2.m.coeffs[i]) != 0; nonzero += gcry_mpi_cmp_ui(pt2.m.coeffs[i], 0) != 0; }
  expect(!differ && nonzero > polyctx.n / 2, "he_dec alone afterwards: the same integers");
  return bad;
}

static int fallback(unsigned slots)
{
  _Complex double *z = malloc(slots * sizeof *z), *was = malloc(slots * sizeof *was);
  memset(z, 0x5a, slots * sizeof *z);
  memcpy(was, z, slots * sizeof *z);
  const int rc = gpq_shim_he_dec_dcd(z, &ct, &sk);
  expect(rc == 0, "q_l no power of two: returns 0");
  expect(!memcmp(z, was, slots * sizeof *z), "q_l no power of two: m untouched");
  struct he_pt pt;
  poly_mpi_alloc(&pt.m);
  he_dec(&pt, &ct, &sk);                                      /* the caller's route still works */
  decode(z, &pt);
  expect(isfinite(creal(z[0])) && memcmp(z, was, sizeof *z), "q_l no power of two: he_dec + host decode");
  return bad;
}

static int cmp_double(const void *a, const void *b) { const double x = *(const double *)a, y = *(const double *)b; return (x > y) - (x < y); }

static int timing(unsigned slots, unsigned iterations)
{
  struct he_pt pt;
  poly_mpi_alloc(&pt.m);
  _Complex double *za = malloc(slots * sizeof *za), *zb = malloc(slots * sizeof *zb);
  for (int w = 0; w < 3; w++) {                               /* warm-up: tables, buffers, residency */
    he_dec(&pt, &ct, &sk);
    decode(za, &pt);
    if (gpq_shim_he_dec_dcd(zb, &ct, &sk) != 1) { printf("FAIL gpq_shim_he_dec_dcd fell back\n"); return 1; }
  }
  if (same_doubles(zb, za, slots, "time: both routes give the same doubles")) return 1;
  double *a = malloc(iterations * sizeof *a), *b = malloc(iterations * sizeof *b), *d = malloc(iterations * sizeof *d);
  for (unsigned k = 0; k < iterations; k++) {                 /* interleaved: A, B, A, B, ... */
    double t0 = now_ms();
    he_dec(&pt, &ct, &sk);
    const double t1 = now_ms();
    decode(za, &pt);
    a[k] = now_ms() - t0; d[k] = a[k] - (t1 - t0);
    t0 = now_ms();
    (void)gpq_shim_he_dec_dcd(zb, &ct, &sk);
    b[k] = now_ms() - t0;
    printf("pair %u: A %.3f ms (host decode %.3f)  B %.3f ms\n", k, a[k], d[k], b[k]);
  }
  unsigned faster = 0;
  for (unsigned k = 0; k < iterations; k++) faster += b[k] < a[k];
  qsort(a, iterations, sizeof *a, cmp_double); qsort(b, iterations, sizeof *b, cmp_double); qsort(d, iterations, sizeof *d, cmp_double);
  printf("logn %u slots %u q_L bits %u W-words down: A %zu bytes, B %zu bytes\n", polyctx.logn, slots, gcry_mpi_get_nbits(hectx.q[ct.l]),
         (size_t)(gcry_mpi_get_nbits(hectx.q[ct.l]) / 64 + 1) * 8 * polyctx.n, (size_t)slots * 16);
  printf("median ms per call: A (he_dec + host decode) %.3f [min %.3f max %.3f], of which host decode %.3f; B (gpq_shim_he_dec_dcd) %.3f [min %.3f max %.3f]; "
         "B faster in %u of %u pairs\n", a[iterations / 2], a[0], a[iterations - 1], d[iterations / 2], b[iterations / 2], b[0], b[iterations - 1], faster, iterations);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 5 && !strcmp(argv[1], "check")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0);
    return check(atoi(argv[4]));
  }
  if (argc >= 5 && !strcmp(argv[1], "fallback")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 159);
    return fallback(atoi(argv[4]));
  }
  if (argc >= 6 && !strcmp(argv[1], "time")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0);
    return timing(atoi(argv[4]), atoi(argv[5]));
  }
  fprintf(stderr, "usage: dcd_host check|fallback <logn> <logq> <slots> | time <logn> <logq> <slots> <iterations>\n");
  return 2;
}
