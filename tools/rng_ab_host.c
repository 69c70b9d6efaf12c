/* rng_ab_host.c -- the timing host of tools/rng_ab.py: he_genrk and he_enc_sk through the MPI-typed surface (include/gpqhe_hip_compat.h) in
 * a program whose randombytes forwards to gpq_randombytes, with the device samplers fed
 *   A  by that randombytes on the host (bytes generated on one CPU core, then uploaded), or
 *   B  by the device generator (gpq_mpi_shim_set_device_rng(1)).
 *
 *   rng_ab_host <A|B> <logn> <logq> <slots> <reps>
 *
 * Every timed call starts from stream position 0, so A and B make the same keys and ciphertexts: a checksum of the words is printed
 * beside every wall time.  The first line is the host generator's rate on this machine. */
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
MPI gcry_mpi_set_ui(MPI w, unsigned long u);
void gcry_mpi_lshift(MPI x, MPI a, unsigned int n);
void gcry_mpi_neg(MPI w, MPI u);
unsigned int gcry_mpi_print(int format, unsigned char *buffer, size_t buflen, size_t *nwritten, const MPI a);

void randombytes(uint8_t *x, size_t xlen) { gpq_randombytes(x, xlen); }

static double now_ms(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

static uint64_t fnv(uint64_t h, const void *p, size_t bytes)
{
  const uint8_t *b = p;
  for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

static uint64_t fnv_words(uint64_t h, const uint64_t *w, size_t words)
{
  for (size_t i = 0; i < words; i++) h = (h ^ w[i]) * 0x100000001b3ull;
  return h;
}

static uint64_t poly_sum(uint64_t h, const poly_mpi_t *p)
{
  unsigned char buf[1024];
  for (unsigned i = 0; i < polyctx.n; i++) {
    size_t len = 0;
    if (gcry_mpi_print(4, buf, sizeof buf, &len, p->coeffs[i])) { fprintf(stderr, "rng_ab_host: gcry_mpi_print failed\n"); exit(3); }
    h = fnv(h, buf, len);
  }
  return h;
}

int main(int argc, char **argv)
{
  if (argc < 6) { fprintf(stderr, "usage: rng_ab_host A|B <logn> <logq> <slots> <reps>\n"); return 2; }
  const int device = !strcmp(argv[1], "B");
  const unsigned logn = atoi(argv[2]), logq = atoi(argv[3]), slots = atoi(argv[4]), reps = atoi(argv[5]);

  const size_t probe = 4u << 20;
  uint8_t *buf = malloc(probe);
  double t0 = now_ms();
  gpq_randombytes(buf, probe);
  printf("host randombytes: %.1f MB/s (%zu bytes on one core)\n", probe / (now_ms() - t0) / 1e3, probe);
  free(buf);

  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  hectx_init(logn, q, slots, 1ull << 30);
  gpq_mpi_shim_set_device_samplers(1);
  gpq_mpi_shim_set_device_rng(device);

  poly_mpi_t sk;
  he_ct_t ct;
  he_pt_t pt;
  poly_mpi_alloc(&sk); poly_mpi_alloc(&ct.c0); poly_mpi_alloc(&ct.c1); poly_mpi_alloc(&pt.m);
  for (unsigned i = 0; i < polyctx.n; i++) {                 /* a ternary secret and a small plaintext: fixed, not random */
    gcry_mpi_set_ui(sk.coeffs[i], i % 1024 == 5);
    if (i % 2048 == 5) gcry_mpi_neg(sk.coeffs[i], sk.coeffs[i]);
    gcry_mpi_set_ui(pt.m.coeffs[i], (i * 2654435761u) >> 4);
  }
  pt.nu = (double)(1ull << 30);
  const size_t words = (size_t)hectx.dimevk * polyctx.n;
  he_evk_t *rk = malloc(slots * sizeof *rk);
  for (unsigned k = 0; k < slots; k++) {
    rk[k].p0.coeffs = malloc(words * 8); rk[k].p1.coeffs = malloc(words * 8);
    if (!rk[k].p0.coeffs || !rk[k].p1.coeffs) { fprintf(stderr, "rng_ab_host: out of memory\n"); return 3; }
  }
  printf("shape: n = 2^%u, q_L = 2^%u, dim %u, dimevk %u, %u rotation keys\n", logn, logq, hectx.dim, hectx.dimevk, slots);

  for (unsigned r = 0; r <= reps; r++) {                     /* repetition 0 warms up: tables, pools, code objects */
    uint64_t pos[2];
    gpq_randombytes_seed(NULL);
    t0 = now_ms();
    he_genrk(rk, &sk);
    const double ms_rk = now_ms() - t0;
    gpq_randombytes_tell(pos);
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned k = 0; k < slots; k++) { h = fnv_words(h, rk[k].p0.coeffs, words); h = fnv_words(h, rk[k].p1.coeffs, words); }
    printf("\n%s he_genrk %u keys%s: %.1f ms, %llu bytes drawn, checksum %016llx\n", argv[1], slots, r ? "" : " (warm-up)", ms_rk,
           (unsigned long long)pos[0], (unsigned long long)h);
    gpq_randombytes_seed(NULL);
    t0 = now_ms();
    he_enc_sk(&ct, &pt, &sk);
    const double ms_enc = now_ms() - t0;
    gpq_randombytes_tell(pos);
    printf("%s he_enc_sk%s: %.1f ms, %llu bytes drawn, checksum %016llx\n", argv[1], r ? "" : " (warm-up)", ms_enc, (unsigned long long)pos[0],
           (unsigned long long)poly_sum(poly_sum(0xcbf29ce484222325ull, &ct.c0), &ct.c1));
    fflush(stdout);
  }
  return 0;
}
