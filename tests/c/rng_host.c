/* rng_host.c -- he_keypair / he_enc_sk / he_enc_pk / he_genrlk / he_genck / he_genrk of include/gpqhe_hip_compat.h with real libgcrypt
 * MPIs in a host program whose randombytes FORWARDS to the library's default stream (gpq_randombytes), as a GPQHE build does under its
 * GPQHE_HIP guard.
 *
 *   rng_host <host|device> <logn> <logq> <slots> <dir>
 *
 * q_L = 2^logq.  gpq_mpi_shim_set_device_samplers(1) always; with `device` gpq_mpi_shim_set_device_rng(1) as well.  The only sampler this
 * program has is sample_sk (64 non-zero coefficients, drawn from randombytes: 8 bytes of signs, then 8 bytes per candidate position), so
 * the secret comes from the same stream as everything else.  Every randombytes call is logged.  The plaintext is <dir>/m.txt.
 * Output: "call ..." lines in call order, "pos <name> <lo> <hi>" with the default stream's position after every drop-in call, "poly
 * <name>" followed by n hexadecimal lines, and the keys as raw words in <dir>/keys.bin -- rlk.p0, rlk.p1, ck.p0, ck.p1, rk[0].p0, ... */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpqhe_hip.h"
#include "gpqhe_hip_compat.h"
#include "gpqhe_hip_ctx.h"

typedef void *MPI;
MPI gcry_mpi_new(unsigned int nbits);
void gcry_mpi_release(MPI a);
MPI gcry_mpi_set(MPI w, const MPI u);
MPI gcry_mpi_set_ui(MPI w, unsigned long u);
void gcry_mpi_lshift(MPI x, MPI a, unsigned int n);
void gcry_mpi_neg(MPI w, MPI u);
unsigned int gcry_mpi_scan(MPI *ret, int format, const void *buffer, size_t buflen, size_t *nscanned);
unsigned int gcry_mpi_print(int format, unsigned char *buffer, size_t buflen, size_t *nwritten, const MPI a);

void randombytes(uint8_t *x, size_t xlen)
{
  printf("call randombytes %zu\n", xlen);
  gpq_randombytes(x, xlen);
}

static uint64_t draw64(void)
{
  uint8_t b[8];
  uint64_t v = 0;
  randombytes(b, 8);
  for (int i = 0; i < 8; i++) v |= (uint64_t)b[i] << (8 * i);
  return v;
}

/* 64 coefficients +-1 at distinct positions: bit k of the first draw is the sign of the k-th position found */
void sample_sk(poly_mpi_t *r)
{
  const unsigned n = polyctx.n;
  printf("call sample_sk\n");
  for (unsigned i = 0; i < n; i++) gcry_mpi_set_ui(r->coeffs[i], 0);
  char *taken = calloc(n, 1);
  const uint64_t signs = draw64();
  for (unsigned found = 0; found < 64;) {
    const unsigned i = (unsigned)(draw64() & (n - 1));
    if (taken[i]) continue;
    taken[i] = 1;
    gcry_mpi_set_ui(r->coeffs[i], 1);
    if ((signs >> found) & 1) gcry_mpi_neg(r->coeffs[i], r->coeffs[i]);
    found++;
  }
  free(taken);
}

static void dump(const char *name, const poly_mpi_t *p)
{
  unsigned char buf[1024];
  printf("poly %s\n", name);
  for (unsigned i = 0; i < polyctx.n; i++) {
    size_t len = 0;
    if (gcry_mpi_print(4, buf, sizeof buf, &len, p->coeffs[i])) { fprintf(stderr, "rng_host: gcry_mpi_print failed\n"); exit(3); }
    printf("%s\n", (const char *)buf);
  }
}

static void pos(const char *name)
{
  uint64_t p[2];
  if (gpq_randombytes_tell(p)) { fprintf(stderr, "rng_host: gpq_randombytes_tell failed\n"); exit(3); }
  printf("\npos %s %llu %llu\n", name, (unsigned long long)p[0], (unsigned long long)p[1]);
}

static void key_alloc(he_evk_t *k, size_t words)
{
  k->p0.coeffs = malloc(words * 8); k->p1.coeffs = malloc(words * 8);
  if (!k->p0.coeffs || !k->p1.coeffs) { fprintf(stderr, "rng_host: out of memory\n"); exit(3); }
}

static void key_write(FILE *f, const he_evk_t *k, size_t words)
{
  if (fwrite(k->p0.coeffs, 8, words, f) != words || fwrite(k->p1.coeffs, 8, words, f) != words) { perror("keys.bin"); exit(3); }
}

int main(int argc, char **argv)
{
  if (argc < 6) { fprintf(stderr, "usage: rng_host host|device <logn> <logq> <slots> <dir>\n"); return 2; }
  const unsigned logn = atoi(argv[2]), logq = atoi(argv[3]), slots = atoi(argv[4]);
  const char *dir = argv[5];
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  hectx_init(logn, q, slots, 1ull << 30);
  gpq_mpi_shim_set_device_samplers(1);
  gpq_mpi_shim_set_device_rng(!strcmp(argv[1], "device"));

  he_pk_t pk;
  poly_mpi_t sk;
  he_ct_t ct_sk, ct_pk;
  he_pt_t pt;
  poly_mpi_alloc(&pk.p0); poly_mpi_alloc(&pk.p1); poly_mpi_alloc(&sk);
  poly_mpi_alloc(&ct_sk.c0); poly_mpi_alloc(&ct_sk.c1); poly_mpi_alloc(&ct_pk.c0); poly_mpi_alloc(&ct_pk.c1);
  poly_mpi_alloc(&pt.m);
  char path[4096], line[1024];
  snprintf(path, sizeof path, "%s/m.txt", dir);
  FILE *fm = fopen(path, "r");
  if (!fm) { perror(path); return 3; }
  for (unsigned i = 0; i < polyctx.n; i++) {
    if (!fgets(line, sizeof line, fm)) { fprintf(stderr, "rng_host: m.txt is too short\n"); return 3; }
    line[strcspn(line, "\r\n")] = 0;
    const int neg = line[0] == '-';
    MPI t = NULL;
    if (gcry_mpi_scan(&t, 4, line + neg, 0, NULL)) { fprintf(stderr, "rng_host: bad line in m.txt\n"); return 3; }
    if (neg) gcry_mpi_neg(t, t);
    gcry_mpi_set(pt.m.coeffs[i], t);
    gcry_mpi_release(t);
  }
  fclose(fm);
  pt.nu = (double)(1ull << 30);

  printf("call he_keypair\n");
  he_keypair(&pk, &sk);
  pos("he_keypair");
  dump("sk", &sk); dump("p0", &pk.p0); dump("p1", &pk.p1);
  printf("call he_enc_sk\n");
  he_enc_sk(&ct_sk, &pt, &sk);
  pos("he_enc_sk");
  dump("sk_c0", &ct_sk.c0); dump("sk_c1", &ct_sk.c1);
  printf("call he_enc_pk\n");
  he_enc_pk(&ct_pk, &pt, &pk);
  pos("he_enc_pk");
  dump("pk_c0", &ct_pk.c0); dump("pk_c1", &ct_pk.c1);

  const size_t words = (size_t)hectx.dimevk * polyctx.n;
  he_evk_t rlk, ck, *rk = malloc(slots * sizeof *rk);
  key_alloc(&rlk, words); key_alloc(&ck, words);
  for (unsigned k = 0; k < slots; k++) key_alloc(&rk[k], words);
  printf("call he_genrlk\n");
  he_genrlk(&rlk, &sk);
  pos("he_genrlk");
  printf("call he_genck\n");
  he_genck(&ck, &sk);
  pos("he_genck");
  printf("call he_genrk\n");
  he_genrk(rk, &sk);
  pos("he_genrk");
  snprintf(path, sizeof path, "%s/keys.bin", dir);
  FILE *o = fopen(path, "wb");
  if (!o) { perror(path); return 3; }
  key_write(o, &rlk, words); key_write(o, &ck, words);
  for (unsigned k = 0; k < slots; k++) key_write(o, &rk[k], words);
  fclose(o);
  printf("done\n");
  return 0;
}
