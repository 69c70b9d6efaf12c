/* enc_host.c -- he_keypair / he_enc_sk / he_enc_pk / he_dec of include/gpqhe_hip_compat.h with real libgcrypt MPIs.
 *
 *   enc_host <host|device> <logn> <logq> <minus> <slots> <dir>
 *
 * q_L = 2^logq - minus.  The host program's samplers are FILLERS: each call of sample_sk / sample_zo / sample_error / sample_uniform hands
 * out the next polynomial of <dir>/sk.txt, zo.txt, error.txt, uniform.txt (n lines of signed hexadecimal per polynomial, written by the
 * test), whatever q is -- no sampler algorithm lives here.  randombytes is a counter-driven stream of this program's own: byte k is byte
 * k % 8 of splitmix64 of (k / 8 + 1) * 0x9e3779b97f4a7c15 (stateless form below).  Every sampler and randombytes call is logged.
 * The plaintext is <dir>/m.txt.  With `device` gpq_mpi_shim_set_device_samplers(1) is set first.
 * Output: "call ..." lines in call order, "info ..." lines with the bookkeeping, and "poly <name>" followed by n hexadecimal lines for
 * sk, p0, p1, the two ciphertexts and their decryptions.  Setup as dcd_host.c. */
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
void gcry_mpi_sub_ui(MPI w, MPI u, unsigned long v);
void gcry_mpi_neg(MPI w, MPI u);
unsigned int gcry_mpi_scan(MPI *ret, int format, const void *buffer, size_t buflen, size_t *nscanned);
unsigned int gcry_mpi_print(int format, unsigned char *buffer, size_t buflen, size_t *nwritten, const MPI a);

static const char *dir;
static FILE *queue[4];
static const char *const queue_name[4] = {"sk", "zo", "error", "uniform"};

static void read_poly(FILE *f, poly_mpi_t *r, const char *what)
{
  char line[1024];
  for (unsigned i = 0; i < polyctx.n; i++) {
    if (!fgets(line, sizeof line, f)) { fprintf(stderr, "enc_host: %s has no polynomial left\n", what); exit(3); }
    line[strcspn(line, "\r\n")] = 0;
    const int neg = line[0] == '-';
    MPI t = NULL;
    if (gcry_mpi_scan(&t, 4, line + neg, 0, NULL)) { fprintf(stderr, "enc_host: bad line in %s\n", what); exit(3); }
    if (neg) gcry_mpi_neg(t, t);
    gcry_mpi_set(r->coeffs[i], t);
    gcry_mpi_release(t);
  }
}

static void next_poly(int k, poly_mpi_t *r)
{
  if (!queue[k]) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s.txt", dir, queue_name[k]);
    if (!(queue[k] = fopen(path, "r"))) { perror(path); exit(3); }
  }
  printf("call sample_%s\n", queue_name[k]);
  read_poly(queue[k], r, queue_name[k]);
}

/* the four samplers the library reaches through weak references (src/sample.c's names), as fillers */
void sample_sk(poly_mpi_t *r) { next_poly(0, r); }
void sample_zo(poly_mpi_t *r) { next_poly(1, r); }
void sample_error(poly_mpi_t *r) { next_poly(2, r); }
void sample_uniform(poly_mpi_t *r, const MPI q) { (void)q; next_poly(3, r); }

static uint64_t stream_pos;
void randombytes(uint8_t *x, size_t xlen)
{
  printf("call randombytes %zu\n", xlen);
  for (size_t i = 0; i < xlen; i++, stream_pos++) {
    uint64_t z = (stream_pos / 8 + 1) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    x[i] = (uint8_t)(z >> (8 * (stream_pos % 8)));
  }
}

static void dump(const char *name, const poly_mpi_t *p)
{
  unsigned char buf[1024];
  printf("poly %s\n", name);
  for (unsigned i = 0; i < polyctx.n; i++) {
    size_t len = 0;
    if (gcry_mpi_print(4, buf, sizeof buf, &len, p->coeffs[i])) { fprintf(stderr, "enc_host: gcry_mpi_print failed\n"); exit(3); }
    printf("%s\n", (const char *)buf);
  }
}

static void info(const char *name, const he_ct_t *ct)
{
  uint64_t nu, B, bc;
  memcpy(&nu, &ct->nu, 8); memcpy(&B, &ct->B, 8); memcpy(&bc, &hectx.bnd.Bclean, 8);
  printf("info %s l %u L %u nu %016llx B %016llx Bclean %016llx\n", name, ct->l, hectx.L, (unsigned long long)nu, (unsigned long long)B, (unsigned long long)bc);
}

int main(int argc, char **argv)
{
  if (argc < 7) { fprintf(stderr, "usage: enc_host host|device <logn> <logq> <minus> <slots> <dir>\n"); return 2; }
  const unsigned logn = atoi(argv[2]), logq = atoi(argv[3]), slots = atoi(argv[5]);
  const unsigned long minus = strtoul(argv[4], NULL, 10);
  dir = argv[6];
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  if (minus) gcry_mpi_sub_ui(q, q, minus);
  hectx_init(logn, q, slots, 1ull << 30);
  gpq_mpi_shim_set_device_samplers(!strcmp(argv[1], "device"));

  he_pk_t pk;
  poly_mpi_t sk;
  he_ct_t ct_sk, ct_pk;
  he_pt_t pt, back;
  poly_mpi_alloc(&pk.p0); poly_mpi_alloc(&pk.p1); poly_mpi_alloc(&sk);
  poly_mpi_alloc(&ct_sk.c0); poly_mpi_alloc(&ct_sk.c1); poly_mpi_alloc(&ct_pk.c0); poly_mpi_alloc(&ct_pk.c1);
  poly_mpi_alloc(&pt.m); poly_mpi_alloc(&back.m);
  char path[4096];
  snprintf(path, sizeof path, "%s/m.txt", dir);
  FILE *fm = fopen(path, "r");
  if (!fm) { perror(path); return 3; }
  read_poly(fm, &pt.m, "m");
  fclose(fm);
  pt.nu = (double)(1ull << 30);

  printf("call he_keypair\n");
  he_keypair(&pk, &sk);
  printf("\n");
  dump("sk", &sk); dump("p0", &pk.p0); dump("p1", &pk.p1);
  printf("call he_enc_sk\n");
  he_enc_sk(&ct_sk, &pt, &sk);
  info("he_enc_sk", &ct_sk);
  dump("sk_c0", &ct_sk.c0); dump("sk_c1", &ct_sk.c1);
  printf("call he_enc_pk\n");
  he_enc_pk(&ct_pk, &pt, &pk);
  info("he_enc_pk", &ct_pk);
  dump("pk_c0", &ct_pk.c0); dump("pk_c1", &ct_pk.c1);
  he_dec(&back, &ct_sk, &sk);
  dump("dec_sk", &back.m);
  he_dec(&back, &ct_pk, &sk);
  dump("dec_pk", &back.m);
  /* once more with everything resident: other samples, the same keys and plaintext */
  printf("call he_enc_pk again\n");
  he_enc_pk(&ct_pk, &pt, &pk);
  dump("pk2_c0", &ct_pk.c0); dump("pk2_c1", &ct_pk.c1);
  he_dec(&back, &ct_pk, &sk);
  dump("dec_pk2", &back.m);
  printf("done\n");
  return 0;
}
