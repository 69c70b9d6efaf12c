/* keygen_host.c -- he_genrlk / he_genck / he_genrk of include/gpqhe_hip_compat.h with real libgcrypt MPIs, then he_rot and he_mul with
 * the keys they made.
 *
 *   keygen_host <host|device> <logn> <logq> <slots> <rot> <dir>
 *
 * q_L = 2^logq.  The secret is <dir>/sk.txt and the ciphertext (c0, c1) <dir>/ct.txt (n lines of signed hexadecimal per polynomial).
 * The host program's samplers are FILLERS as in enc_host.c: each call of sample_error / sample_uniform hands out the next polynomial of
 * <dir>/error.txt / uniform.txt; randombytes is the same counter-driven stream.  Every sampler and randombytes call is logged.  With
 * `device` gpq_mpi_shim_set_device_samplers(1) is set first.
 * Output: "call ..." lines in call order; the keys as raw words in <dir>/keys.bin -- rlk.p0, rlk.p1, ck.p0, ck.p1, rk[0].p0, rk[0].p1, ...,
 * dimevk * n words each; "poly <name>" followed by n hexadecimal lines for he_rot(ct, rot) and he_mul(ct, ct). */
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

static const char *dir;
static FILE *queue[2];
static const char *const queue_name[2] = {"error", "uniform"};

static void read_poly(FILE *f, poly_mpi_t *r, const char *what)
{
  char line[1024];
  for (unsigned i = 0; i < polyctx.n; i++) {
    if (!fgets(line, sizeof line, f)) { fprintf(stderr, "keygen_host: %s has no polynomial left\n", what); exit(3); }
    line[strcspn(line, "\r\n")] = 0;
    const int neg = line[0] == '-';
    MPI t = NULL;
    if (gcry_mpi_scan(&t, 4, line + neg, 0, NULL)) { fprintf(stderr, "keygen_host: bad line in %s\n", what); exit(3); }
    if (neg) gcry_mpi_neg(t, t);
    gcry_mpi_set(r->coeffs[i], t);
    gcry_mpi_release(t);
  }
}

static FILE *open_in(const char *name)
{
  char path[4096];
  snprintf(path, sizeof path, "%s/%s.txt", dir, name);
  FILE *f = fopen(path, "r");
  if (!f) { perror(path); exit(3); }
  return f;
}

static void next_poly(int k, poly_mpi_t *r)
{
  if (!queue[k]) queue[k] = open_in(queue_name[k]);
  printf("call sample_%s\n", queue_name[k]);
  read_poly(queue[k], r, queue_name[k]);
}

/* the samplers the library reaches through weak references (src/sample.c's names), as fillers */
void sample_error(poly_mpi_t *r) { next_poly(0, r); }
void sample_uniform(poly_mpi_t *r, const MPI q) { (void)q; next_poly(1, r); }

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
    if (gcry_mpi_print(4, buf, sizeof buf, &len, p->coeffs[i])) { fprintf(stderr, "keygen_host: gcry_mpi_print failed\n"); exit(3); }
    printf("%s\n", (const char *)buf);
  }
}

static void key_alloc(he_evk_t *k, size_t words)
{
  k->p0.coeffs = malloc(words * 8); k->p1.coeffs = malloc(words * 8);
  if (!k->p0.coeffs || !k->p1.coeffs) { fprintf(stderr, "keygen_host: out of memory\n"); exit(3); }
}

static void key_write(FILE *f, const he_evk_t *k, size_t words)
{
  if (fwrite(k->p0.coeffs, 8, words, f) != words || fwrite(k->p1.coeffs, 8, words, f) != words) { perror("keys.bin"); exit(3); }
}

int main(int argc, char **argv)
{
  if (argc < 7) { fprintf(stderr, "usage: keygen_host host|device <logn> <logq> <slots> <rot> <dir>\n"); return 2; }
  const unsigned logn = atoi(argv[2]), logq = atoi(argv[3]), slots = atoi(argv[4]);
  const int rot = atoi(argv[5]);
  dir = argv[6];
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  hectx_init(logn, q, slots, 1ull << 30);
  gpq_mpi_shim_set_device_samplers(!strcmp(argv[1], "device"));

  poly_mpi_t sk;
  he_ct_t ct, rotated, prod;
  poly_mpi_alloc(&sk);
  poly_mpi_alloc(&ct.c0); poly_mpi_alloc(&ct.c1); poly_mpi_alloc(&rotated.c0); poly_mpi_alloc(&rotated.c1); poly_mpi_alloc(&prod.c0); poly_mpi_alloc(&prod.c1);
  FILE *f = open_in("sk");
  read_poly(f, &sk, "sk");
  fclose(f);
  f = open_in("ct");
  read_poly(f, &ct.c0, "ct"); read_poly(f, &ct.c1, "ct");
  read_poly(f, &rotated.c0, "ct"); read_poly(f, &rotated.c1, "ct");
  fclose(f);
  ct.l = rotated.l = hectx.L; ct.nu = rotated.nu = hectx.Delta; ct.B = rotated.B = hectx.bnd.Bclean;

  const size_t words = (size_t)hectx.dimevk * polyctx.n;
  he_evk_t rlk, ck, *rk = malloc(slots * sizeof *rk);
  key_alloc(&rlk, words); key_alloc(&ck, words);
  for (unsigned k = 0; k < slots; k++) key_alloc(&rk[k], words);
  printf("call he_genrlk\n");
  he_genrlk(&rlk, &sk);
  printf("\ncall he_genck\n");
  he_genck(&ck, &sk);
  printf("\ncall he_genrk\n");
  he_genrk(rk, &sk);
  printf("\ninfo dimevk %u dim %u\n", hectx.dimevk, hectx.dim);

  char path[4096];
  snprintf(path, sizeof path, "%s/keys.bin", dir);
  FILE *o = fopen(path, "wb");
  if (!o) { perror(path); return 3; }
  key_write(o, &rlk, words); key_write(o, &ck, words);
  for (unsigned k = 0; k < slots; k++) key_write(o, &rk[k], words);
  fclose(o);

  he_rot(&rotated, rot, rk);
  dump("rot_c0", &rotated.c0); dump("rot_c1", &rotated.c1);
  he_mul(&prod, &ct, &ct, &rlk);
  dump("mul_c0", &prod.c0); dump("mul_c1", &prod.c1);
  printf("done\n");
  return 0;
}
