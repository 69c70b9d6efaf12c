/* gemv_host.c -- he_gemv / he_sum / he_idx (src/he-algo.c:47-113) through the reference's signatures with real libgcrypt MPIs, against the
 * reference's loop spelled here over the library's per-call he_copy_ct / he_rot / he_mulpt / he_add / he_rs.
 *
 *   gemv_host check <logn> <logq> <slots> <odd>   every coefficient, l, and the bits of nu and B equal; odd = 1: q = 2^logq - 1 (the fallback);
 *                                                 he_gemv also after a host-side edit of its operand (`poly stats` lines around that call)
 *   gemv_host gemvtime <logn> <logq> <slots>      wall time of he_gemv against the loop (conversions and copies included)
 *   gemv_host ref <path> <logn> <logq> <slots>    the same MPIs through the reference built into oracle/_ref/ (dlopen) and through this library;
 *                                                 `refonly <path> ..`: the reference alone; `ref - <ecd file> ..`: this library alone (see refmode)
 *
 * he_ecd is the host program's (src/he-encode.c:107-111); here a deterministic stand-in: both sides call it on the same vectors. */
#define _GNU_SOURCE            /* RTLD_DEEPBIND */
#include <complex.h>
#include <dlfcn.h>
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
void gcry_mpi_add_ui(MPI w, MPI u, unsigned long v);
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

static void (*ref_he_ecd)(struct he_pt *, const _Complex double *);
static struct ecd_rec *ecd_tab;                             /* mode `ref - <file>`: the reference's recorded plaintexts (below) */
static void ecd_lookup(struct he_pt *pt, const _Complex double *m);   /* mode `ref`: the reference's own encoder, for both sides */

/* the stand-in encoder: any deterministic function of the slot vector */
void he_ecd(struct he_pt *pt, const _Complex double *m)
{
  if (ecd_tab) { ecd_lookup(pt, m); return; }
  if (ref_he_ecd) {
    for (unsigned i = 0; i < polyctx.n; i++) gcry_mpi_set_ui(pt->m.coeffs[i], 0);   /* the reference's writes 2 slots coefficients of a fresh plaintext */
    ref_he_ecd(pt, m);
    return;
  }
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

static void poly_stats(const char *when)
{
  uint64_t confirmed = 0, changed = 0;
  gpq_mpi_shim_poly_stats(&confirmed, &changed);
  printf("poly stats %s: resident %u confirmed %llu changed %llu\n", when, gpq_mpi_shim_resident_polys(), (unsigned long long)confirmed, (unsigned long long)changed);
}

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
  /* one coefficient of c0 edited behind the library's back: where ct is resident the call starts from the kept copy, the recheck finds
   * the edit and the device work runs a second time on the integers as they are now */
  he_ct_t got2;
  ct_alloc(&got2);
  gcry_mpi_add_ui(ct.c0.coeffs[polyctx.n / 3], ct.c0.coeffs[polyctx.n / 3], 1);
  poly_stats("before the edited call");
  he_gemv(&got2, A, &ct, rk);
  poly_stats("after the edited call");
  ref_gemv(&want, A, &ct, rk);
  bad |= same(&got2, &want, "he_gemv after a host edit");
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

/* he_gemv / he_sum / he_idx of the reference itself (a build of `make -C oracle ref`, opened RTLD_LOCAL | RTLD_DEEPBIND: its own polyctx /
 * hectx, initialised by its own hectx_init) and of this library on the same MPIs and the same keys.  Each side prints a digest of every result.
 *   ref <path>          both sides, compared word for word; the diagonals are encoded by the REFERENCE's he_ecd on both sides
 *   refonly <path>      the reference alone, no device touched: its digests (`ref ..`) and, for every diagonal vector the calls encode, the
 *                       plaintext its he_ecd makes of it (`ecd <hash of the vector> <index:hex> ..`) -- how tests/golden/ref_hosts.json is written
 *   ref - <ecd file>    this library alone (a machine without the reference): he_ecd looks the vector up among the recorded `ecd` lines
 * Inputs and keys are functions of fixed seeds (keys: seeded residue slabs), so the reference's side needs no device. */
static uint64_t fnv_bytes(uint64_t h, const void *p, size_t bytes) { for (size_t i = 0; i < bytes; i++) { h ^= ((const unsigned char *)p)[i]; h *= 0x100000001b3ull; } return h; }
unsigned int gcry_mpi_aprint(int format, unsigned char **buffer, size_t *nwritten, const MPI a);
void gcry_free(void *p);
int gcry_mpi_cmp_ui(const MPI u, unsigned long v);
MPI gcry_mpi_set(MPI w, const MPI u);

static uint64_t ct_digest(const he_ct_t *a, unsigned n)
{
  uint64_t w[3] = {a->l, 0, 0};
  memcpy(&w[1], &a->nu, 8); memcpy(&w[2], &a->B, 8);
  uint64_t h = fnv_bytes(0xcbf29ce484222325ull, w, sizeof w);
  const poly_mpi_t *p[2] = {&a->c0, &a->c1};
  for (int c = 0; c < 2; c++)
    for (unsigned k = 0; k < n; k++) {
      unsigned char *t = NULL;
      gcry_mpi_aprint(4, &t, NULL, p[c]->coeffs[k]);
      h = fnv_bytes(h, t, strlen((char *)t) + 1);
      gcry_free(t);
    }
  return h;
}

/* recorded plaintexts of the reference's he_ecd, by the hash of the slot vector (mode `ref - <file>`) */
struct ecd_rec { uint64_t hash; unsigned count; unsigned *idx; char **hex; };
static unsigned ecd_count, ecd_slots, ecd_n;
static double ecd_delta;

static void ecd_lookup(struct he_pt *pt, const _Complex double *m)
{
  const uint64_t hash = fnv_bytes(0xcbf29ce484222325ull, m, ecd_slots * sizeof *m);
  for (unsigned r = 0; r < ecd_count; r++)
    if (ecd_tab[r].hash == hash) {
      for (unsigned i = 0; i < ecd_n; i++) gcry_mpi_set_ui(pt->m.coeffs[i], 0);
      for (unsigned k = 0; k < ecd_tab[r].count; k++) {
        MPI t = NULL;
        gcry_mpi_scan(&t, 4, ecd_tab[r].hex[k], 0, NULL);
        gcry_mpi_release(pt->m.coeffs[ecd_tab[r].idx[k]]);
        pt->m.coeffs[ecd_tab[r].idx[k]] = t;
      }
      pt->nu = ecd_delta;
      return;
    }
  fprintf(stderr, "he_ecd: a slot vector (hash %016llx) that the reference's record does not hold\n", (unsigned long long)hash);
  exit(3);
}

static int ecd_load(const char *file)
{
  FILE *f = fopen(file, "r");
  if (!f) return 1;
  static char line[1 << 16];
  while (fgets(line, sizeof line, f)) {
    if (strncmp(line, "ecd ", 4)) continue;
    ecd_tab = realloc(ecd_tab, (ecd_count + 1) * sizeof *ecd_tab);
    struct ecd_rec *r = &ecd_tab[ecd_count++];
    char *tok = strtok(line + 4, " \n");
    r->hash = strtoull(tok, NULL, 16); r->count = 0; r->idx = NULL; r->hex = NULL;
    while ((tok = strtok(NULL, " \n"))) {
      char *colon = strchr(tok, ':');
      if (!colon) return 1;
      r->idx = realloc(r->idx, (r->count + 1) * sizeof *r->idx); r->hex = realloc(r->hex, (r->count + 1) * sizeof *r->hex);
      r->idx[r->count] = (unsigned)strtoul(tok, NULL, 10); r->hex[r->count] = strdup(colon + 1); r->count++;
    }
  }
  fclose(f);
  return 0;
}

static int refmode(const char *path, const char *ecd_file, int with_lib, unsigned logn, unsigned logq, unsigned slots)
{
  const int have = strcmp(path, "-") != 0;
  if (!have && (!with_lib || !ecd_file || ecd_load(ecd_file))) { fprintf(stderr, "ref -: needs the file of recorded `ecd` lines\n"); return 2; }
  void *h = have ? dlopen(path, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND) : NULL;
  if (have && !h) { fprintf(stderr, "ref: cannot open %s: %s\n", path, dlerror()); return 2; }
#define SYM(name) (have ? dlsym(h, #name) : NULL)
  void (*r_hectx_init)(unsigned int, MPI, unsigned int, uint64_t) = SYM(hectx_init);
  void (*r_poly_mpi_alloc)(poly_mpi_t *) = SYM(poly_mpi_alloc);
  void (*r_he_gemv)(he_ct_t *, const _Complex double *, const he_ct_t *, const he_evk_t *) = SYM(he_gemv);
  void (*r_he_sum)(he_ct_t *, const he_ct_t *, const he_evk_t *) = SYM(he_sum);
  void (*r_he_idx)(he_ct_t *, const he_ct_t *, const unsigned int, const he_evk_t *) = SYM(he_idx);
  void (*r_he_ecd)(struct he_pt *, const _Complex double *) = SYM(he_ecd);
  struct he_ctx *r_hectx = SYM(hectx);
  struct poly_ctx *r_polyctx = SYM(polyctx);
#undef SYM
  if (have && (!r_hectx_init || !r_poly_mpi_alloc || !r_he_gemv || !r_he_sum || !r_he_idx || !r_he_ecd || !r_hectx || !r_polyctx || (void *)r_he_ecd == (void *)he_ecd)) {
    fprintf(stderr, "ref: symbols missing or not the reference's own\n"); return 2;
  }
  MPI q = gcry_mpi_new(0);
  gcry_mpi_set_ui(q, 1);
  gcry_mpi_lshift(q, q, logq);
  if (with_lib) hectx_init(logn, q, slots, 1ull << 30);       /* the bounds are hectx_init's: nothing overridden in this mode */
  if (have) r_hectx_init(logn, q, slots, 1ull << 30);
  const struct he_ctx *hx = with_lib ? &hectx : r_hectx;
  const struct poly_ctx *px = with_lib ? &polyctx : r_polyctx;
  const unsigned n = px->n;
  void (*palloc)(poly_mpi_t *) = with_lib ? poly_mpi_alloc : r_poly_mpi_alloc;
  ecd_slots = slots; ecd_n = n; ecd_delta = hx->Delta;
  if (have) ref_he_ecd = r_he_ecd;                            /* both sides encode with the reference's */
  const size_t words = (size_t)hx->dimevk * n;
  he_evk_t *keys = calloc(slots, sizeof *keys);              /* rk[0..slots): seeded residues of each prime */
  for (unsigned k = 0; k < slots; k++) {
    keys[k].p0.coeffs = malloc(words * 8); keys[k].p1.coeffs = malloc(words * 8);
    uint64_t ks = 8800 + k;
    const struct rns_ctx *r = px->rns;
    for (unsigned d = 0; d < hx->dimevk; d++, r = r->next)
      for (unsigned i = 0; i < n; i++) { keys[k].p0.coeffs[(size_t)d * n + i] = splitmix64(&ks) % r->p; keys[k].p1.coeffs[(size_t)d * n + i] = splitmix64(&ks) % r->p; }
  }
  he_ct_t src, got, want, x, y;
  he_ct_t *all[5] = {&src, &got, &want, &x, &y};
  for (int i = 0; i < 5; i++) { palloc(&all[i]->c0); palloc(&all[i]->c1); }
  src.l = hx->L; src.nu = hx->Delta * 3.5; src.B = 17.25;
  MPI qh = gcry_mpi_new(0);
  gcry_mpi_set_ui(qh, 1);
  gcry_mpi_lshift(qh, qh, logq - 1);
  uint64_t s2 = 444;
  for (unsigned i = 0; i < n; i++) {                          /* centred uniform mod q_L */
    uniform_mod(src.c0.coeffs[i], q, &s2);
    uniform_mod(src.c1.coeffs[i], q, &s2);
    if (gcry_mpi_cmp(src.c0.coeffs[i], qh) >= 0) gcry_mpi_sub(src.c0.coeffs[i], src.c0.coeffs[i], q);
    if (gcry_mpi_cmp(src.c1.coeffs[i], qh) >= 0) gcry_mpi_sub(src.c1.coeffs[i], src.c1.coeffs[i], q);
  }
  _Complex double *A = matrix(slots, 5), *S = calloc((size_t)slots * slots, sizeof *S);
  for (size_t i = 0; i < (size_t)slots * slots; i++) A[i] /= 8.0;
  const unsigned idxs[3] = {0, 5 % slots, slots - 1};
  if (!with_lib) {                                            /* the record of he_ecd: every diagonal vector of every matrix below (zrotdiag, src/he-algo.c:29-43) */
    unsigned n1 = (unsigned)sqrt(slots);
    if (slots != n1 * n1) n1 = (unsigned)sqrt(2 * slots);
    he_pt_t pt;
    palloc(&pt.m);
    _Complex double *rd = malloc(slots * sizeof *rd);
    for (int mtx = 0; mtx < 5; mtx++) {
      memset(S, 0, (size_t)slots * slots * sizeof *S);
      if (mtx == 1) for (unsigned i = 0; i < slots; i++) S[i] = 1;
      if (mtx >= 2) S[idxs[mtx - 2] * slots + idxs[mtx - 2]] = 1;
      const _Complex double *M = mtx ? S : A;
      for (unsigned d = 0; d < slots; d++) {
        const int shift = (int)(d / n1 * n1);
        for (unsigned k = 0; k < slots; k++) { int r = ((int)k - shift) % (int)slots; if (r < 0) r += (int)slots; rd[k] = M[(r % slots) * slots + (d + r) % slots]; }
        for (unsigned i = 0; i < n; i++) gcry_mpi_set_ui(pt.m.coeffs[i], 0);
        r_he_ecd(&pt, rd);
        printf("ecd %016llx", (unsigned long long)fnv_bytes(0xcbf29ce484222325ull, rd, slots * sizeof *rd));
        for (unsigned i = 0; i < n; i++)
          if (gcry_mpi_cmp_ui(pt.m.coeffs[i], 0)) { unsigned char *t = NULL; gcry_mpi_aprint(4, &t, NULL, pt.m.coeffs[i]); printf(" %u:%s", i, (char *)t); gcry_free(t); }
        printf("\n");
      }
    }
  }
  int bad = 0;
#define BOTH(what, dl, dr, lib_call, ref_call) do { \
    if (with_lib) { lib_call; printf("lib %s %016llx\n", what, (unsigned long long)ct_digest(dl, n)); } \
    if (have) { ref_call; printf("ref %s %016llx\n", what, (unsigned long long)ct_digest(dr, n)); } \
    if (with_lib && have) bad |= same(dl, dr, what); } while (0)
  BOTH("he_gemv", &got, &want, he_gemv(&got, A, &src, keys), r_he_gemv(&want, A, &src, keys));
  BOTH("he_sum", &got, &want, he_sum(&got, &src, keys), r_he_sum(&want, &src, keys));
  for (int t = 0; t < 3; t++) {
    char name[32];
    snprintf(name, sizeof name, "he_idx %u", idxs[t]);
    BOTH(name, &got, &want, he_idx(&got, &src, idxs[t], keys), r_he_idx(&want, &src, idxs[t], keys));
  }
  for (unsigned i = 0; i < n; i++) {                          /* ct_dest == ct */
    gcry_mpi_set(x.c0.coeffs[i], src.c0.coeffs[i]); gcry_mpi_set(x.c1.coeffs[i], src.c1.coeffs[i]);
    gcry_mpi_set(y.c0.coeffs[i], src.c0.coeffs[i]); gcry_mpi_set(y.c1.coeffs[i], src.c1.coeffs[i]);
  }
  x.l = y.l = src.l; x.nu = y.nu = src.nu; x.B = y.B = src.B;
  BOTH("he_gemv in place", &x, &y, he_gemv(&x, A, &x, keys), r_he_gemv(&y, A, &y, keys));
#undef BOTH
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
  if (argc >= 7 && !strcmp(argv[1], "ref") && !strcmp(argv[2], "-")) return refmode("-", argv[3], 1, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
  if (argc >= 6 && (!strcmp(argv[1], "ref") || !strcmp(argv[1], "refonly"))) return refmode(argv[2], NULL, !strcmp(argv[1], "ref"), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
  if (argc >= 5 && !strcmp(argv[1], "gemvtime")) {
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0);
    return gemvtime(atoi(argv[4]));
  }
  fprintf(stderr, "usage: gemv_host check <logn> <logq> <slots> <odd> | gemvtime <logn> <logq> <slots> | ref <path> <logn> <logq> <slots>\n");
  return 2;
}
