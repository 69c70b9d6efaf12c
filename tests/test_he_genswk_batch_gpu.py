"""gpq_he_genswk_batch: `count` switching keys per call (src/he-kem.c:74-118 per key) through the CRT split of P 2^k.

Words against the Python-integer model (tests/genswk_model.py) in all hidden forms, at the word edges of k and one word above the least
W; the model's window inputs (every number of additions of P, the centring bit of h, the compare-and-subtract of the raw p1, carries over
every word boundary of P hs); a product that wraps the dimmul-limb basis; the existing one-key path at n = 2^13 across launch groups;
keys from the caller's bytes; keys that key-switch; every refusal, and a stream capture."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import big_to_ints, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref
from tests import enc_model
from tests import genswk_model as gm

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A


def _shape(engine_ctx, oracle_ctx, logn, k):
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 20).he_dims(k, k)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    primes = [int(p) for p in o.p]
    P = gm.product_of(primes[:dimP])
    dimmul = gm.dimmul_of(P, k, logn)
    assert g.he_genswk_dimmul(dimP, k) == dimmul and dimmul <= dimevk
    return g, o, primes, P, dimP, dimevk, dimmul, gm.nbits_of(P, k) // 64 + 1


def _evk_slab(o, poly, dimevk):
    """rns_decompose + ntt per limb, src/he-kem.c:103-110"""
    return o.ntt_slab(np.array([v % o.p[d] for d in range(dimevk) for v in poly], dtype=np.uint64), dimevk)


def _big(polys, W):
    return to_device(np.concatenate([ints_to_big(p, W).reshape(-1) for p in polys]))


def _small(polys):
    return torch.from_numpy(np.array(polys, dtype=np.int8).reshape(-1)).cuda()


def _sk_ntt(g, sk, W, dimmul):
    out = torch.empty(dimmul * g.n, dtype=torch.int64, device="cuda")
    assert g.lib.gpq_evk_pack(g.h, g._ptr(out), g._ptr(_big([sk], W)), W, dimmul, 1, g._stream()) == 0
    return out


def _keys(g, dimevk, count):
    return [torch.full((count * dimevk * g.n,), PATTERN, dtype=torch.int64, device="cuda") for _ in range(2)]


def _check(g, o, primes, P, k, dimP, dimevk, dimmul, W, p1s, es, sk, sps, galois=None, Wsp=0, sk_small=None):
    """one call for len(p1s) keys against the model key by key; sps = the hidden polynomials the model takes"""
    count, n = len(p1s), g.n
    evk0, evk1 = _keys(g, dimevk, count)
    kw = dict(sk_small=_small([sk if sk_small is None else sk_small]), galois=galois) if galois is not None else dict(sp=_big(sps, Wsp), Wsp=Wsp)
    g.he_genswk_batch(evk0, evk1, _big(p1s, W), _small(es), _sk_ntt(g, sk, W, dimmul), W, dimP, k, dimevk, **kw)
    got0, got1 = to_host(evk0).reshape(count, -1), to_host(evk1).reshape(count, -1)
    for j in range(count):
        w0, w1 = gm.genswk(P, k, primes, p1s[j], es[j], sps[j], sk, dimmul, dimevk)
        assert np.array_equal(got1[j], _evk_slab(o, w1, dimevk)), "key %d: swk.p1 differs" % j
        assert np.array_equal(got0[j], _evk_slab(o, w0, dimevk)), "key %d: swk.p0 differs" % j


@pytest.mark.parametrize("logn,k", [(7, 1), (7, 63), (7, 64), (7, 65), (7, 120), (7, 128), (8, 200)])
def test_words_against_the_model(engine_ctx, oracle_ctx, logn, k):
    g, o, primes, P, dimP, dimevk, dimmul, W = _shape(engine_ctx, oracle_ctx, logn, k)
    n, rng = g.n, random.Random(100 * logn + k)
    sk = [rng.choice((-1, 0, 1)) for _ in range(n)]
    p1s = [[rng.randrange(1 << gm.nbits_of(P, k)) for _ in range(n)] for _ in range(3)]
    es = [[rng.randrange(-11, 12) for _ in range(n)] for _ in range(3)]
    args = (g, o, primes, P, k, dimP, dimevk, dimmul)
    # big slabs: s^2 centred mod q_L (he_genrlk, src/he-kem.c:130), a dense k-bit polynomial, a ternary one in one word
    s2 = gm.poly_mul(primes, sk, sk, (k + 1) // 59 + 1, 1 << k)
    dense = [rng.randrange(-(1 << (k - 1)), 1 << (k - 1)) for _ in range(n)]
    _check(*args, W, p1s, es, sk, [s2, dense, s2], Wsp=k // 64 + 1)
    _check(*args, W, p1s[:1], es[:1], sk, [gm.galois_image(sk, 5)], Wsp=1)
    # rotations: rot = 0, a repeated rot, rot >= n/2; conjugation
    gs = [1, pow(5, n // 2 + 3, 1 << 64), pow(5, n // 2 + 3, 1 << 64)]
    _check(*args, W, p1s, es, sk, [gm.galois_image(sk, v) for v in gs], galois=gs)
    gs = [2 * n - 1, 5, 2 * n - 1]
    _check(*args, W, p1s, es, sk, [gm.galois_image(sk, v) for v in gs], galois=gs)
    # one word above the least
    _check(*args, W + 1, p1s, es, sk, [gm.galois_image(sk, v) for v in gs], galois=gs)
    _check(*args, W + 1, p1s[:2], es[:2], sk, [dense, s2], Wsp=k // 64 + 2)


@pytest.mark.parametrize("k", [63, 64, 65, 128])
def test_window_inputs_through_the_call(engine_ctx, oracle_ctx, k):
    """tests/test_genswk_model.py counts the windows of these inputs; here they go through the device, in both hidden forms"""
    g, o, primes, P, dimP, dimevk, dimmul, W = _shape(engine_ctx, oracle_ctx, 7, k)
    n = g.n
    one = [1] + [0] * (n - 1)
    p1, e, sp = gm.window_inputs(P, k, n)
    stats = {}
    gm.structured(P, k, primes, p1, e, sp, one, dimmul, stats=stats)
    assert not gm.windows_missing(P, k, stats, p1)
    _check(g, o, primes, P, k, dimP, dimevk, dimmul, W, [p1], [e], one, [sp], Wsp=k // 64 + 1)
    p1, e, sp = gm.window_inputs(P, k, n, sp=one)
    _check(g, o, primes, P, k, dimP, dimevk, dimmul, W, [p1, p1], [e, e], one, [one, one], galois=[1, 5])


def test_product_that_wraps_the_basis(engine_ctx, oracle_ctx):
    """sk_ntt is any slab: with |coefficients| up to 2^20 the exact product p1 sk leaves (-P'/2, P'/2) and the key follows the value
    centred mod P', as poly_rns2mpi does"""
    logn, k = 7, 105
    g, o, primes, P, dimP, dimevk, dimmul, W = _shape(engine_ctx, oracle_ctx, logn, k)
    n, rng = g.n, random.Random(3)
    sk = [rng.randrange(-(1 << 20), (1 << 20) + 1) for _ in range(n)]
    p1s = [[rng.randrange(1 << gm.nbits_of(P, k)) for _ in range(n)] for _ in range(2)]
    es = [[rng.randrange(-11, 12) for _ in range(n)] for _ in range(2)]
    Pp = gm.product_of(primes[:dimmul])
    assert all(any(abs(v) > Pp // 2 for v in gm.negacyclic(p1, sk)) for p1 in p1s)
    tern = [rng.choice((-1, 0, 1)) for _ in range(n)]
    _check(g, o, primes, P, k, dimP, dimevk, dimmul, W, p1s, es, sk, [gm.galois_image(tern, 5), gm.galois_image(tern, 2 * n - 1)], galois=[5, 2 * n - 1],
           sk_small=tern)
    sps = [[rng.randrange(-(1 << (k - 1)), 1 << (k - 1)) for _ in range(n)] for _ in range(2)]
    _check(g, o, primes, P, k, dimP, dimevk, dimmul, W, p1s, es, sk, sps, Wsp=k // 64 + 1)


def test_against_the_one_key_path_across_launch_groups(engine_ctx, oracle_ctx):
    """n = 2^13, logqL = 438, 5 rotation keys in groups of 2 (an odd remainder group) and in one group of 32: each key is gpq_he_genswk's
    on the same polynomials (gpq_small_to_big of e, gpq_poly_rot of the secret as sp)"""
    logn, k, count = 13, 438, 5
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 20).he_dims(k, k)
    g = engine_ctx(logn, dimevk)
    n = g.n
    dimmul = g.he_genswk_dimmul(dimP, k)
    nbits = gm.nbits_of(gm.product_of(g.p[:dimP]), k)
    W = nbits // 64 + 1
    rng = np.random.default_rng(13)
    sk = np.zeros(n, dtype=np.int8)
    sk[rng.choice(n, 64, replace=False)] = rng.choice(np.array([-1, 1], dtype=np.int8), 64)
    sk_small = torch.from_numpy(sk).cuda()
    sk_big = g.small_to_big(torch.empty(W * n, dtype=torch.int64, device="cuda"), sk_small, W)
    p1 = g.sample_uniform(torch.empty(count * W * n, dtype=torch.int64, device="cuda"),
                          torch.from_numpy(rng.integers(0, 256, count * n * (nbits // 8 + 1), dtype=np.uint8)).cuda(), nbits, W)
    e = g.sample_error(torch.empty(count * n, dtype=torch.int8, device="cuda"), torch.from_numpy(rng.integers(0, 256, count * n, dtype=np.uint8)).cuda())
    e_big = g.small_to_big(torch.empty(count * W * n, dtype=torch.int64, device="cuda"), e, W)
    rots = [0, 1, 4097, 1, 77]
    want = []
    for j, rot in enumerate(rots):
        sp = g.poly_rot(torch.empty_like(sk_big), sk_big, W, rot)
        k0, k1 = (torch.empty(dimevk * n, dtype=torch.int64, device="cuda") for _ in range(2))
        g.he_genswk(k0, k1, p1[j * W * n:(j + 1) * W * n], sk_big, e_big[j * W * n:(j + 1) * W * n], sp, W, dimP, k, dimevk)
        want.append((k0, k1))
    sk_ntt = torch.empty(dimmul * n, dtype=torch.int64, device="cuda")
    assert g.lib.gpq_evk_pack(g.h, g._ptr(sk_ntt), g._ptr(sk_big), W, dimmul, 1, g._stream()) == 0
    try:
        for chunk in (2, 32):
            g.set_chunk(chunk)
            evk0, evk1 = _keys(g, dimevk, count)
            g.he_genswk_batch(evk0, evk1, p1, e, sk_ntt, W, dimP, k, dimevk, sk_small=sk_small, galois=[pow(5, r, 1 << 64) for r in rots])
            for j in range(count):
                assert torch.equal(evk0[j * dimevk * n:(j + 1) * dimevk * n], want[j][0]), "chunk %d, key %d: swk.p0" % (chunk, j)
                assert torch.equal(evk1[j * dimevk * n:(j + 1) * dimevk * n], want[j][1]), "chunk %d, key %d: swk.p1" % (chunk, j)
    finally:
        g.set_chunk(32)
    assert not torch.equal(want[0][0], want[1][0])


@pytest.mark.parametrize("k", [63, 120])
def test_keys_from_the_callers_bytes(engine_ctx, oracle_ctx, k):
    """one byte stream e_0, u_0, e_1, u_1, ... through gpq_sample_error / gpq_sample_uniform(nbits) into the call, against the model fed by
    enc_model's samplers on the same bytes"""
    g, o, primes, P, dimP, dimevk, dimmul, W = _shape(engine_ctx, oracle_ctx, 7, k)
    n, count, nbits = g.n, 3, gm.nbits_of(P, k)
    nb = nbits // 8 + 1
    rng = np.random.default_rng(k)
    stream = rng.integers(0, 256, count * (n + n * nb), dtype=np.uint8)
    dev = torch.from_numpy(stream).cuda()
    sk = [int(v) for v in rng.integers(-1, 2, n)]
    e, p1 = torch.empty(count * n, dtype=torch.int8, device="cuda"), torch.empty(count * W * n, dtype=torch.int64, device="cuda")
    s, p1s, es = enc_model.Stream(stream), [], []
    for j in range(count):
        at = j * (n + n * nb)
        g.sample_error(e[j * n:(j + 1) * n], dev[at:at + n])
        g.sample_uniform(p1[j * W * n:(j + 1) * W * n], dev[at + n:at + n + n * nb], nbits, W)
        es.append([int(v) for v in enc_model.sample_error(s, n)])
        p1s.append(enc_model.sample_uniform(s, n, P << k))
    assert s.pos == stream.size
    gs = [5, 2 * n - 1, pow(5, 9, 1 << 64)]
    evk0, evk1 = _keys(g, dimevk, count)
    g.he_genswk_batch(evk0, evk1, p1, e, _sk_ntt(g, sk, W, dimmul), W, dimP, k, dimevk, sk_small=_small([sk]), galois=gs)
    got0, got1 = to_host(evk0).reshape(count, -1), to_host(evk1).reshape(count, -1)
    for j in range(count):
        w0, w1 = gm.genswk(P, k, primes, p1s[j], es[j], gm.galois_image(sk, gs[j]), sk, dimmul, dimevk)
        assert np.array_equal(got0[j], _evk_slab(o, w0, dimevk)) and np.array_equal(got1[j], _evk_slab(o, w1, dimevk)), "key %d" % j


def _sparse_negacyclic(dense, terms, n):
    out = [0] * n
    for t, c in terms:
        for i, v in enumerate(dense):
            j = i + t
            if j < n:
                out[j] += c * v
            else:
                out[j - n] -= c * v
    return out


def test_rotation_and_conjugation_keys_switch_keys(engine_ctx, oracle_ctx):
    """the construction and the bound of test_rotate_and_conjugate_decrypt_to_the_permuted_message (tests/test_ckks_roundtrip_gpu.py) at
    n = 2^13 with the keys made by the batch call: he_rot / he_conj decrypt under s to the permuted message within 2^30 at scale 2^40"""
    logn, logq = 13, 438
    n, q = 1 << logn, 1 << logq
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 20).he_dims(logq, logq)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    rng = random.Random(99 + logn)
    nprng = np.random.default_rng(5)
    dimmul = g.he_genswk_dimmul(dimP, logq)
    nbits = gm.nbits_of(gm.product_of(o.p[:dimP]), logq)
    Wk = nbits // 64 + 1
    sparse = lambda cnt, draw: sorted({rng.randrange(n): draw() for _ in range(cnt)}.items())
    s_terms = sparse(24, lambda: rng.choice((-1, 1)))
    s = [0] * n
    for t, c in s_terms:
        s[t] = c
    perms = [("rot3", lambda a: ref.poly_rot(a, 3), pow(5, 3, 1 << 64)), ("conj", ref.poly_conj, 2 * n - 1)]
    count = len(perms)
    p1 = g.sample_uniform(torch.empty(count * Wk * n, dtype=torch.int64, device="cuda"),
                          torch.from_numpy(nprng.integers(0, 256, count * n * (nbits // 8 + 1), dtype=np.uint8)).cuda(), nbits, Wk)
    e = g.sample_error(torch.empty(count * n, dtype=torch.int8, device="cuda"), torch.from_numpy(nprng.integers(0, 256, count * n, dtype=np.uint8)).cuda())
    evk0, evk1 = _keys(g, dimevk, count)
    g.he_genswk_batch(evk0, evk1, p1, e, _sk_ntt(g, s, Wk, dimmul), Wk, dimP, logq, dimevk, sk_small=_small([s]), galois=[p[2] for p in perms])
    a_terms = sparse(6, lambda: rng.randrange(q))
    a = [0] * n
    for t, c in a_terms:
        a[t] += c
    m = [rng.randrange(-1000, 1001) << 40 for _ in range(n)]
    c0 = [ref.centred_mod(-x + mm + rng.randrange(-8, 9), q) for x, mm in zip(_sparse_negacyclic(s, a_terms, n), m)]
    c1 = [ref.centred_mod(v, q) for v in a]
    W = logq // 64 + 1
    d0, d1 = to_device(ints_to_big(c0, W)), to_device(ints_to_big(c1, W))
    for j, (which, perm, _) in enumerate(perms):
        r0, r1 = torch.empty_like(d0), torch.empty_like(d0)
        if which == "conj":
            g.poly_conj(r0, d0, W); g.poly_conj(r1, d1, W)
        else:
            g.poly_rot(r0, d0, W, 3); g.poly_rot(r1, d1, W, 3)
        o0, o1 = torch.empty_like(d0), torch.empty_like(d0)
        per = dimevk * n
        g.he_swk(o0, o1, r0, r1, evk0[j * per:(j + 1) * per], evk1[j * per:(j + 1) * per], W, logq, dimB, dimP)
        k0, k1 = big_to_ints(to_host(o0), W, n)[0], big_to_ints(to_host(o1), W, n)[0]
        got = [ref.centred_mod(x + y, q) for x, y in zip(k0, _sparse_negacyclic(k1, s_terms, n))]
        assert max(abs(x - y) for x, y in zip(got, perm(m))) < 1 << 30, which


def test_refusals_and_capture(engine_ctx, oracle_ctx):
    logn, k = 7, 120
    g, o, primes, P, dimP, dimevk, dimmul, W = _shape(engine_ctx, oracle_ctx, logn, k)
    n, count, rng = g.n, 2, random.Random(8)
    sk = [rng.choice((-1, 0, 1)) for _ in range(n)]
    p1 = _big([[rng.randrange(1 << gm.nbits_of(P, k)) for _ in range(n)] for _ in range(count)], W)
    e = _small([[rng.randrange(-11, 12) for _ in range(n)] for _ in range(count)])
    sk_ntt, sk_small = _sk_ntt(g, sk, W, dimmul), _small([sk])
    sp = _big([sk, sk], 1)
    evk0, evk1 = _keys(g, dimevk, count)
    ws = torch.empty(g.lib.gpq_he_genswk_batch_workspace_bytes(g.h, W, dimP, k, dimevk, count) // 8 + 8, dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    gal = lambda *v: (C.c_uint64 * len(v))(*v)
    good = dict(h=g.h, evk0=evk0, evk1=evk1, p1=p1, e=e, sk_ntt=sk_ntt, sk_small=sk_small, galois=gal(5, 2 * n - 1), sp=None, Wsp=0, W=W, dimP=dimP, k=k,
                dimevk=dimevk, count=count, ws=ws)

    def call(**over):
        a = dict(good, **over)
        return g.lib.gpq_he_genswk_batch(a["h"], p(a["evk0"]), p(a["evk1"]), p(a["p1"]), p(a["e"]), p(a["sk_ntt"]), p(a["sk_small"]), a["galois"], p(a["sp"]),
                                         a["Wsp"], a["W"], a["dimP"], a["k"], a["dimevk"], a["count"], p(a["ws"]), g._stream())

    few = engine_ctx(logn, 3)                                        # three primes: dimP fits, the product's dimmul limbs do not
    torch.cuda.synchronize()
    g.profile(True)
    few.profile(True)
    try:
        assert call(h=None) == -1
        for name in ("evk0", "evk1", "p1", "e", "sk_ntt", "ws"):
            assert call(**{name: None}) == -1, name
        assert call(sk_small=None) == -1                                 # galois without the secret
        assert call(galois=None) == -1                                   # neither form
        assert call(galois=None, sp=sp, Wsp=0) == -1
        assert call(galois=gal(5, 6)) == -1                              # an even g
        assert call(k=0) == -1 and call(count=0) == -1
        assert call(W=W - 1) == -1                                       # 64 W <= bits of P q_L
        assert call(dimevk=g.nprimes + 1) == -1 and call(dimevk=0) == -1
        assert call(dimP=g.nprimes + 1) == -1 and call(dimP=0) == -1
        assert call(h=few.h, dimevk=1) == -1                             # dimmul the context lacks
        assert call(evk1=evk0) == -1 and call(evk0=p1) == -1 and call(evk1=sk_ntt) == -1
        assert call(evk0=e.view(torch.int64)) == -1 and call(evk1=sk_small.view(torch.int64)) == -1
        assert call(galois=None, sp=evk0, Wsp=1) == -1
        assert call(ws=evk0) == -1 and call(ws=p1) == -1
        assert call(W=33) == -3                                          # where gpq_he_genswk is unsupported
        assert g.lib.gpq_he_genswk_batch_workspace_bytes(g.h, W - 1, dimP, k, dimevk, count) == 0
        assert g.lib.gpq_he_genswk_dimmul(g.h, dimP, 0) == 0 and g.lib.gpq_he_genswk_dimmul(g.h, g.nprimes + 1, k) == 0
        if torch.cuda.device_count() > 1:                               # the wrong current device
            with torch.cuda.device(1):
                assert call() == -1
        assert g.profile_collect() == {} and few.profile_collect() == {}   # nothing was launched
    finally:
        g.profile(False)
        few.profile(False)
    torch.cuda.synchronize()
    assert bool((evk0 == evk0[0]).all()) and bool((evk1 == evk0[0]).all())
    # the constants are the context's: built once per (dimP, logqL), counted, not uploaded per call
    before = g.debug_table_bytes(0)
    assert call() == 0
    torch.cuda.synchronize()
    assert g.debug_table_bytes(0) == before
    g.profile(True)
    try:
        assert call() == 0
        assert "genswk_crt_tail" in g.profile_collect()
    finally:
        g.profile(False)
    eager0, eager1 = evk0.clone(), evk1.clone()
    evk0.fill_(PATTERN)
    evk1.fill_(PATTERN)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call() == 0
    evk0.fill_(PATTERN)
    evk1.fill_(PATTERN)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(evk0, eager0) and torch.equal(evk1, eager1) and bool((eager0 != eager0[0]).any())


def test_constants_are_counted_once(engine_ctx):
    import gpqhe_amd
    g = gpqhe_amd.PolyContext(7, 8)
    try:
        dimP, k = 2, 64
        g.he_genswk_dimmul(dimP, k)                                    # builds the basis of dimP limbs and the constants
        before = g.debug_table_bytes(0)
        g.he_genswk_dimmul(dimP, k)
        assert g.debug_table_bytes(0) == before
        g.he_genswk_dimmul(dimP, k + 1)                                # another pair: P, P^-1 mod 2^(64 W2), M, floor(M/2), M + floor(M/2)
        P = gm.product_of(g.p[:dimP])
        words = lambda v: (v.bit_length() + 63) // 64
        assert g.debug_table_bytes(0) - before == (words(P) + (k + 1 + 63) // 64 + 3 * words(3 * (P << k))) * 8
    finally:
        torch.cuda.synchronize()
        g.close()
