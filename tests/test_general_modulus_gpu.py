"""The general-modulus entry points (include/gpqhe_hip.h, "general moduli") against Python integers.

Every one of them ends in bridge_smod_general, a multiword Barrett reduction (HAC 14.42) whose constants launch_smod_general
computes on the host.  The inputs here are built to land where that reduction and the roundings around it can go wrong: on
k*q + floor(q/2) and its neighbours, on multiples of q, on the most negative value a basis or a word count admits, on moduli
of a special shape (1, 2^(64k), 2^(64k) +- 1, 3*2^64, the widest modulus check_modulus accepts) and on Delta at the top of the
word.  The expected words always come from oracle/bigint_ref.py (mpi_smod, mpi_rdiv, he_relin_tail, he_mulpt, he_mul, he_swk);
where a power-of-two entry point computes the same thing it is compared as well, never instead."""
import random

import numpy as np
import pytest

from gpqhe_amd import to_device, to_host
from oracle import bigint_ref as ref
from oracle.expect import ints_to_words, words_to_ints
from tests.he_anchors import group_ends

pytestmark = pytest.mark.gpu

B = 1 << 64
ODD_1000 = 1000003 ** 50                 # odd, 997 bits (16 words)
ODD_48W = 1000003 ** 154                 # odd, 3070 bits: 48 words, the most check_modulus accepts
MODULI = [("1", 1), ("2", 2), ("3", 3), ("2^61", 1 << 61), ("2^64-1", B - 1), ("2^64", B), ("2^64+1", B + 1), ("3*2^64", 3 * B),
          ("2^128-1", B * B - 1), ("2^128", B * B), ("2^128+1", B * B + 1), ("2^192", B ** 3), ("odd997", ODD_1000),
          ("odd48w", ODD_48W), ("2^3008", B ** 47)]


def _torch():
    import torch
    return torch


def _words(q):
    return max(1, (q.bit_length() + 63) // 64)


def _big(polys, W):
    """lists of signed ints per polynomial -> device big slab [polys][W][n]"""
    return to_device(np.concatenate([ints_to_words(p, W) for p in polys]))


def _ints(t, W, n):
    """device big slab -> lists of signed ints per polynomial"""
    h = to_host(t).reshape(-1, W * n)
    return [words_to_ints(row, W, n) for row in h]


def _residues(polys, primes):
    """the RNS slab [polys][dim][n] of known integers: x mod p_d written on the host, so the CRT value is x itself"""
    return to_device(np.array([v % p for xs in polys for p in primes for v in xs], dtype=np.uint64))


def _crt_columns(rng, q, P, n):
    """centred CRT values for a basis of product P: the corners of mpi_smod(., q) at several multiples of q, 0, +-(floor(P/2) - 1)
    and the most negative value the basis admits (floor(P/2) - P); random values in between.  Shuffled: each polynomial of a batch
    has the corners on other coefficients."""
    lo, hi = P // 2 - P, P // 2 - 1
    h = q // 2
    kmax = (hi - h - 1) // q
    assert kmax >= 2, "the basis must admit several multiples of q"
    cols = []
    for k in sorted({0, 1, 2, kmax, rng.randrange(1, kmax + 1)}):
        for v in (k * q + h - 1, k * q + h, k * q + h + 1, k * q, k * q - 1):
            cols += [v, -v]
    cols += [0, hi - 1, -(hi - 1), lo, hi]
    cols = [c for c in cols if lo <= c <= hi]
    cols += [rng.randint(lo, hi) for _ in range(n - len(cols))]
    rng.shuffle(cols)
    return cols


def _basis_dim(q):
    return (q.bit_length() + 64) // 59 + 2           # P above q * 2^60: many multiples of q below floor(P/2)


# ---------------------------------------------------------------------------
# (a) gpq_rns_reconstruct_general on built CRT values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("q", [q for _, q in MODULI], ids=[name for name, _ in MODULI])
def test_rns_reconstruct_general_on_built_crt_values(engine_ctx, q):
    """poly_rns2mpi (src/poly.c:109-120) = mpi_smod(x, q) of the centred CRT value x, for Wout = L, Wout > L (the sign-fill
    words) and q passed with zero top words (Lq > L); batch 3, other corners in every polynomial."""
    torch = _torch()
    g = engine_ctx(7, 56)
    n, L, dim = g.n, _words(q), _basis_dim(q)
    assert dim <= 56
    P = ref.RnsBasis(g.p[:dim]).P
    rng = random.Random(q % 1000003 + q.bit_length())
    polys = [_crt_columns(rng, q, P, n) for _ in range(3)]
    exp = [[ref.mpi_smod(x, q) for x in xs] for xs in polys]
    slab = _residues(polys, g.p[:dim])
    for Wout, Lq in ((L, None), (L + 2, None), (L + 1, L + 2)):
        if Lq and Lq > 48:
            Lq = 48 if 48 > L else None              # the widest modulus has no room for zero top words
        out = torch.full((3 * Wout * n,), 0x5A5A, dtype=torch.int64, device="cuda")
        g.rns_reconstruct_general(out, Wout, slab, dim, q, Lq)
        got = _ints(out, Wout, n)
        for k in range(3):
            bad = [i for i in range(n) if got[k][i] != exp[k][i]]
            assert not bad, "q=%#x Wout=%d Lq=%s poly %d: %d coefficients differ, first x=%d gave %d, want %d" % (
                q, Wout, Lq, k, len(bad), polys[k][bad[0]], got[k][bad[0]], exp[k][bad[0]])


@pytest.mark.parametrize("q", [ODD_1000 >> 800 | 1, B * B], ids=["odd197", "2^128"])
def test_rns_reconstruct_general_at_n_2_16(engine_ctx, q):
    """the kernel's coefficient and polynomial indices at n = 2^16, batch 3: corners at both ends of every polynomial"""
    torch = _torch()
    g = engine_ctx(16, 45)
    n, L, dim = g.n, _words(q), _basis_dim(q)
    P = ref.RnsBasis(g.p[:dim]).P
    rng = random.Random(16 + L)
    polys = []
    for _ in range(3):
        edges = _crt_columns(rng, q, P, 64)
        polys.append(edges + [rng.randint(P // 2 - P, P // 2 - 1) for _ in range(n - 128)] + edges[::-1])
    out = torch.empty(3 * (L + 1) * n, dtype=torch.int64, device="cuda")
    g.rns_reconstruct_general(out, L + 1, _residues(polys, g.p[:dim]), dim, q)
    got = _ints(out, L + 1, n)
    for k in range(3):
        assert got[k] == [ref.mpi_smod(x, q) for x in polys[k]], "polynomial %d" % k


# ---------------------------------------------------------------------------
# (b) q = 2^k through the general entry points gives the tuned power-of-two entry points' words
# ---------------------------------------------------------------------------
POW2 = [1, 61, 63, 64, 65, 127, 128, 129, 192]


@pytest.mark.parametrize("k", POW2)
def test_general_equals_power_of_two_path(engine_ctx, oracle_ctx, k):
    """q = 2^k: gpq_rns_reconstruct_general, gpq_he_rs_general (Delta = 2^s) and gpq_he_mul_general give the words of
    gpq_rns_reconstruct, gpq_he_rs and gpq_he_mul, and those words are the restated reference's"""
    torch = _torch()
    q = 1 << k
    # rns_reconstruct
    g = engine_ctx(7, 12)
    n, W, dim = g.n, k // 64 + 1, 6                  # the words of q = 2^k itself: check_modulus wants Wout >= them
    P = ref.RnsBasis(g.p[:dim]).P
    rng = random.Random(k)
    polys = [_crt_columns(rng, q, P, n) for _ in range(3)]
    slab = _residues(polys, g.p[:dim])
    a, b = torch.empty(3 * W * n, dtype=torch.int64, device="cuda"), torch.empty(3 * W * n, dtype=torch.int64, device="cuda")
    g.rns_reconstruct(a, W, slab, dim, k)
    g.rns_reconstruct_general(b, W, slab, dim, q)
    assert _ints(a, W, n) == [[ref.mpi_smod(x, q) for x in xs] for xs in polys], "gpq_rns_reconstruct, logq = %d" % k
    assert torch.equal(a, b), "gpq_rns_reconstruct_general(q = 2^%d) differs from gpq_rns_reconstruct" % k
    # he_rs: Delta = 2^s
    Wr = W + 1
    top = 1 << (64 * Wr - 1)
    for s in (1, 30, 63):
        d = 1 << s
        vals = [[rng.randrange(-top, top) for _ in range(n)] for _ in range(6)]
        for v in vals:
            v[:8] = [top - 1, -(top - 1), -top, 0, 5 * d + d // 2, -5 * d + d // 2, 5 * d + d // 2 + 1, -(5 * d + d // 2 + 1)]
        c = [_big(vals[:3], Wr), _big(vals[3:], Wr)]
        t = [x.clone() for x in c]
        g.he_rs(c[0], c[1], Wr, s, k)
        g.he_rs_general(t[0], t[1], Wr, d, q)
        exp = [[ref.mpi_smod(ref.mpi_rdiv(x, d), q) for x in v] for v in vals]
        assert _ints(c[0], Wr, n) + _ints(c[1], Wr, n) == exp, "gpq_he_rs, logDelta = %d, logql = %d" % (s, k)
        assert torch.equal(c[0], t[0]) and torch.equal(c[1], t[1]), "gpq_he_rs_general(2^%d, 2^%d) differs from gpq_he_rs" % (s, k)
    # he_mul at one small shape
    dimP, dimA, dimB, dimevk = g.he_dims(k, k)
    g, o = engine_ctx(7, dimevk), oracle_ctx(7, dimevk)
    rlk0, rlk1 = o.gen(3100 + k, dimevk), o.gen(3200 + k, dimevk)
    cts = [[[ref.mpi_smod(rng.randrange(q), q) for _ in range(n)] for _ in range(4)] for _ in range(2)]
    dev = [_big([cts[j][i] for j in range(2)], W) for i in range(4)]
    o0, o1, t0, t1 = (torch.empty_like(dev[0]) for _ in range(4))
    g.he_mul(o0, o1, *dev, to_device(rlk0), to_device(rlk1), W, k, dimA, dimB, dimP)
    g.he_mul_general(t0, t1, *dev, to_device(rlk0), to_device(rlk1), W, q, dimA, dimB, dimP)
    for j in range(2):
        e0, e1 = ref.he_mul(o, (cts[j][0], cts[j][1]), (cts[j][2], cts[j][3]), rlk0[: dimB * n], rlk1[: dimB * n], dimP, dimA, dimB, k)
        assert _ints(o0, W, n)[j] == e0 and _ints(o1, W, n)[j] == e1, "gpq_he_mul, logql = %d, ciphertext %d" % (k, j)
    assert torch.equal(o0, t0) and torch.equal(o1, t1), "gpq_he_mul_general(q = 2^%d) differs from gpq_he_mul" % k


# ---------------------------------------------------------------------------
# (c) gpq_he_rs_general: remainders on the rounding tie, Delta at the top of the word
# ---------------------------------------------------------------------------
DELTAS = [1, 2, 3, (1 << 32) + 1, 1 << 63, (1 << 63) + 1, B - 1]
RS_CASES = [(1, B - 59), (1, 3),
            (2, (1 << 127) - 1), (2, B), (2, 3 * B),
            (14, ODD_1000 >> 200 | 1), (14, B), (14, B * B), (14, 3 * B)]


def _rs_values(rng, delta, W, n):
    top = 1 << (64 * W - 1)
    h = delta // 2
    kmax = max(1, (top - delta) // delta)
    vals = [top - 1, -(top - 1), -top, 0, 1, -1]
    for r in {h, h + 1}:
        if r >= delta:                              # Delta = 1: the only remainder is 0
            continue
        for k in {0, 1, -1, -2, kmax, -kmax, rng.randrange(-kmax, kmax), rng.randrange(-kmax, kmax)}:
            vals += [k * delta + r, -(k * delta + r)]      # floor remainder r, and delta - r on the negation
    vals = [v for v in vals if -top <= v < top]
    vals += [rng.randrange(-top, top) for _ in range(n - len(vals))]
    rng.shuffle(vals)
    return vals


@pytest.mark.parametrize("W,ql", RS_CASES, ids=["W%d-%#x" % (W, ql) if ql < 1 << 130 else "W%d-odd" % W for W, ql in RS_CASES])
def test_he_rs_general_ties_and_top_word_delta(engine_ctx, W, ql):
    """src/he-rescale.c:45-48: mpi_rdiv by Delta (round up only when the floor remainder exceeds floor(Delta/2)), then
    mpi_smod(., q_l); Delta up to 2^64 - 1, W = 1, 2, 14 words, batch 3 per component"""
    g = engine_ctx(7, 12)
    n = g.n
    rng = random.Random(W * 7919 + ql % 65521)
    for delta in DELTAS:
        vals = [_rs_values(rng, delta, W, n) for _ in range(6)]
        c0, c1 = _big(vals[:3], W), _big(vals[3:], W)
        g.he_rs_general(c0, c1, W, delta, ql)
        got = _ints(c0, W, n) + _ints(c1, W, n)
        for k in range(6):
            exp = [ref.mpi_smod(ref.mpi_rdiv(x, delta), ql) for x in vals[k]]
            bad = [i for i in range(n) if got[k][i] != exp[i]]
            assert not bad, "Delta=%#x q_l=%#x W=%d poly %d: %d differ, first x=%d gave %d, want %d" % (
                delta, ql, W, k, len(bad), vals[k][bad[0]], got[k][bad[0]], exp[bad[0]])


# ---------------------------------------------------------------------------
# (d) gpq_relin_tail_general on the rounding ties and the wrap corner
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("ql", [ODD_1000 >> 797 | 1, B * B], ids=["odd200", "2^128"])
def test_relin_tail_general_rounding_ties_and_wrap_corner(engine_ctx, oracle_ctx, ql, mfma):
    """The construction of test_relin_tail_rounding_ties_and_wrap_corner through the general entry: x mod P on floor(P/2) - 1,
    floor(P/2), floor(P/2) + 1, 0, P - 1; the quotient on floor(Pi'/2), floor(Pi'/2) - 1 and at the most negative value.  With d,
    with d = NULL and in place (out == d); batch 2."""
    torch = _torch()
    logn, bits = 7, ql.bit_length()
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 12).he_dims(bits, bits)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    g.set_bridge_mfma(mfma)
    n, W = g.n, (bits + 64) // 64
    P = ref.RnsBasis(o.p[:dimP]).P
    PiB = ref.RnsBasis(o.p[:dimB]).P
    Piq = PiB // P
    half, hq = P // 2, Piq // 2
    rng = random.Random(bits)
    chats, dvals, exp = [], [], []
    for k in range(2):
        xs = []
        for i in range(n):
            r = [half - 1, half, half + 1, 0, P - 1][(i + k) % 5] if i < 60 else rng.randrange(P)
            if i < 20:
                qt = hq
            elif i < 40:
                qt = hq - 1
            elif i < 50:
                qt = -hq - 1 if r else -hq
            else:
                qt = rng.randrange(-hq + 2, hq - 2)
            xs.append((qt * P + r) % PiB)
        chat = np.array([v % o.p[d] for d in range(dimB) for v in xs], dtype=np.uint64)
        dv = [rng.randrange(-(ql // 2), ql - ql // 2) for _ in range(n)]
        dv[:4] = [ql // 2 - 1, -(ql - ql // 2), 0, -1]
        chats.append(chat)
        dvals.append(dv)
        exp.append(ref.he_relin_tail(o, chat, chat, dv, None, dimP, dimB, ql))
    chat = to_device(np.concatenate(chats))
    try:
        out = torch.empty(2 * W * n, dtype=torch.int64, device="cuda")
        g.relin_tail_general(out, chat, _big(dvals, W), W, ql, dimB, dimP)
        assert _ints(out, W, n) == [e[0] for e in exp], "with d"
        g.relin_tail_general(out, chat, None, W, ql, dimB, dimP)
        assert _ints(out, W, n) == [e[1] for e in exp], "d = NULL"
        inplace = _big(dvals, W)
        g.relin_tail_general(inplace, chat, inplace, W, ql, dimB, dimP)
        assert _ints(inplace, W, n) == [e[0] for e in exp], "in place"
    finally:
        g.set_bridge_mfma(True)


# ---------------------------------------------------------------------------
# (e) gpq_he_mulpt_general
# ---------------------------------------------------------------------------
def test_he_mulpt_general_matches_reference_semantics(engine_ctx, oracle_ctx):
    torch = _torch()
    logn, dim, ql = 8, 4, 1000003 ** 7            # odd, 140 bits
    g, o = engine_ctx(logn, 12), oracle_ctx(logn, 12)
    n, W = g.n, 3
    rng = random.Random(29)
    h = ql // 2
    cts = [[[rng.randrange(-h, ql - h) for _ in range(n)] for _ in range(2)] for _ in range(3)]
    ms = [[rng.randrange(-(1 << 40), 1 << 40) for _ in range(n)] for _ in range(3)]
    for k in range(3):
        cts[k][0][:3] = [h - 1, -(ql - h), 0]
        ms[k][:3] = [(1 << 40) - 1, -(1 << 40), 1]
    c0, c1, m = _big([c[0] for c in cts], W), _big([c[1] for c in cts], W), _big(ms, W)
    o0, o1 = torch.empty_like(c0), torch.empty_like(c0)
    g.he_mulpt_general(o0, o1, c0, c1, m, W, ql, dim)
    got0, got1 = _ints(o0, W, n), _ints(o1, W, n)
    for k in range(3):
        e0, e1 = ref.he_mulpt(o, cts[k], ms[k], dim, 0, ql=ql)
        assert got0[k] == e0 and got1[k] == e1, "ciphertext %d" % k


# ---------------------------------------------------------------------------
# (f) launch groups and squaring in gpq_he_mul_general / gpq_he_swk_general
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [7, 13])
def test_he_mul_swk_general_launch_groups_and_squaring(engine_ctx, oracle_ctx, logn):
    """gpq_set_chunk(2), batch 5: groups of 2, 2 and 1 ciphertexts.  Every ciphertext at the end of a group (here: all five) against
    the restated reference; squaring (ct1 and ct2 the same pointers) against the call on copies and against the reference."""
    torch = _torch()
    Delta, L = 1000003, 5
    ql = Delta ** L * 1048573                      # odd, 120 bits (test_general_moduli_he_mul_swk_rs's q_L)
    probe = engine_ctx(logn, 12)
    nbl = ql.bit_length()
    dimP = (nbl + logn) // 59 + 1
    nbPq = (ref.RnsBasis(probe.p[:dimP]).P * ql).bit_length()
    dimA, dimB = (2 * nbl + logn) // 59 + 1, (nbl + nbPq + logn) // 59 + 1
    g, o = engine_ctx(logn, dimB), oracle_ctx(logn, dimB)
    n, W, batch, chunk = g.n, nbl // 64 + 1, 5, 2
    rng = random.Random(logn)
    h = ql // 2
    cts = [[[rng.randrange(-h, ql - h) for _ in range(n)] for _ in range(4)] for _ in range(batch)]
    for k in range(batch):
        cts[k][k % 4][:3] = [h - 1, -(ql - h), 0]
    rlk0, rlk1 = o.gen(3300, dimB), o.gen(3301, dimB)
    krl0, krl1 = to_device(rlk0), to_device(rlk1)
    dev = [_big([cts[k][i] for k in range(batch)], W) for i in range(4)]
    idx = group_ends(batch, chunk)
    try:
        g.set_chunk(chunk)
        o0, o1 = torch.empty_like(dev[0]), torch.empty_like(dev[0])
        g.he_mul_general(o0, o1, *dev, krl0, krl1, W, ql, dimA, dimB, dimP)
        got = [_ints(o0, W, n), _ints(o1, W, n)]
        prods = {}
        for k in idx:
            prods[k] = ref.he_mul(o, (cts[k][0], cts[k][1]), (cts[k][2], cts[k][3]), rlk0[: dimB * n], rlk1[: dimB * n], dimP, dimA, dimB, 0, ql=ql)
            assert got[0][k] == prods[k][0] and got[1][k] == prods[k][1], "he_mul_general, ciphertext %d" % k
        # squaring: the same pointers for ct1 and ct2
        s0, s1, t0, t1 = (torch.empty_like(dev[0]) for _ in range(4))
        g.he_mul_general(s0, s1, dev[0], dev[1], dev[0], dev[1], krl0, krl1, W, ql, dimA, dimB, dimP)
        g.he_mul_general(t0, t1, dev[0], dev[1], dev[0].clone(), dev[1].clone(), krl0, krl1, W, ql, dimA, dimB, dimP)
        assert torch.equal(s0, t0) and torch.equal(s1, t1), "squaring differs from the call on copies"
        sq = [_ints(s0, W, n), _ints(s1, W, n)]
        for k in idx:
            e0, e1 = ref.he_mul(o, (cts[k][0], cts[k][1]), (cts[k][0], cts[k][1]), rlk0[: dimB * n], rlk1[: dimB * n], dimP, dimA, dimB, 0, ql=ql)
            assert sq[0][k] == e0 and sq[1][k] == e1, "squaring, ciphertext %d" % k
        # he_swk on the products
        w0, w1 = torch.empty_like(dev[0]), torch.empty_like(dev[0])
        g.he_swk_general(w0, w1, o0, o1, krl1, krl0, W, ql, dimB, dimP)
        sw = [_ints(w0, W, n), _ints(w1, W, n)]
        for k in idx:
            e0, e1 = ref.he_swk(o, prods[k][0], prods[k][1], rlk1[: dimB * n], rlk0[: dimB * n], dimP, dimB, 0, ql=ql)
            assert sw[0][k] == e0 and sw[1][k] == e1, "he_swk_general, ciphertext %d" % k
    finally:
        g.set_chunk(32)
