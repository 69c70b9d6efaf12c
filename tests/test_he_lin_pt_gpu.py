"""gpq_he_lin_pt -- gpq_he_lin_const plus ONE dense plaintext m, added with sign msign into c0 only and shared by the whole batch
(algo_kernels.hpp, he_lin_const<K, true>) -- against Python integers and word for word against gpq_he_lin_const + gpq_big_addsub +
gpq_he_rs(.., 0, logql) per ciphertext.

Shapes: logn 7 (half a 256-lane block) and logn 9 (two blocks), W 1 and 4, batch 1 and 3, logql at a word's first, last and inner bits, K 1..3,
every sign pattern for K <= 2 and two for K = 3.  m: 0; -1 on every coefficient (sign-extended: all-ones words); +-(2^(64 j) - 1), which
carries across every word boundary when it meets the terms' own carry patterns; 64 W random bits; each with a = b = 0 and with a != 0, b != 0.
Exact integers: no tolerance."""
import ctypes as C
import random

import numpy as np
import pytest

from gpqhe_amd import ints_to_big, to_device
from oracle import bigint_ref as ref
from tests.const_pt_cases import BIG
from tests.test_he_lin_const_gpu import download, expected, terms_for, upload

pytestmark = pytest.mark.gpu

GPQ_ERR_INVALID = -1
POISON = 0x5A5A5A5A
SIGNS = [(1,), (-1,), (1, 1), (1, -1), (-1, 1), (-1, -1), (1, -1, 1), (-1, -1, -1)]
CONSTANTS = [(0, 0), (7, -3), BIG, (-(1 << 62), 1 << 62)]
SHAPES = [(logn, W, batch, logql) for logn in (7, 9) for W in (1, 4) for batch in (1, 3) for logql in (1, 63, 64, 65, 128, 200) if logql <= 64 * W]


def _torch():
    import torch
    return torch


def plaintexts(n, W, seed):
    rng = random.Random(seed)
    lim = 1 << (64 * W - 1)
    fit = lambda v: max(-lim, min(lim - 1, v))
    carry = [fit((1 << (64 * (1 + i % W))) - 1) * (1 if (i // W) % 2 == 0 else -1) for i in range(n)]
    return {"zero": [0] * n, "ones": [-1] * n, "carry": carry, "random": [rng.randrange(-lim, lim) for _ in range(n)]}


def shape(engine_ctx, logn, W, batch, logql, seed):
    g = engine_ctx(logn, 4)
    full = terms_for(g.n, W, logql, seed)                   # three ciphertexts per term; a batch of one takes the one with the carry patterns
    terms = [cts[1:2] if batch == 1 else cts for cts in full]
    ms = plaintexts(g.n, W, seed + 1)
    return g, terms, upload(terms, W), ms, {k: to_device(ints_to_big(v, W)) for k, v in ms.items()}


def expected_pt(terms, signs, m, msign, a, b, logql):
    q = 1 << logql
    res = expected(terms, signs, a, b, logql)
    return [[[ref.mpi_smod(x + msign * y, q) for x, y in zip(ct[0], m)], ct[1]] for ct in res]


def call(g, dev, signs, mdev, msign, a, b, W, logql, in_place=None):
    torch = _torch()
    use = [(d[0].clone(), d[1].clone()) if in_place is not None else d for d in dev[:len(signs)]]
    if in_place is None:
        o0, o1 = torch.full_like(dev[0][0], POISON), torch.full_like(dev[0][1], POISON)
    else:
        o0, o1 = use[in_place]
    g.he_lin_pt(o0, o1, [(x0, x1, s) for (x0, x1), s in zip(use, signs)], mdev, W, logql, msign, a, b)
    return o0, o1


@pytest.mark.parametrize("logn,W,batch,logql", SHAPES)
def test_against_integers_and_the_calls_it_replaces(engine_ctx, logn, W, batch, logql):
    torch = _torch()
    g, terms, dev, ms, mdev = shape(engine_ctx, logn, W, batch, logql, 1000 * logn + 64 * W + logql)
    names = sorted(ms)
    poly = W * g.n
    cases = [(signs, names[i % 4], 1 if i % 3 else -1, CONSTANTS[i % 4]) for i, signs in enumerate(SIGNS)]
    cases += [((1, -1), name, msign, c) for name in names for msign in (1, -1) for c in (CONSTANTS[0], CONSTANTS[1 + names.index(name) % 3])]
    m_before = {k: v.clone() for k, v in mdev.items()}
    for signs, name, msign, (a, b) in cases:
        K = len(signs)
        o0, o1 = call(g, dev, signs, mdev[name], msign, a, b, W, logql)
        assert download(g, o0, o1, W) == expected_pt(terms[:K], signs, ms[name], msign, a, b, logql), (signs, name, msign, a, b)
        # ... and the separate calls: the sum without m, then m into c0 of each ciphertext, then one more mpi_smod
        r0, r1 = torch.empty_like(o0), torch.empty_like(o1)
        g.he_lin_const(r0, r1, [(d[0], d[1], s) for d, s in zip(dev, signs)], W, logql, a, b)
        for k in range(batch):
            sl = r0[k * poly:(k + 1) * poly]
            sl.copy_(g.big_addsub(torch.empty_like(sl), sl, mdev[name], W, 0 if msign > 0 else 1))
        g.he_rs(r0, r1, W, 0, logql)
        assert torch.equal(o0, r0) and torch.equal(o1, r1), (signs, name, msign, a, b)
    for t, cts in zip(dev, terms):                          # the inputs and the plaintexts are as they were
        assert download(g, t[0], t[1], W) == cts
    assert all(torch.equal(mdev[k], m_before[k]) for k in mdev)


@pytest.mark.parametrize("logn,W,batch,logql", [(7, 1, 3, 64), (7, 4, 1, 200), (9, 4, 3, 65), (9, 1, 1, 1)])
def test_in_place_on_term_zero(engine_ctx, logn, W, batch, logql):
    g, terms, dev, ms, mdev = shape(engine_ctx, logn, W, batch, logql, 77 * logn + W + logql)
    for signs, name, msign, (a, b) in [((-1,), "carry", -1, (7, -3)), ((1, -1), "random", 1, BIG), ((-1, 1, 1), "ones", -1, (0, 0))]:
        o0, o1 = call(g, dev, signs, mdev[name], msign, a, b, W, logql, in_place=0)
        assert download(g, o0, o1, W) == expected_pt(terms[:len(signs)], signs, ms[name], msign, a, b, logql), (signs, name)


def test_msign_and_c1(engine_ctx):
    """m enters c0 only, and with its sign: + m and - m differ from each other and from no m exactly where m is not 0 mod q"""
    logn, W, batch, logql = 7, 4, 3, 200
    g, terms, dev, ms, mdev = shape(engine_ctx, logn, W, batch, logql, 4242)
    plus = download(g, *call(g, dev, (1,), mdev["random"], 1, 0, 0, W, logql), W)
    minus = download(g, *call(g, dev, (1,), mdev["random"], -1, 0, 0, W, logql), W)
    none = expected(terms[:1], (1,), 0, 0, logql)
    q = 1 << logql
    for k in range(batch):
        assert plus[k][1] == none[k][1] and minus[k][1] == none[k][1]
        assert all((p - z - m) % q == 0 and (z - s - m) % q == 0 for p, s, z, m in zip(plus[k][0], minus[k][0], none[k][0], ms["random"]))
        assert plus[k][0] != minus[k][0]


def test_bad_arguments_are_refused_and_nothing_is_written(engine_ctx):
    torch = _torch()
    g = engine_ctx(7, 4)
    W, batch = 2, 3
    words, band = batch * W * g.n, 512
    x = [torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(4)]
    m = torch.zeros(W * g.n, dtype=torch.int64, device="cuda")
    arena = torch.full((2 * words + 3 * band,), POISON, dtype=torch.int64, device="cuda")       # band | out0 | band | out1 | band
    o0, o1 = arena[band:band + words], arena[2 * band + words:2 * band + 2 * words]
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    NULL = C.c_void_p(None)

    def rc(K=2, signs=(1, -1, 1), logql=100, o0=o0, o1=o1, x0=(x[0], x[2]), x1=(x[1], x[3]), m=g._ptr(m), msign=1):
        return g.lib.gpq_he_lin_pt(g.h, g._ptr(o0), g._ptr(o1), arr(x0), arr(x1), (C.c_int * 3)(*signs), K, m, msign, 0, 0, W, logql, batch, g._stream())

    assert rc() == 0 and rc(msign=-1) == 0
    torch.cuda.synchronize()
    assert bool((o0 == 0).all()) and bool((o1 == 0).all())
    for bad in (dict(m=NULL), dict(msign=0), dict(msign=2), dict(msign=-2),
                dict(m=g._ptr(o0[g.n:])), dict(m=g._ptr(arena[2 * band + 2 * words - 8:])),       # m overlapping out0 / the end of out1
                dict(K=0), dict(K=4), dict(signs=(1, 0, 1)), dict(signs=(2, 1, 1)), dict(logql=0), dict(logql=64 * W + 1),
                dict(o0=x[1]), dict(o0=x[2], x0=(x[0], x[2][g.n:]))):
        arena.fill_(POISON)
        x[1].fill_(POISON); x[2].fill_(POISON)
        assert rc(**bad) == GPQ_ERR_INVALID, bad
        torch.cuda.synchronize()
        assert bool((arena == POISON).all()) and bool((x[1] == POISON).all()) and bool((x[2] == POISON).all()), bad
    assert b"gpq_he_lin_pt" in g.lib.gpq_last_error()
