"""gpq_he_lin_const -- up to three signed ciphertexts, he_const_pt's a + b x^(n/2) and ONE mpi_smod in one launch (algo_kernels.hpp) -- against
Python integers, and word for word against the calls it replaces: gpq_big_addsub + gpq_he_rs(.., 0, logql) and gpq_he_addpt_const.

Shapes: logn 6 (one workgroup), every word count with a different last word (1, 2, 4, 5: a word that holds sign extension only), every logql
that puts the sign bit at a word's first, last or an inner bit; logn 11 for several workgroups per polynomial.  Inputs: values centred for a
modulus 2^30 above the output's (he_moddown), the four values around +-2^(logql-1), all-ones words, and pairs whose sum or difference carries
across every word boundary.  The expectation is exact integer arithmetic: no tolerance."""
import itertools
import random

import numpy as np
import pytest

from gpqhe_amd import big_to_ints, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref
from tests.const_pt_cases import BIG

pytestmark = pytest.mark.gpu

LOGN, BATCH = 6, 3
GPQ_ERR_INVALID = -1
SHAPES = [(W, logql) for W in (1, 2, 4, 5) for logql in (1, 63, 64, 65, 127, 128, 200) if logql <= 64 * W]
CONSTANTS = [(0, 0), (1, 0), (-1, 0), (1 << 62, 0), (-(1 << 62), 0), BIG, (0, 1), (0, -(1 << 62)), (7, -3)]
SIGNS = [s for K in (1, 2, 3) for s in itertools.product((1, -1), repeat=K)]


def _torch():
    import torch
    return torch


def terms_for(n, W, logql, seed):
    """three terms of BATCH ciphertexts each: [term][ciphertext][c0 | c1][coefficient]"""
    rng = random.Random(seed)
    lim = 1 << (64 * W - 1)
    fit = lambda v: max(-lim, min(lim - 1, v))
    wide = min(logql + 30, 64 * W)                          # centred for a larger modulus, then moved down
    h, hw = 1 << (logql - 1), 1 << (wide - 1)
    edges = [h - 1, -h, h, -h - 1, hw - 1, -hw, -1, 0, 1, lim - 1, -lim]
    out = []
    for t in range(3):
        cts = []
        for k in range(BATCH):
            ct = []
            for c in range(2):
                if k == 2:
                    v = [rng.randrange(-lim, lim) for _ in range(n)]               # any W-word value
                else:
                    v = [rng.randrange(-hw, hw) for _ in range(n)]
                if k == 1:                                                         # all-ones words and carries across every word boundary
                    for j in range(1, W + 1):
                        top = fit((1 << (64 * j)) - 1)                             # 64 j ones: + 1, or - (-1), carries into word j
                        v[j] = [(top, 1, -top), (-top, -1, top)][c][t]
                        v[8 + j] = fit(-(1 << (64 * j - 1)))                       # twice this borrows from word j
                        v[16 + j] = -1
                e = edges[t:] + edges[:t]
                v[0], v[n // 2] = fit(e[0]), fit(e[1])                             # where a and b land
                v[40:40 + len(e) - 2] = [fit(x) for x in e[2:]]
                ct.append(v)
            cts.append(ct)
        out.append(cts)
    return out


def expected(terms, signs, a, b, logql):
    q, n = 1 << logql, len(terms[0][0][0])
    res = []
    for k in range(len(terms[0])):
        c0 = [ref.mpi_smod(sum(s * t[k][0][i] for s, t in zip(signs, terms)) + (a if i == 0 else b if i == n // 2 else 0), q) for i in range(n)]
        c1 = [ref.mpi_smod(sum(s * t[k][1][i] for s, t in zip(signs, terms)), q) for i in range(n)]
        res.append([c0, c1])
    return res


def upload(terms, W):
    """[term] -> (c0 slab, c1 slab) of the term's ciphertexts"""
    return [tuple(to_device(np.concatenate([ints_to_big(ct[c], W) for ct in cts])) for c in range(2)) for cts in terms]


def download(g, o0, o1, W):
    r0, r1 = big_to_ints(to_host(o0), W, g.n), big_to_ints(to_host(o1), W, g.n)
    return [[r0[k], r1[k]] for k in range(len(r0))]


def call(g, dev, signs, a, b, W, logql, in_place=None):
    torch = _torch()
    use = [(d[0].clone(), d[1].clone()) if in_place is not None else d for d in dev[:len(signs)]]
    if in_place is None:
        o0, o1 = torch.full_like(dev[0][0], 0x5A5A5A5A), torch.full_like(dev[0][1], 0x5A5A5A5A)
    else:
        o0, o1 = use[in_place]
    g.he_lin_const(o0, o1, [(x0, x1, s) for (x0, x1), s in zip(use, signs)], W, logql, a, b)
    return download(g, o0, o1, W)


@pytest.mark.parametrize("W,logql", SHAPES)
def test_every_sign_pattern_against_integers(engine_ctx, W, logql):
    g = engine_ctx(LOGN, 4)
    terms = terms_for(g.n, W, logql, 64 * W + logql)
    dev = upload(terms, W)
    for i, signs in enumerate(SIGNS):
        a, b = CONSTANTS[i % len(CONSTANTS)]
        assert call(g, dev, signs, a, b, W, logql) == expected(terms[:len(signs)], signs, a, b, logql), (signs, a, b)
    for a, b in CONSTANTS:                                  # every constant on one pattern of each K
        for signs in ((1,), (-1, 1), (1, -1, -1)):
            assert call(g, dev, signs, a, b, W, logql) == expected(terms[:len(signs)], signs, a, b, logql), (signs, a, b)
    for t, cts in zip(dev, terms):                          # the inputs are as they were
        assert download(g, t[0], t[1], W) == cts


@pytest.mark.parametrize("W,logql", [(1, 1), (1, 64), (2, 65), (4, 200), (5, 200)])
def test_in_place_on_each_input_position(engine_ctx, W, logql):
    g = engine_ctx(LOGN, 4)
    terms = terms_for(g.n, W, logql, 3 * W + logql)
    dev = upload(terms, W)
    for signs, (a, b) in zip([(-1,), (1, -1), (-1, 1, 1), (-1, -1, -1)], [(2 << 30, 0), (0, 0), BIG, (-5, 9)]):
        exp = expected(terms[:len(signs)], signs, a, b, logql)
        for pos in range(len(signs)):
            assert call(g, dev, signs, a, b, W, logql, in_place=pos) == exp, (signs, pos)


@pytest.mark.parametrize("W,logql", [(1, 63), (2, 64), (2, 128), (4, 200), (5, 200)])
def test_equals_the_calls_it_replaces_word_for_word(engine_ctx, W, logql):
    torch = _torch()
    g = engine_ctx(LOGN, 4)
    terms = terms_for(g.n, W, logql, 11 * W + logql)
    dev = upload(terms, W)
    (x0, x1), (y0, y1) = dev[0], dev[1]
    for mode, signs in ((0, (1, 1)), (1, (1, -1)), (2, (-1,))):         # he_add / he_sub / he_neg: gpq_big_addsub, then gpq_he_rs(.., 0, logql)
        r0, r1 = torch.empty_like(x0), torch.empty_like(x1)
        g.big_addsub(r0, x0, y0 if mode < 2 else None, W, mode)
        g.big_addsub(r1, x1, y1 if mode < 2 else None, W, mode)
        g.he_rs(r0, r1, W, 0, logql)
        o0, o1 = torch.empty_like(x0), torch.empty_like(x1)
        g.he_lin_const(o0, o1, [(d[0], d[1], s) for d, s in zip(dev, signs)], W, logql)
        assert torch.equal(o0, r0) and torch.equal(o1, r1), mode
    r0, r1 = x0.clone(), x1.clone()                                     # he_moddown / he_copy_ct of a centred value: gpq_he_rs(.., 0, logql) alone
    g.he_rs(r0, r1, W, 0, logql)
    o0, o1 = torch.empty_like(x0), torch.empty_like(x1)
    g.he_lin_const(o0, o1, [(x0, x1, 1)], W, logql)
    assert torch.equal(o0, r0) and torch.equal(o1, r1)
    for a, b in CONSTANTS[1:]:                                          # he_addpt / he_subpt: gpq_he_addpt_const
        for sub in (False, True):
            if sub and (a == -(1 << 63) or b == -(1 << 63)):
                continue                                                # -INT64_MIN is no int64_t: he_subpt by it has no gpq_he_lin_const spelling
            r0, r1 = torch.empty_like(x0), torch.empty_like(x1)
            g.he_addpt_const(r0, r1, x0, x1, a, b, W, logql, sub)
            g.he_lin_const(o0, o1, [(x0, x1, 1)], W, logql, -a if sub else a, -b if sub else b)
            assert torch.equal(o0, r0) and torch.equal(o1, r1), (a, b, sub)


def test_several_workgroups_per_polynomial(engine_ctx):
    logn, W, logql = 11, 4, 200
    g = engine_ctx(logn, 4)
    terms = terms_for(g.n, W, logql, 2011)
    dev = upload(terms, W)
    for signs, (a, b) in (((1, -1, 1), BIG), ((-1,), (2 << 30, 0))):
        exp = expected(terms[:len(signs)], signs, a, b, logql)
        assert call(g, dev, signs, a, b, W, logql) == exp
        assert call(g, dev, signs, a, b, W, logql, in_place=len(signs) - 1) == exp


def test_bad_arguments_are_refused_and_nothing_is_written(engine_ctx):
    import ctypes as C
    torch = _torch()
    g = engine_ctx(LOGN, 4)
    W = 2
    x = [torch.zeros(BATCH * W * g.n, dtype=torch.int64, device="cuda") for _ in range(4)]
    o = [torch.full_like(x[0], 0x5A5A5A5A) for _ in range(2)]
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])

    def rc(K=2, signs=(1, -1, 1), logql=100, o0=o[0], o1=o[1], x0=(x[0], x[2]), x1=(x[1], x[3])):
        return g.lib.gpq_he_lin_const(g.h, g._ptr(o0), g._ptr(o1), arr(x0), arr(x1), (C.c_int * 3)(*signs), K, 0, 0, W, logql, BATCH, g._stream())

    assert rc() == 0
    for bad in (dict(K=0), dict(K=4), dict(signs=(1, 0, 1)), dict(signs=(2, 1, 1)), dict(logql=0), dict(logql=64 * W + 1),
                dict(o0=x[1]),                                          # c0's output on a term's c1
                dict(o0=x[2], x0=(x[0], x[2][g.n:]))):                  # overlapping a term, but not in the same position
        o[0].fill_(0x5A5A5A5A); o[1].fill_(0x5A5A5A5A)
        assert rc(**bad) == GPQ_ERR_INVALID, bad
        torch.cuda.synchronize()
        assert bool((o[0] == 0x5A5A5A5A).all()) and bool((o[1] == 0x5A5A5A5A).all()), bad
