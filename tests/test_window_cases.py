"""tests/window_cases.py on the CPU: the conditions of the construction hold at every shape tests/test_he_windows_gpu.py runs, the model of
the estimate agrees with exact rationals about its own error bound, and the identity the construction stands on -- the key switch of the
constant polynomial 1 with the key NTT(chat) is chat -- holds in the oracle."""
import random
from fractions import Fraction

import numpy as np
import pytest

from oracle import bigint_ref as ref
from tests import window_cases as wc

# (logn, log2 q_L, log2 q_l) of tests/test_he_windows_gpu.py
SHAPES = [(9, 200, 200), (10, 438, 438), (9, 850, 850), (9, 850, 500), (13, 200, 200), (13, 438, 438), (13, 850, 850), (13, 850, 500)]


def _model(oracle_ctx, logn, logqL, logql):
    o = oracle_ctx(logn, 60)
    dimP, dimA, dimB, _ = ref.he_dims(logn, o.p, logqL, logql)
    return o, wc.TailModel(o.p, dimP, dimB), (dimA, dimB, dimP)


@pytest.mark.parametrize("logn,logqL,logql", SHAPES)
def test_builder_conditions(oracle_ctx, logn, logqL, logql):
    o, M, _ = _model(oracle_ctx, logn, logqL, logql)
    n = 1 << logn
    a, b = wc.build(M, n, 11), wc.build(M, n, 12)                  # (build() asserts check() itself)
    wc.check(M, a, n, False)
    scattered = lambda c: set(c.cls) - {0, 63, 64, n - 1}
    assert scattered(a) != scattered(b), "rlk0 and rlk1 must carry different layouts"
    assert any(i not in b.cls for i in scattered(a)) and any(i not in a.cls for i in scattered(b))
    rng = random.Random(logn)
    d = [rng.randrange(-(1 << (logql - 1)), 1 << (logql - 1)) for _ in range(n)]
    for s in (1, 40, 63, 64) if logn < 13 else (40,):      # (the quotient is made from the addend the same way for every s)
        c = wc.build(M, n, 13 + s, rs=(s, d))
        wc.check(M, c, n, True)
        for i, (name, _) in c.cls.items():
            if name in wc.RS_CLASSES:
                x = c.xs[i] - M.PiB if c.xs[i] > M.PiB // 2 else c.xs[i]
                assert x % M.P == M.half + 1
                low = (ref.mpi_rdiv(x, M.P) + d[i]) % (1 << s)
                assert low == ((1 << (s - 1)) + wc.RS_CLASSES.index(name) - 1) % (1 << s)


@pytest.mark.parametrize("logn,logqL,logql", SHAPES[:3])
def test_model_underestimates_by_less_than_its_bound(oracle_ctx, logn, logqL, logql):
    """frac / 2^104 <= (x mod P) / P < frac / 2^104 + dimP 2^60 / 2^104 (mod 1), exactly 0 apart for multiples of P"""
    o, M, _ = _model(oracle_ctx, logn, logqL, logql)
    rng = random.Random(1)
    c = wc.build(M, 1 << logn, 11)
    for x in [c.xs[i] for i in c.cls] + [rng.randrange(M.PiB) for _ in range(40)]:
        true = Fraction(x % M.P, M.P)
        est = Fraction(M.frac(x), 1 << wc.FRAC_BITS)
        gap = (true - est) % 1
        assert gap < Fraction(M.dimP << 60, 1 << wc.FRAC_BITS)
        if x % M.P == 0:
            assert gap == 0


def test_random_coefficients_are_not_in_a_window(oracle_ctx):
    o, M, _ = _model(oracle_ctx, 9, 200, 200)
    rng = random.Random(2)
    assert not any(M.window(rng.randrange(M.PiB)) for _ in range(2000))


@pytest.mark.parametrize("logn,logqL", [(9, 200), (10, 438)])
def test_key_switch_of_one_with_the_transformed_residues_returns_them(oracle_ctx, logn, logqL):
    o, M, (dimA, dimB, dimP) = _model(oracle_ctx, logn, logqL, logqL)
    n = 1 << logn
    c0, c1 = wc.build(M, n, 21), wc.build(M, n, 22)
    chat0, chat1 = c0.slab(o.p, dimB), c1.slab(o.p, dimB)
    one = ref._slab(o, [1] + [0] * (n - 1), dimB)
    got = o.keyswitch(one, o.ntt_slab(chat0, dimB), o.ntt_slab(chat1, dimB), dimB)
    assert np.array_equal(got[0], chat0) and np.array_equal(got[1], chat1)
    # ... and the whole restated he_swk then sees the chosen integers: its output is rdiv(x, P) + d0 in closed form
    ql = 1 << logqL
    rng = random.Random(3)
    d0 = [rng.randrange(-(ql // 2), ql // 2) for _ in range(n)]
    e0, e1 = ref.he_swk(o, d0, [1] + [0] * (n - 1), o.ntt_slab(chat0, dimB), o.ntt_slab(chat1, dimB), dimP, dimB, logqL)
    for xs, dd, e in ((c0.xs, d0, e0), (c1.xs, None, e1)):
        for i in range(n):
            x = ref.mpi_smod(ref.mpi_smod(xs[i], M.PiB), M.P * ql)
            assert e[i] == ref.mpi_smod((ref.mpi_rdiv(x, M.P) + (dd[i] if dd else 0)) % ql, ql)


@pytest.mark.parametrize("dim,fb,wb", [(15, 104, 38), (45, 104, 38), (58, 104, 38), (15, 128, 61), (58, 128, 61)])
def test_crt_ladder_has_both_sides(oracle_ctx, dim, fb, wb):
    o = oracle_ctx(8, 60)
    M = wc.CrtModel(o.p, dim, fb, wb)
    lad = wc.crt_ladder(M)
    assert sum(1 for _, w in lad if w) >= 4 and sum(1 for _, w in lad if not w) >= 4
    assert all(0 <= x < M.P for x, _ in lad)
