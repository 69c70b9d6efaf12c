"""The closed form of he_mulpt / he_rs / he_addpt / he_subpt by he_const_pt's plaintext (tests/const_pt_cases.py) pinned to the restated
reference (oracle/bigint_ref.py), to the executed one where oracle/_ref/ is built, and gpq_const_pt to exact rationals.  No GPU."""
import ctypes as C
import random
from fractions import Fraction

import pytest

from oracle import bigint_ref as ref
from oracle import ref as oref
from tests import const_pt_cases as cp

LOGN = 6


def _dimub():
    return max(cp.mulpt_dim(logql, lognu, LOGN) for logql, lognu in cp.SHAPES)


@pytest.mark.parametrize("logql,lognu", cp.SHAPES)
def test_closed_form_is_the_restated_reference(oracle_ctx, logql, lognu):
    o = oracle_ctx(LOGN, _dimub())
    n, dim = o.n, cp.mulpt_dim(logql, lognu, LOGN)
    ct = (cp.centred_inputs(n, logql, 3 * logql), cp.centred_inputs(n, logql, 3 * logql + 1))
    differed = 0
    for a, b in cp.constants(lognu, logql) + [cp.BIG]:
        want = ref.he_mulpt(o, ct, cp.const_plaintext(n, a, b), dim, logql)
        if not cp.fits(o.p, a, b, logql, dim):
            # the product wraps the basis: the reference's words are NOT the closed form, on both polynomials at every shift
            assert (a, b) == cp.BIG and logql <= 65
            for s in cp.shifts(logql, lognu):
                got = cp.closed_mulpt(ct, a, b, logql, s)
                exp = cp.ref_rs(want, s, logql) if s else want
                assert got[0] != exp[0] and got[1] != exp[1]
            differed += 1
            continue
        for s in cp.shifts(logql, lognu):
            exp = cp.ref_rs(want, s, logql) if s else want
            assert cp.closed_mulpt(ct, a, b, logql, s) == exp, (a, b, s)
            if s:
                assert cp.closed_mulpt_no_inner_smod(ct, a, b, logql, s) == exp, (a, b, s)
    assert differed == (1 if logql <= 65 else 0)


def test_fits_predicate(oracle_ctx):
    o = oracle_ctx(LOGN, _dimub())
    for logql, lognu in cp.SHAPES:
        dim = cp.mulpt_dim(logql, lognu, LOGN)
        for a, b in cp.constants(lognu, logql):
            assert cp.fits(o.p, a, b, logql, dim)
        assert cp.fits(o.p, *cp.BIG, logql, dim) == (logql > 65)
    # the boundary itself: (|a| + |b|) 2^(logql-1) against floor(P/2) of one prime
    P = int(o.p[0])
    top = (P // 2) >> 9                                     # logql = 10
    assert cp.fits(o.p, top, 0, 10, 1) == ((top << 9) < P // 2)
    assert not cp.fits(o.p, top + 1, 0, 10, 1)
    assert cp.fits(o.p, top - 1, 0, 10, 1) and cp.fits(o.p, 0, -(top - 1), 10, 1)


def test_closed_form_is_the_executed_reference():
    from tests import ref_jobs
    ref_jobs.require_reference()
    out, = oref.run(cp.reference_job, [cp.REF_CONSTANTS], workers=1)
    logq, s = cp.REF_SHAPE["logq"], cp.REF_SHAPE["logdelta"]
    ct, q = out["ct"], 1 << cp.REF_SHAPE["logq"]
    n = len(ct[0])
    for a, b in cp.REF_CONSTANTS:
        prod, rs, addpt, subpt = out[(a, b)]
        m = cp.const_plaintext(n, a, b)
        assert [list(c) for c in prod] == cp.closed_mulpt(ct, a, b, logq), (a, b)
        assert [list(c) for c in rs] == cp.closed_mulpt(ct, a, b, logq, s), (a, b)
        assert tuple(list(c) for c in addpt) == ref.he_addpt(ct, m, q), (a, b)
        assert tuple(list(c) for c in subpt) == ref.he_subpt(ct, m, q), (a, b)


def _half_away(x):
    """round half away from zero of a Fraction"""
    f = abs(x)
    r = (f.numerator * 2 + f.denominator) // (2 * f.denominator)
    return r if x >= 0 else -r


def test_gpq_const_pt_against_exact_rationals():
    from gpqhe_amd import _native
    lib = _native.load()
    a, b = C.c_int64(), C.c_int64()
    vals = [1.0, 2.0, 0.5, 0.25, -1 / 48, -17 / 80640, 31 / 1451520, -12.0]
    for logdelta in (30, 40, 50):
        for re in vals:
            im = -re / 3
            assert lib.gpq_const_pt(re, im, logdelta, C.byref(a), C.byref(b)) == 0
            assert a.value == _half_away(Fraction(re) * (1 << logdelta)) and b.value == _half_away(Fraction(im) * (1 << logdelta))
    for k in (1, 3, 12345):                                  # ties at logDelta 50: (k + 1/2) 2^-50, exactly representable
        for sign in (1, -1):
            x = sign * (k + 0.5) * 2.0 ** -50
            assert lib.gpq_const_pt(x, -x, 50, C.byref(a), C.byref(b)) == 0
            assert a.value == sign * (k + 1) and b.value == -sign * (k + 1)
    assert lib.gpq_const_pt(-(2.0 ** 13), 0.0, 50, C.byref(a), C.byref(b)) == 0 and a.value == -(1 << 63)
    a.value = b.value = 77
    for re, im in ((2.0 ** 14, 0.0), (0.0, -(2.0 ** 14)), (2.0 ** 13, 0.0), (float("inf"), 0.0), (0.0, float("nan"))):
        assert lib.gpq_const_pt(re, im, 50, C.byref(a), C.byref(b)) != 0
        assert (a.value, b.value) == (77, 77)
