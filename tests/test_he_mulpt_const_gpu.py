"""gpq_he_mulpt_const / gpq_he_addpt_const -- he_mulpt [+ he_rs], he_addpt and he_subpt by he_const_pt's plaintext a + b x^(n/2) as one pass
over the big slabs -- against the restated reference (oracle/bigint_ref.py: the plaintext as a dense polynomial through the RNS path) and
the closed form of tests/const_pt_cases.py."""
import random

import numpy as np
import pytest

from gpqhe_amd import big_to_ints, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref
from tests import const_pt_cases as cp

pytestmark = pytest.mark.gpu

LOGN = 6
GPQ_ERR_INVALID = -1                                        # include/gpqhe_hip.h
DIMUB = max(cp.mulpt_dim(logql, lognu, LOGN) for logql, lognu in cp.SHAPES)


def _torch():
    import torch
    return torch


class Device:
    """the two calls on lists of ciphertexts ((c0, c1) of Python ints); returns the outputs the same way"""

    def __init__(self, g):
        self.g = g

    def _up(self, cts, W):
        return [to_device(np.concatenate([ints_to_big(ct[i], W) for ct in cts])) for i in range(2)]

    def _down(self, o0, o1, W, batch):
        n = self.g.n
        r0, r1 = big_to_ints(to_host(o0), W, n), big_to_ints(to_host(o1), W, n)
        return [[r0[k], r1[k]] for k in range(batch)]

    def mul(self, cts, a, b, W, logql, dim, s=0, in_place=False, count_bad=False):
        torch = _torch()
        d0, d1 = self._up(cts, W)
        o0, o1 = (d0, d1) if in_place else (torch.full_like(d0, 0x5A5A5A5A), torch.full_like(d1, 0x5A5A5A5A))
        bad = torch.zeros(1, dtype=torch.int32, device=d0.device) if count_bad else None
        self.g.he_mulpt_const(o0, o1, d0, d1, a, b, W, logql, dim, s, bad)
        out = self._down(o0, o1, W, len(cts))
        if not in_place:
            assert self._down(d0, d1, W, len(cts)) == [[list(c) for c in ct] for ct in cts], "the inputs changed"
        return out, (int(bad.item()) if count_bad else None)

    def refused(self, cts, a, b, W, logql, dim, s=0):
        """the call must fail with GPQ_ERR_INVALID and leave the outputs as they were"""
        torch = _torch()
        d0, d1 = self._up(cts, W)
        o0, o1 = torch.full_like(d0, 0x5A5A5A5A), torch.full_like(d1, 0x5A5A5A5A)
        rc = self.g.lib.gpq_he_mulpt_const(self.g.h, self.g._ptr(o0), self.g._ptr(o1), self.g._ptr(d0), self.g._ptr(d1), a, b, W, logql, dim, s,
                                           len(cts), None, self.g._stream())
        torch.cuda.synchronize()
        return rc, bool((o0 == 0x5A5A5A5A).all()) and bool((o1 == 0x5A5A5A5A).all())

    def fits(self, a, b, logql, dim):
        return self.g.he_mulpt_const_fits(a, b, logql, dim)

    def add(self, cts, a, b, W, logql, sub, in_place=False):
        torch = _torch()
        d0, d1 = self._up(cts, W)
        o0, o1 = (d0, d1) if in_place else (torch.full_like(d0, 0x5A5A5A5A), torch.full_like(d1, 0x5A5A5A5A))
        self.g.he_addpt_const(o0, o1, d0, d1, a, b, W, logql, sub)
        return self._down(o0, o1, W, len(cts))


@pytest.fixture
def dev(engine_ctx):
    return lambda logn, nprimes: Device(engine_ctx(logn, nprimes))


def _mul_shifts(logql, lognu):
    s = set(cp.shifts(logql, lognu))
    if 63 < logql:
        s.add(63)
    if logql >= 200:
        s |= {64, 70}
    return sorted(s)


@pytest.mark.parametrize("logql,lognu", cp.SHAPES)
def test_parity_with_the_restated_reference(dev, oracle_ctx, logql, lognu):
    d, o = dev(LOGN, DIMUB), oracle_ctx(LOGN, DIMUB)
    n, W, dim = o.n, (logql + 63) // 64, cp.mulpt_dim(logql, lognu, LOGN)
    ct = [cp.centred_inputs(n, logql, 5 * logql), cp.centred_inputs(n, logql, 5 * logql + 1)]
    consts = cp.constants(lognu, logql) + ([cp.BIG] if cp.fits(o.p, *cp.BIG, logql, dim) else [])
    assert len(consts) == (7 if logql > 65 else 6)
    for a, b in consts:
        assert d.fits(a, b, logql, dim)
        want = ref.he_mulpt(o, ct, cp.const_plaintext(n, a, b), dim, logql)
        for s in _mul_shifts(logql, lognu):
            exp = cp.ref_rs(want, s, logql) if s else want
            (got,), bad = d.mul([ct], a, b, W, logql, dim, s, count_bad=True)
            assert got == exp, (a, b, s)
            assert bad == 0, (a, b, s)


@pytest.mark.parametrize("s", [1, 40, 63])
def test_rounding_ties(dev, s):
    logql, dim = 200, cp.mulpt_dim(200, 40, LOGN)
    d = dev(LOGN, DIMUB)
    ct = [cp.tie_inputs(d.g.n, logql, s, 40 + s), cp.tie_inputs(d.g.n, logql, s, 41 + s)]
    exp = cp.closed_mulpt(ct, 1, 0, logql, s)
    t = 1 << (s - 1)
    if s > 1:                                               # the inputs are what they claim: tie down, above up, below down
        q = [ref.mpi_rdiv(v, 1 << s) - (v >> s) for v in ct[0][:3]]
        assert [v & ((1 << s) - 1) for v in ct[0][:3]] == [t, t + 1, t - 1] and q == [0, 1, 0]
    (got,), bad = d.mul([ct], 1, 0, 4, logql, dim, s, count_bad=True)
    assert got == exp and bad == 0
    (got,), _ = d.mul([ct], -1, 0, 4, logql, dim, s)       # the other sign of every coefficient
    assert got == cp.closed_mulpt(ct, -1, 0, logql, s)


def test_in_place_batch_and_wider_slabs(dev):
    logql, lognu = 200, 40
    dim = cp.mulpt_dim(logql, lognu, LOGN)
    d = dev(LOGN, DIMUB)
    n = d.g.n
    cts = [[cp.centred_inputs(n, logql, 100 + 2 * k), cp.centred_inputs(n, logql, 101 + 2 * k)] for k in range(3)]
    for a, b in cp.constants(lognu, 77)[4:] + [cp.BIG]:
        for s in (0, 40, 70):
            exp = [cp.closed_mulpt(ct, a, b, logql, s) for ct in cts]
            for W in (4, 5):                                # 5: a word that holds sign extension only
                assert d.mul(cts, a, b, W, logql, dim, s)[0] == exp, (a, b, s, W)
                assert d.mul(cts, a, b, W, logql, dim, s, in_place=True)[0] == exp, (a, b, s, W, "in place")


def test_several_workgroups_per_polynomial(dev):
    logn, logql, lognu = 11, 200, 40
    dim = cp.mulpt_dim(logql, lognu, logn)
    d = dev(logn, dim)
    n = d.g.n
    cts = [[cp.centred_inputs(n, logql, 200 + 2 * k), cp.centred_inputs(n, logql, 201 + 2 * k)] for k in range(2)]
    for a, b in cp.constants(lognu, 78)[4:]:
        exp = [cp.closed_mulpt(ct, a, b, logql, lognu) for ct in cts]
        got, bad = d.mul(cts, a, b, 4, logql, dim, lognu, count_bad=True)
        assert got == exp and bad == 0, (a, b)
        assert d.mul(cts, a, b, 4, logql, dim, lognu, in_place=True)[0] == exp, (a, b)
    m = (-(1 << 39) + 12345, 0)
    for sub in (False, True):
        exp = [list((ref.he_subpt if sub else ref.he_addpt)(ct, cp.const_plaintext(n, *m), 1 << logql)) for ct in cts]
        assert d.add(cts, m[0], m[1], 4, logql, sub) == exp


def test_refusal_and_fits(dev, oracle_ctx):
    d, o = dev(LOGN, DIMUB), oracle_ctx(LOGN, DIMUB)
    n = o.n
    for logql, lognu in cp.SHAPES:
        dim, W = cp.mulpt_dim(logql, lognu, LOGN), (logql + 63) // 64
        for a, b in cp.constants(lognu, logql) + [cp.BIG]:
            assert d.fits(a, b, logql, dim) == cp.fits(o.p, a, b, logql, dim), (logql, a, b)
        if logql <= 65:
            assert not cp.fits(o.p, *cp.BIG, logql, dim)
            ct = [cp.centred_inputs(n, logql, 9), cp.centred_inputs(n, logql, 10)]
            for s in (0, 1):
                rc, untouched = d.refused([ct], *cp.BIG, W, logql, dim, s)
                assert rc == GPQ_ERR_INVALID
                assert untouched
    P = int(o.p[0])                                         # the boundary on one limb
    top = (P // 2) >> 9
    assert d.fits(top - 1, 0, 10, 1) and d.fits(0, -(top - 1), 10, 1) and not d.fits(top + 1, 0, 10, 1)
    assert d.fits(top, 0, 10, 1) == cp.fits(o.p, top, 0, 10, 1)
    assert d.fits(-(1 << 63), -(1 << 63), 1000, DIMUB) == cp.fits(o.p, -(1 << 63), -(1 << 63), 1000, DIMUB)


@pytest.mark.parametrize("a,b", [(12345, 0), (-7, 3)])
def test_input_check_counts_non_centred_coefficients(dev, a, b):
    logql, W = 200, 4
    dim = cp.mulpt_dim(logql, 40, LOGN)
    d = dev(LOGN, DIMUB)
    n = d.g.n
    ct = [cp.centred_inputs(n, logql, 31), cp.centred_inputs(n, logql, 32)]
    ct[0][7] = 1 << 199                                     # one past the largest centred value
    ct[0][n // 2 + 9] = -(1 << 199) - 1
    ct[1][20] = (1 << 230) + 5
    for s in (0, 40):
        (got,), bad = d.mul([ct], a, b, W, logql, dim, s, count_bad=True)
        assert bad == 3
        assert got == cp.closed_mulpt(ct, a, b, logql, s)


ADD_SHAPES = [(1, 63), (1, 64), (2, 63), (2, 64), (2, 65), (2, 128), (14, 63), (14, 64), (14, 65), (14, 850), (14, 896)]


@pytest.mark.parametrize("W,logql", ADD_SHAPES)
def test_addpt_subpt(dev, W, logql):
    d = dev(LOGN, DIMUB)
    n = d.g.n
    rng = random.Random(64 * W + logql)
    lim = 1 << (64 * W - 1)
    cts = [[[rng.randrange(-lim, lim) for _ in range(n)] for _ in range(2)] for _ in range(3)]      # any W-word values
    cts[0][0][0], cts[0][0][n // 2], cts[1][0][0], cts[2][0][n // 2] = lim - 1, -lim, -1, (1 << (logql - 1)) - 1
    q = 1 << logql
    for a, b in [(1, 0), (0, -1), (rng.randrange(1 << 50), -rng.randrange(1 << 50)), (-(1 << 63), (1 << 63) - 1)]:
        m = cp.const_plaintext(n, a, b)
        for sub, f in ((False, ref.he_addpt), (True, ref.he_subpt)):
            exp = [list(f(ct, m, q)) for ct in cts]
            assert d.add(cts, a, b, W, logql, sub) == exp, (a, b, sub)
            assert d.add(cts, a, b, W, logql, sub, in_place=True) == exp, (a, b, sub, "in place")
