"""gpq_automorphism_index (include/gpqhe_hip.h) against the C oracle's forward transform: the map the hoisted rotations rest on.

For g = 5^rot mod 2n (poly_rot, src/poly.c:263-275) and g = 2n - 1 (poly_conj, :277-283), NTT(rot(a))[j] == NTT(a)[sigma(j)] (mod p) in
the reference's forward output order; sigma is a permutation and maps every aligned block of 2^8 or 2^9 outputs onto one aligned block of
inputs (the tiles of keyswitch_rot_mid8x2).  No device: the table is computed on the host."""
import random

import numpy as np
import pytest

import gpqhe_amd
from gpqhe_amd import _native
from oracle import bigint_ref as ref
from oracle.oracle import OracleCtx

ROTS = [0, 1, 2, 3, 7, 15, 40, 1000]


def _g(rot, n):
    return pow(5, rot, 1 << 64) % (2 * n)


@pytest.mark.parametrize("logn", range(7, 15))
def test_sigma_is_the_ntt_domain_rotation(logn):
    o = OracleCtx(logn, 2)
    n = o.n
    rng = random.Random(logn)
    a = [rng.randrange(-(1 << 40), 1 << 40) for _ in range(n)]
    cases = [(rot, _g(rot, n), ref.poly_rot(a, rot)) for rot in ROTS] + [("conj", 2 * n - 1, ref.poly_conj(a))]
    for d in range(2):
        p = o.p[d]
        A = o.ntt(np.array([v % p for v in a], dtype=np.uint64), d).astype(object) % p
        for rot, g, b in cases:
            sigma = gpqhe_amd.automorphism_index(logn, g)
            B = o.ntt(np.array([v % p for v in b], dtype=np.uint64), d).astype(object) % p
            assert np.array_equal(B, A[sigma.astype(np.int64)]), "logn %d rot %s limb %d" % (logn, rot, d)


@pytest.mark.parametrize("logn", range(7, 18))
def test_sigma_is_a_permutation_with_the_block_property(logn):
    n = 1 << logn
    for g in [_g(r, n) for r in ROTS] + [2 * n - 1]:
        s = gpqhe_amd.automorphism_index(logn, g).astype(np.int64)
        assert np.array_equal(np.sort(s), np.arange(n)), "g %d is not a permutation" % g
        for k in (8, 9):
            if k > logn:
                continue
            blocks = s.reshape(-1, 1 << k)
            hi = blocks >> k
            assert (hi == hi[:, :1]).all(), "g %d: a 2^%d block reads two source blocks" % (g, k)
            assert np.array_equal(np.sort(hi[:, 0]), np.arange(n >> k))


def test_identity_and_a_hand_checked_table():
    assert np.array_equal(gpqhe_amd.automorphism_index(7, 1), np.arange(128))
    # logn 2, g 3: brv = [0, 2, 1, 3], exponents 2 brv + 1 = [1, 5, 3, 7] -> x 3 mod 8 = [3, 7, 1, 5] -> brv((e - 1) / 2) = [2, 3, 0, 1]
    assert list(gpqhe_amd.automorphism_index(2, 3)) == [2, 3, 0, 1]


@pytest.mark.parametrize("logn,g", [(7, 0), (7, 2), (10, 5 ** 3 - 1), (0, 5), (18, 5)])
def test_even_g_and_bad_logn_are_rejected(logn, g):
    lib = _native.load()
    idx = np.zeros(1 << min(logn, 17), dtype=np.uint32)
    assert lib.gpq_automorphism_index(logn, g, idx.ctypes.data) == -1
    assert not idx.any()
