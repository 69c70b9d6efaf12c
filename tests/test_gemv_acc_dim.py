"""Planned he_gemv, the host-only part (include/gpqhe_hip.h, "he_gemv with a plan"):

* gpq_gemv_acc_dim against its inequality evaluated with Python integers -- the smallest d with
  logql - 1 + diag_bits + logn + ceil(log2 n1) + 1 <= 59 d -- over a sweep, including shapes where it equals the reference's dimpt
  (src/he-mult.c:168) and shapes where it is one more;
* the integer model of gemv_mac's accumulation (gpqhe_amd/csrc/ntt_kernels.hpp): products of words in [0, p] leave mulmod_lazy in (0, 4p),
  the running sum stays below 4p with one conditional subtraction per term and never wraps 64 bits, for n1 = 511 terms (the reference's
  n1 <= sqrt(2 slots), slots <= n / 2 <= 2^16) and the extreme c of the prime family.
CPU only; the kernel itself is checked on the GPU (tests/test_gemv_inner_gpu.py)."""
import random

import pytest

from gpqhe_amd import gemv_acc_dim

M64 = (1 << 64) - 1
FOLD_CMAX = 319000000    # GPQ_FOLD_CMAX


def _smallest_d(logql, diag_bits, logn, n1):
    bound = 1 << (logql - 1 + diag_bits + logn + (n1 - 1).bit_length())       # |S| < bound
    d = 1
    while 2 * bound > 1 << (59 * d):                                          # 2 |S| < 2^(59 d) < P
        d += 1
    return d


def test_acc_dim_is_the_smallest_basis_that_holds_the_sum():
    for logql in (1, 2, 30, 59, 60, 118, 120, 135, 176, 177, 178, 438, 850, 1000):
        for diag_bits in (0, 1, 29, 30, 31, 32, 33, 60, 64):
            for logn in (1, 10, 13, 14, 16, 17):
                for n1 in (1, 2, 3, 4, 5, 8, 9, 16, 255, 256, 257, 511):
                    assert gemv_acc_dim(logql, diag_bits, logn, n1) == _smallest_d(logql, diag_bits, logn, n1), (logql, diag_bits, logn, n1)


def _dimpt(logql, logdelta, logn):
    return (logql + 1 + logdelta + logn) // 59 + 1           # src/he-mult.c:168 with nu = 2^logdelta


def test_acc_dim_against_the_reference_limb_count():
    # the measured shapes: the sum fits the reference's own basis
    assert gemv_acc_dim(438, 30, 14, 4) == _dimpt(438, 30, 14) == 9
    assert gemv_acc_dim(850, 30, 16, 8) == _dimpt(850, 30, 16) == 16
    # logn 10, q = 2^135, 30-bit diagonals: 135 + 31 + 10 = 176 = 2 * 59 + 58, so dimpt = 3 with one spare bit; eight terms need a fourth limb
    assert _dimpt(135, 30, 10) == 3
    assert gemv_acc_dim(135, 30, 10, 1) == 3
    assert gemv_acc_dim(135, 30, 10, 2) == 3
    assert gemv_acc_dim(135, 30, 10, 8) == 4
    # never below what one product needs
    for logql in range(60, 900, 7):
        for logn in (10, 14, 16):
            for n1 in (1, 4, 8, 23):
                d = gemv_acc_dim(logql, 30, logn, n1)
                assert d >= gemv_acc_dim(logql, 30, logn, 1) and d <= gemv_acc_dim(logql, 30, logn, 1) + 1


def mulmod_raw(a, w, c):
    """mulmod_raw_t() of modarith.hpp: T' with a w == T' + (c + 1) (mod p); asserts what the device code relies on."""
    a0, a1, w0, w1 = a & 0xFFFFFFFF, a >> 32, w & 0xFFFFFFFF, w >> 32
    assert a1 < (1 << 32) and w1 < (1 << 32)
    m00 = a0 * w0
    mid = a0 * w1 + (m00 >> 32)
    assert mid <= M64
    mid = a1 * w0 + mid
    assert mid <= M64
    hi = a1 * w1 + (mid >> 32)
    assert hi <= M64
    x = a * w
    xh, xl = x >> 59, x & ((1 << 59) - 1)
    assert xh < (1 << 64) and xh == ((hi << 5) | ((mid & 0xFFFFFFFF) >> 27))
    t = c * xh
    th, tl = t >> 59, t & ((1 << 59) - 1)
    assert th < (1 << 32)
    r = c * th + xl + ((1 << 59) - 1 - tl)
    assert r <= M64
    return r


@pytest.mark.parametrize("c", [1 + 2048, 4849665, 134217000, 306000000 - 1, FOLD_CMAX - 1])
def test_accumulation_stays_below_4p_and_is_exact_for_511_terms(c):
    p = (1 << 59) + c
    rnd = random.Random(c)
    edge = [0, 1, 2, p - 2, p - 1, p, (1 << 59) - 1, 1 << 59, (1 << 32) - 1, 1 << 32]
    for trial in range(6):
        acc, exact = 0, 0
        for t in range(511):
            if trial == 0:
                u, d = p, p                                  # the reference's p-for-zero words on both sides
            elif trial == 1:
                u, d = p - 1, p - 1
            elif trial == 2:
                u, d = rnd.choice(edge), rnd.choice(edge)
            else:
                u, d = rnd.randrange(p + 1), rnd.randrange(p + 1)
            prod = mulmod_raw(u, d, c) + c + 1               # mulmod_lazy
            assert 0 < prod < 4 * p and prod % p == u * d % p
            s = acc + prod
            assert s < 8 * p < (1 << 63)                     # no 64-bit wrap
            acc = s - 4 * p if s >= 4 * p else s             # csub4
            assert acc < 4 * p
            exact += u * d
        r = acc
        r = r - 2 * p if r >= 2 * p else r                   # canon4
        r = r - p if r >= p else r
        assert r == exact % p


def test_the_largest_n1_the_reference_can_produce():
    """n1 = floor(sqrt(slots)) or floor(sqrt(2 slots)) (src/he-algo.c:51-54) with slots <= n / 2 = 2^16"""
    from gpqhe_amd import gemv_steps
    assert max(gemv_steps(1 << k)[0] for k in range(17)) <= 511
