"""numpy restatement of the reference's decoder: `decode` (src/he-encode.c:66-74) with `canemb` (src/canemb.c:43-60) and `mpi_to_double`
(src/types.c:77-106).

The discipline of tests/ecd_model.py: real and imaginary parts live in separate float64 arrays and EVERY product, sum, difference and
quotient is one ufunc call of its own, so that no operation can be fused with another -- the arithmetic of the reference compiled by gcc
for x86-64 without fused multiply-add.  The roots come from a table argument T[t] = (cos, sin)(2 pi t / (4 S)), a (4 S + 1) x 2 array for
S >= slots slots read by stride (the reference's polyctx.ring.zetas[t m / (4 S)]).

`mpi_to_double` is a closed form on Python integers.  The reference runs `num = num * 2 + bit` from the top bit down in double arithmetic:
for a magnitude of L <= 53 bits that is exact; beyond, the first 53 bits M are exact, the 54th bit b makes 2 M + b -- a tie, which
round-to-nearest-even resolves to the even mantissa: M' = M + (b & M & 1) -- and every later bit is at most a quarter of the last place
and rounds away.  The result is M' 2^(L - 53), +inf from 2^1024, the sign applied last.  tests/test_ref_dcd.py holds model + table
against the executed reference bit for bit.  `decode` takes the conversion, the quotient and the real part of the complex product as
arguments, so that the tests can show what a differently rounded decoder would have given on the recorded inputs."""
import math

import numpy as np

from tests.ecd_model import bit_reverse


def mpi_to_double(v):
    """src/types.c:77-106 on a Python integer"""
    a = abs(int(v))
    L = a.bit_length()
    if L <= 53:
        num = float(a)
    else:
        M, b = a >> (L - 53), (a >> (L - 54)) & 1
        M += b & M & 1
        try:
            num = math.ldexp(float(M), L - 53)
        except OverflowError:
            num = math.inf
    return -num if v < 0 else num


def to_double_nearest(v):
    """what a correctly rounded conversion gives (NOT the reference)"""
    return float(int(v))


def to_double_truncating(v):
    """what a truncating conversion gives (NOT the reference)"""
    a = abs(int(v))
    L = a.bit_length()
    num = float(a) if L <= 53 else math.ldexp(float(a >> (L - 53)), L - 53)
    return -num if v < 0 else num


def product_real(br, bi, c, s):
    """the real part of (br + i bi)(c + i s): two products and one difference, each rounded"""
    return np.subtract(np.multiply(br, c), np.multiply(bi, s))


def canemb(re, im, T, real_part=product_real):
    """src/canemb.c:43-60 on [count][slots] arrays, returned as new arrays"""
    re, im = np.array(re, dtype=np.float64, ndmin=2), np.array(im, dtype=np.float64, ndmin=2)
    count, slots = re.shape
    S = (T.shape[0] - 1) // 4
    assert T.shape == (4 * S + 1, 2) and S % slots == 0, "a table for %d slots does not serve %d" % (S, slots)
    stride = S // slots
    pow5 = [1]
    for _ in range(max(slots // 2, 1) - 1):
        pow5.append(pow5[-1] * 5 % (4 * slots))                               # cyc_group[j] mod 4 slots
    pow5 = np.array(pow5, dtype=np.int64)
    perm = bit_reverse(slots)
    re, im = np.ascontiguousarray(re[:, perm]), np.ascontiguousarray(im[:, perm])   # :45
    length = 2
    while length <= slots:
        mid, idx_mod = length // 2, 4 * length
        k = (pow5[:mid] % idx_mod) * (4 * slots // idx_mod) * stride          # :52, in units of this table
        c, s = T[k, 0], T[k, 1]
        R, I = re.reshape(count, slots // length, length), im.reshape(count, slots // length, length)
        ur, ui, br, bi = R[:, :, :mid].copy(), I[:, :, :mid].copy(), R[:, :, mid:].copy(), I[:, :, mid:].copy()
        vr = real_part(br, bi, c, s)                                          # :54: (br + i bi)(c + i s), four products, two sums
        vi = np.add(np.multiply(br, s), np.multiply(bi, c))
        R[:, :, :mid] = np.add(ur, vr)                                        # :55
        I[:, :, :mid] = np.add(ui, vi)
        R[:, :, mid:] = np.subtract(ur, vr)                                   # :56
        I[:, :, mid:] = np.subtract(ui, vi)
        length *= 2
    return re, im


def decode(coeffs, T, slots, nu, to_double=mpi_to_double, quotient=np.divide, real_part=product_real):
    """coeffs: [count][n] Python integers (the plaintext polynomials) -> float64 [count][slots][2], the (re, im) pairs of he_dcd"""
    n = len(coeffs[0])
    nh, gap = n // 2, n // 2 // slots
    with np.errstate(all="ignore"):
        re = np.array([[to_double(p[i * gap]) for i in range(slots)] for p in coeffs], dtype=np.float64)
        im = np.array([[to_double(p[i * gap + nh]) for i in range(slots)] for p in coeffs], dtype=np.float64)
        re, im = quotient(re, np.float64(nu)), quotient(im, np.float64(nu))   # src/he-encode.c:72
        re, im = canemb(re, im, T, real_part)
    return np.ascontiguousarray(np.stack([re, im], axis=-1))


def bits(z):
    """the 64-bit patterns of an array of doubles"""
    return np.ascontiguousarray(z, dtype=np.float64).view(np.uint64)


def words(coeffs, W):
    """[count][n] Python integers -> the big slab uint64 [count][W][n]: two's complement over 64 W bits, little-endian words"""
    mask, wrap = (1 << 64) - 1, 1 << (64 * W)
    out = np.empty((len(coeffs), W, len(coeffs[0])), dtype=np.uint64)
    for k, p in enumerate(coeffs):
        for i, v in enumerate(p):
            assert -(wrap >> 1) <= v < (wrap >> 1), "a coefficient of %d bits does not fit %d words" % (int(v).bit_length(), W)
            u = int(v) % wrap
            for j in range(W):
                out[k, j, i] = (u >> (64 * j)) & mask
    return out
