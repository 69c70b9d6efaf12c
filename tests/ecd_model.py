"""numpy restatement of the reference's encoder: `encode` (src/he-encode.c:53-64) with `invcanemb` (src/canemb.c:62-81), and `zrotdiag`
(src/he-algo.c:29-43).

Real and imaginary parts live in separate float64 arrays and EVERY product, sum and difference is one ufunc call of its own, so that no
operation can be fused with another: the arithmetic is that of the reference compiled by gcc for x86-64 without fused multiply-add.  The
roots come from a table argument T[t] = (cos, sin)(2 pi t / (4 S)), a (4 S + 1) x 2 array for S >= slots slots read by stride -- the
reference's polyctx.ring.zetas[t m / (4 S)].  `roots_via_sincos` makes that table with the C library's sincos through ctypes, which is what
gcc -O2 turns the reference's `cos(theta) + I*sin(theta)` (src/precomp.c:306-309) into; tests/test_ref_ecd.py holds model + table against
the executed reference word for word."""
import ctypes
import ctypes.util
import math

import numpy as np

PI = 3.141592653589793238462643383279502884              # src/params.h:52


def roots_via_sincos(slots):
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.sincos.restype = None
    libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    m4 = 4 * slots
    T = np.empty((m4 + 1, 2), dtype=np.float64)
    s, c = ctypes.c_double(), ctypes.c_double()
    for t in range(m4):
        libm.sincos(2 * PI * t / m4, ctypes.byref(s), ctypes.byref(c))       # src/precomp.c:307 (2 PI i / m with i = t m / (4 slots): the same double)
        T[t] = (c.value, s.value)
    T[m4] = T[0]                                                              # :310
    return T


def bit_reverse(slots):
    """perm with new[i] = old[perm[i]] for bitrev_vec (src/canemb.c:28-41)"""
    bits = slots.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(slots)], dtype=np.int64)


def invcanemb(re, im, T):
    """src/canemb.c:62-81 on [count][slots] arrays, returned as new arrays"""
    re, im = np.array(re, dtype=np.float64, ndmin=2), np.array(im, dtype=np.float64, ndmin=2)
    count, slots = re.shape
    S = (T.shape[0] - 1) // 4
    assert T.shape == (4 * S + 1, 2) and S % slots == 0, "a table for %d slots does not serve %d" % (S, slots)
    stride = S // slots
    pow5 = [1]
    for _ in range(max(slots // 2, 1) - 1):
        pow5.append(pow5[-1] * 5 % (4 * slots))                               # cyc_group[j] mod 4 slots
    pow5 = np.array(pow5, dtype=np.int64)
    length = slots
    while length >= 2:
        mid, idx_mod = length // 2, 4 * length
        k = (idx_mod - pow5[:mid] % idx_mod) * (4 * slots // idx_mod) * stride  # :70, in units of this table
        c, s = T[k, 0], T[k, 1]
        R, I = re.reshape(count, slots // length, length), im.reshape(count, slots // length, length)
        ar, ai, br, bi = R[:, :, :mid].copy(), I[:, :, :mid].copy(), R[:, :, mid:].copy(), I[:, :, mid:].copy()
        dr, di = np.subtract(ar, br), np.subtract(ai, bi)
        R[:, :, :mid] = np.add(ar, br)                                        # :71
        I[:, :, :mid] = np.add(ai, bi)
        p, q = np.multiply(dr, c), np.multiply(di, s)                         # :72: (dr + i di)(c + i s), four products, two sums
        R[:, :, mid:] = np.subtract(p, q)
        p, q = np.multiply(dr, s), np.multiply(di, c)
        I[:, :, mid:] = np.add(p, q)
        length //= 2
    perm = bit_reverse(slots)
    return np.divide(re[:, perm], float(slots)), np.divide(im[:, perm], float(slots))   # :78-80


def c_round(v):
    """C's round(): half away from zero, exactly (trunc and the fraction are exact)"""
    t = np.trunc(v)
    frac = np.subtract(v, t)
    return np.where(np.abs(frac) >= 0.5, np.add(t, np.copysign(1.0, v)), t)


def encode(z, T, n, logDelta):
    """z: [count][slots] complex128 -> (coefficients int64 [count][n], offending): he_ecd's plaintext polynomials.  A coefficient whose
    rounded value is not finite or reaches 2^63 in magnitude is 0 and counted (the reference is the identity below 2^64 only,
    src/types.c:225-245)."""
    z = np.array(z, dtype=np.complex128, ndmin=2)
    count, slots = z.shape
    with np.errstate(all="ignore"):
        re, im = invcanemb(z.real, z.imag, T)
        delta = math.ldexp(1.0, logDelta)
        vals = [c_round(np.multiply(x, delta)) for x in (re, im)]              # src/he-encode.c:61-62 (the product is exact for a power of two)
    out = np.zeros((count, n), dtype=np.int64)
    gap, offending = n // 2 // slots, 0
    for half, v in enumerate(vals):
        ok = np.isfinite(v) & (np.abs(v) < 2.0 ** 63)
        offending += int((~ok).sum())
        out[:, half * (n // 2):(half + 1) * (n // 2):gap] = np.where(ok, v, 0.0).astype(np.int64)
    return out, offending


def words(coeffs, W):
    """int64 [count][n] -> the big slab uint64 [count][W][n]: W sign-extended little-endian words"""
    coeffs = np.asarray(coeffs, dtype=np.int64)
    out = np.empty((coeffs.shape[0], W, coeffs.shape[1]), dtype=np.uint64)
    out[:, 0] = coeffs.view(np.uint64)
    out[:, 1:] = (coeffs >> 63).view(np.uint64)[:, None, :]
    return out


def max_bits(coeffs):
    return max(int(v).bit_length() for v in (np.asarray(coeffs).max(initial=0), -int(np.asarray(coeffs).min(initial=0))))


def gemv_steps(slots):
    """(n1, n2) of src/he-algo.c:51-54"""
    n1 = int(math.sqrt(slots))
    if slots != n1 * n1:
        n1 = int(math.sqrt(2 * slots))
    return n1, slots // n1


def zrotdiag(A, idx, rot):
    """src/he-algo.c:29-43 on a slots x slots array"""
    A = np.asarray(A)
    m = A.shape[0]
    i = np.arange(m)
    diag = A[i % m, (idx + i) % m]
    return diag[(i + rot) % m]


def diagonal_vectors(A):
    """[slots][slots]: vector i n1 + j = zrotdiag(A, i n1 + j, -i n1), the order of he_gemv's `diag` (src/he-algo.c:63-72)"""
    m = np.asarray(A).shape[0]
    n1, n2 = gemv_steps(m)
    return np.array([zrotdiag(A, i * n1 + j, -(i * n1)) for i in range(n2) for j in range(n1)])
