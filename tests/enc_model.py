"""Python-integer and numpy model of the reference's samplers and encryptor: what tests/test_he_samplers_gpu.py and tests/test_he_enc_gpu.py
hold the device against, and what tests/test_ref_enc.py holds against the executed reference.

  sample_zo        src/sample.c:112-131   n/4 bytes; bit 2i of their little-endian integer clear -> 0, else bit 2i+1 clear -> +1, else -1
  sample_error     src/sample.c:60-82     n bytes; (coeff[i], coeff[i+1]) = T[buf[i]][buf[i+1]] for even i, T = gauss_table()
  sample_uniform   src/sample.c:133-141   nbits/8 + 1 bytes per coefficient, the low nbits bits of their little-endian integer (raw)
  sample_hwt       src/sample.c:84-100    8 bytes of signs, then 8 bytes per draw until 64 distinct positions are set
  he_keypair       src/he-kem.c:43-71     sample_sk, sample_error, sample_uniform(q_L)
  he_enc_sk        src/he-encrypt.c:75-103   sample_error, sample_uniform(q)
  he_enc_pk        src/he-encrypt.c:37-73    sample_zo, sample_error, sample_error
  he_dec           src/he-encrypt.c:105-125
The products go through the restated poly_mul (oracle.oracle's limb loop, oracle.bigint_ref's poly_rns2mpi), so a product that wraps the
dim-limb basis follows the reference.  The samplers take their bytes from a `Stream`, which counts what they consume."""
import math

import numpy as np

from oracle import bigint_ref as br

PI = 3.141592653589793238462643383279502884          # src/params.h:52
SIGMA = 3.1915382432114616                           # src/params.h:55


class Stream:
    """the caller's random bytes, consumed in order (the reference's randombytes)"""

    def __init__(self, data, pos=0):
        self.data, self.pos = np.ascontiguousarray(data, dtype=np.uint8), pos

    def take(self, count):
        assert self.pos + count <= self.data.size, "the stream holds %d bytes, %d are asked for" % (self.data.size, self.pos + count)
        out = self.data[self.pos:self.pos + count]
        self.pos += count
        return out


_TABLE = None


def gauss_table():
    """int8 [65536][2]: T[b0 * 256 + b1] = ((int16_t)floor(rr cos(theta) + 0.5), (int16_t)floor(rr sin(theta) + 0.5)), theta = 2 PI b0 / 256,
    rr = sqrt(-2 log(b1 / 256)) SIGMA; (0, 0) for b1 = 0, where log 0 = -inf makes the C conversion undefined and the executed reference
    gives 0.  `margin` (gauss_margin) is the distance of floor's argument from the nearest integer."""
    global _TABLE
    if _TABLE is None:
        T = np.zeros((65536, 2), dtype=np.int8)
        for b0 in range(256):
            theta = 2 * PI * (b0 / 256)
            cs, sn = math.cos(theta), math.sin(theta)
            for b1 in range(1, 256):
                rr = math.sqrt(-2 * math.log(b1 / 256)) * SIGMA
                T[b0 * 256 + b1] = (math.floor(rr * cs + 0.5), math.floor(rr * sn + 0.5))
        _TABLE = T
    return _TABLE


def gauss_margin():
    """the smallest distance of floor's argument from an integer over the 65280 defined entries"""
    best = 1.0
    for b0 in range(256):
        theta = 2 * PI * (b0 / 256)
        for b1 in range(1, 256):
            rr = math.sqrt(-2 * math.log(b1 / 256)) * SIGMA
            for t in (rr * math.cos(theta) + 0.5, rr * math.sin(theta) + 0.5):
                best = min(best, abs(t - round(t)))
    return best


def zo_from_bytes(buf, n):
    """int8 [n] from n/4 bytes"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    assert n >= 4 and buf.size == n // 4
    two = (buf[:, None] >> (2 * np.arange(4, dtype=np.uint8))[None, :]) & 3             # bits (2i, 2i+1) of the little-endian integer
    return np.where(two & 1, np.where(two & 2, -1, 1), 0).astype(np.int8).reshape(-1)


def error_from_bytes(buf, n):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    assert buf.size == n and n % 2 == 0
    return gauss_table()[buf[0::2].astype(np.int64) * 256 + buf[1::2]].reshape(-1)


def uniform_from_bytes(buf, n, nbits):
    """[n] Python integers in [0, 2^nbits) from n (nbits/8 + 1) bytes"""
    nb = nbits // 8 + 1
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    assert buf.size == n * nb
    mask = (1 << nbits) - 1
    return [int.from_bytes(buf[i * nb:(i + 1) * nb].tobytes(), "little") & mask for i in range(n)]


def sample_zo(stream, n):
    return zo_from_bytes(stream.take(n // 4), n)


def sample_error(stream, n):
    return error_from_bytes(stream.take(n), n)


def sample_uniform(stream, n, q):
    nbits = int(q).bit_length()
    return uniform_from_bytes(stream.take(n * (nbits // 8 + 1)), n, nbits)


def sample_hwt(stream, n):
    """sample_sk: [n] coefficients in {-1, 0, 1} with 64 non-zero ones"""
    num = int.from_bytes(stream.take(8).tobytes(), "little")
    logn = n.bit_length() - 1
    vec, idx = [0] * n, 0
    while idx < 64:
        i = int.from_bytes(stream.take(8).tobytes(), "little") & ((1 << logn) - 1)     # loadnbits_littleendian(buf, logm), src/types.c:144-164
        if vec[i] == 0:
            vec[i] = 1 if (num >> idx) & 1 == 0 else -1
            idx += 1
    return vec


def poly_mul(o, a, b, dim, q):
    """src/poly.c:84-107 on lists of Python integers with the oracle context o (at least dim primes)"""
    prod = o.poly_mul_rns(br._slab(o, a, dim), br._slab(o, b, dim), dim)
    return br.poly_rns2mpi(br._limbs(prod, dim, o.n), br.RnsBasis(o.p[:dim]), q)


def he_dim(logn, q):
    return (int(q).bit_length() + logn) // 59 + 1                        # hectx.dim, src/precomp.c:401


def enc_sk_from(o, m, a, e, sk, dim, q):
    """(c0, c1) of src/he-encrypt.c:91-98 from the sampled polynomials; m = None: he_keypair's (p0, p1), src/he-kem.c:59-65"""
    x = poly_mul(o, a, sk, dim, q)
    c0 = [br.mpi_smod((-x[i] + (m[i] if m is not None else 0) + int(e[i])) % q, q) for i in range(o.n)]
    return c0, [br.mpi_smod(v, q) for v in a]


def enc_pk_from(o, m, v, e0, e1, pk, dim, q):
    """(c0, c1) of src/he-encrypt.c:58-66 from the sampled polynomials"""
    vi = [int(t) for t in v]
    x0, x1 = poly_mul(o, pk[0], vi, dim, q), poly_mul(o, pk[1], vi, dim, q)
    c0 = [br.mpi_smod((x0[i] + (m[i] if m is not None else 0) + int(e0[i])) % q, q) for i in range(o.n)]
    return c0, [br.mpi_smod((x1[i] + int(e1[i])) % q, q) for i in range(o.n)]


def he_keypair(o, stream, q):
    """(pk = (p0, p1), sk) as src/he-kem.c:43-71 draws and computes them"""
    n = o.n
    sk = sample_hwt(stream, n)
    e = sample_error(stream, n)
    a = sample_uniform(stream, n, q)
    return enc_sk_from(o, None, a, e, sk, he_dim(o.logn, q), q), sk


def he_enc_sk(o, stream, m, sk, q):
    n = o.n
    e = sample_error(stream, n)
    a = sample_uniform(stream, n, q)
    return enc_sk_from(o, m, a, e, sk, he_dim(o.logn, q), q)


def he_enc_pk(o, stream, m, pk, q):
    n = o.n
    v = sample_zo(stream, n)
    e0 = sample_error(stream, n)
    e1 = sample_error(stream, n)
    return enc_pk_from(o, m, v, e0, e1, pk, he_dim(o.logn, q), q)


def he_dec(o, ct, sk, q):
    dim = int(q).bit_length() // 59 + 1                                  # src/he-encrypt.c:113
    x = poly_mul(o, ct[1], sk, dim, q)
    return [br.mpi_smod((x[i] + ct[0][i]) % q, q) for i in range(o.n)]
