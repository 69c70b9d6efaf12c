"""Shared by the constant-plaintext tests: the closed form of he_mulpt / he_rs / he_addpt / he_subpt by he_const_pt's plaintext
a + b x^(n/2) (src/he-encode.c:119-125) in Python integers, the exactness predicate, and the inputs the tests run on."""
import random

from oracle import bigint_ref as ref

LOGP = 59                                                   # GPQHE_LOGP
# (logql, lognu): q_l = 2^logql, pt->nu = Delta = 2^lognu
SHAPES = [(27, 17), (63, 30), (64, 30), (65, 40), (88, 30), (200, 40), (438, 50), (850, 50), (1000, 60)]
BIG = ((1 << 62) + 12345, -(1 << 63))                       # wraps he_mulpt's basis at logql <= 65


def mulpt_dim(logql, lognu, logn):
    """src/he-mult.c:168 for q_l = 2^logql (nbits = logql + 1) and nu = 2^lognu"""
    return (logql + 1 + lognu + logn) // LOGP + 1


def constants(lognu, seed):
    """the first six (a, b) of the issue's list"""
    rng = random.Random(seed)
    r = lambda bits: rng.randrange(1 << (bits - 1), 1 << bits) * rng.choice((1, -1))
    return [(1, 0), (0, 1), (-1, 0), (0, -1), (r(lognu), 0), (r(lognu), r(lognu))]


def shifts(logql, lognu):
    return sorted({0, 1, min(lognu, logql - 2)})


def fits(primes, a, b, logql, dim):
    """(|a| + |b|) 2^(logql-1) < floor(P_dim / 2): |v| stays below half the basis for inputs centred mod 2^logql"""
    P = 1
    for p in primes[:dim]:
        P *= int(p)
    return (abs(a) + abs(b)) << (logql - 1) < P // 2


def closed_v(c, a, b):
    """c * (a + b x^h) in Z[x]/(x^n + 1)"""
    n = len(c)
    h = n // 2
    return [a * c[k] - b * c[k + h] for k in range(h)] + [a * c[k] + b * c[k - h] for k in range(h, n)]


def closed_mulpt(ct, a, b, logql, s=0):
    """he_mulpt, then -- s != 0 -- he_rs by 2^s (src/he-rescale.c:33-54)"""
    q = 1 << logql
    out = []
    for c in ct:
        v = [ref.mpi_smod(x, q) for x in closed_v(c, a, b)]
        if s:
            v = [ref.mpi_smod(ref.mpi_rdiv(x, 1 << s), q >> s) for x in v]
        out.append(v)
    return out


def closed_mulpt_no_inner_smod(ct, a, b, logql, s):
    """the form the kernel computes for s >= 1: bits [s, logql) of v plus the rounding carry, sign from result bit logql - s - 1"""
    return [[ref.mpi_smod(ref.mpi_rdiv(x, 1 << s), 1 << (logql - s)) for x in closed_v(c, a, b)] for c in ct]


def ref_rs(ct, s, logql):
    """he_rs on the reference's he_mulpt output"""
    return [[ref.mpi_smod(ref.mpi_rdiv(x, 1 << s), 1 << (logql - s)) for x in c] for c in ct]


def const_plaintext(n, a, b):
    m = [0] * n
    m[0], m[n // 2] = a, b
    return m


def centred_inputs(n, logql, seed):
    """one polynomial centred mod 2^logql: the edge values at 0..4 and h..h+4, the rest seeded random"""
    rng = random.Random(seed)
    half = 1 << (logql - 1)
    edge = [half - 1, -half, 0, 1, -1]
    c = [rng.randrange(-half, half) for _ in range(n)]
    h = n // 2
    c[0:5] = edge
    c[h:h + 5] = edge
    return c


def tie_inputs(n, logql, s, seed):
    """for a = 1, b = 0: coefficients whose low s bits are exactly 2^(s-1) (the tie: rounds down), 2^(s-1) + 1 (up) and 2^(s-1) - 1 (down),
    of both signs, repeated over the polynomial on random high parts"""
    rng = random.Random(seed)
    half = 1 << (logql - 1)
    t = 1 << (s - 1)
    lows = [t, t + 1, t - 1] if s > 1 else [1, 0, 1]
    c = []
    for i in range(n):
        hi = rng.randrange(0, half >> s) << s
        v = hi | lows[i % 3]
        c.append(v if (i // 3) % 2 == 0 else v - half)       # v - half is negative with the same low s bits (s < logql - 1)
    return c


# the executed reference (oracle.ref.run: a worker process, one context)
REF_SHAPE = dict(logn=6, logq=88, logdelta=30, slots=4)
REF_CONSTANTS = [(1, 0), (0, 1), (-3, 0), (0x2B3C4D5E | (1 << 29), -(0x9ABCDEF | (1 << 27))), (-12 << 30, 0)]


def reference_job(arg):
    """he_mulpt, he_rs, he_addpt, he_subpt of the reference itself by the plaintexts a + b x^(n/2): {(a, b): (mulpt, rs, addpt, subpt)}"""
    from oracle import ref as oref
    logn, logq, logdelta, slots = (REF_SHAPE[k] for k in ("logn", "logq", "logdelta", "slots"))
    R = oref.Ref().init(logn, 1 << logq, slots, 1 << logdelta)
    n, L = R.n, R.Lmax
    ct = (centred_inputs(n, logq, 11), centred_inputs(n, logq, 12))
    out = {"ct": ct}
    for a, b in arg:
        R.ct_set(0, ct, L, float(1 << logdelta), 1.0)
        R.pt_set(0, const_plaintext(n, a, b), float(1 << logdelta))
        R.he_mulpt(1, 0, 0)
        prod = R.ct_get(1)[0]
        R.he_rs(1)
        rs = R.ct_get(1)[0]
        R.he_addpt(2, 0, 0)
        R.he_subpt(3, 0, 0)
        out[(a, b)] = (prod, rs, R.ct_get(2)[0], R.ct_get(3)[0])
    return out
