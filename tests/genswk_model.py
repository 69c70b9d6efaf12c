"""Python-integer model of he_genswk (src/he-kem.c:74-118) and of the structured reduction gpq_he_genswk_batch runs instead of the general
one: what tests/test_genswk_model.py holds against the executed reference and tests/test_he_genswk_batch_gpu.py holds the device against.

  genswk          src/he-kem.c:83-110 from the sampled polynomials: the reference's own operations in its order
  structured      the same key polynomials through the CRT split of M = P 2^k ("Key generation on the device")
  galois_image    the image of a polynomial under X -> X^g (poly_rot: g = 5^rot, src/poly.c:263-275; poly_conj: g = 2n - 1, :277-283)
  window_inputs   coefficients that sit in every window of the structured form: each number of additions of P, the centring bit of h,
                  the compare-and-subtract of the raw p1, and carries over every word boundary of P hs
Python integers only; the storage step (:103-110: rns_decompose + ntt per limb) takes the transform as a callable."""
import random


def smod(r, q):
    """mpi_smod, src/types.c:108-113"""
    r %= q
    return r - q if r >= q // 2 else r


def product_of(primes):
    P = 1
    for p in primes:
        P *= int(p)
    return P


def dimmul_of(P, k, logn):
    return ((P << k).bit_length() + logn) // 59 + 1                       # src/he-kem.c:83


def nbits_of(P, k):
    return (P << k).bit_length()


def negacyclic(a, b):
    """a * b mod x^n + 1 over the integers; zero coefficients of b cost nothing"""
    n = len(a)
    r = [0] * n
    for j, bj in enumerate(b):
        if bj == 0:
            continue
        for i, ai in enumerate(a):
            t = i + j
            if t < n:
                r[t] += ai * bj
            else:
                r[t - n] -= ai * bj
    return r


def rns_product(primes, a, b, dim):
    """what poly_mul's limb loop and rns_reconstruct leave (src/poly.c:94-104, src/rns.c:60-75): a * b centred mod P', the product of the
    first `dim` primes -- the value poly_rns2mpi then reduces"""
    Pp = product_of(primes[:dim])
    return [smod(v, Pp) for v in negacyclic(a, b)]


def poly_mul(primes, a, b, dim, q):
    """src/poly.c:84-107: centred mod P', then centred mod q (poly_rns2mpi, :109-120)"""
    return [smod(v, q) for v in rns_product(primes, a, b, dim)]


def galois_image(sk, g):
    """coefficient t = sk[i'] for i' = t g^-1 mod 2n < n, else -sk[i' - n]"""
    n = len(sk)
    assert g & 1
    ginv = pow(int(g) % (2 * n), -1, 2 * n)
    out = []
    for t in range(n):
        i = (t * ginv) % (2 * n)
        out.append(sk[i] if i < n else -sk[i - n])
    return out


def genswk(P, k, primes, p1_raw, e, sp, sk, dimmul, dimevk, ntt=None):
    """src/he-kem.c:83-110.  Returns the centred key polynomials (swkp0, swkp1); with `ntt` (limb index, residues -> transformed residues)
    the stored slabs [dimevk][n] of both instead (:103-110)."""
    n = len(p1_raw)
    PqL = P << k                                                          # hectx.PqL, q_L = 2^k
    assert dimmul == dimmul_of(P, k, n.bit_length() - 1)                  # :83
    Psp = [int(v) * P for v in sp]                                        # :89-90
    swkp0 = poly_mul(primes, [int(v) for v in p1_raw], [int(v) for v in sk], dimmul, PqL)   # :95
    out0, out1 = [], []
    for i in range(n):
        v = -swkp0[i]                                                     # :97
        v = v + int(e[i])                                                 # :98
        v = (v + Psp[i]) % PqL                                            # :99  mpi_addm
        out0.append(smod(v, PqL))                                         # :100
        out1.append(smod(int(p1_raw[i]), PqL))                            # :101
    if ntt is None:
        return out0, out1
    store = lambda poly: [ntt(d, [v % int(primes[d]) for v in poly]) for d in range(dimevk)]   # :103-110
    return store(out0), store(out1)


def structured(P, k, primes, p1_raw, e, sp, sk, dimmul, stats=None):
    """The same two polynomials as the device forms them: X = p1 sk centred mod P'; aX = X mod P; c2 = smod(X, 2^k); a = (e - aX) mod P by at
    most two additions of P; z2 = (-c2 + e + P sp) mod 2^k; h = (z2 - a) P^-1 mod 2^k; p0 = a + P hs with hs = h as a signed k-bit integer;
    p1c = p1 - m M with m = [p1 >= floor(M/2)] + [p1 >= M + floor(M/2)].  `stats` (a dict) collects what each coefficient went through."""
    n = len(p1_raw)
    M, two_k = P << k, 1 << k
    Pinv = pow(P, -1, two_k)
    X = rns_product(primes, [int(v) for v in p1_raw], [int(v) for v in sk], dimmul)
    out0, out1 = [], []
    for i in range(n):
        aX, c2 = X[i] % P, smod(X[i], two_k)
        a, adds = int(e[i]) - aX, 0
        while a < 0:
            a += P
            adds += 1
        assert adds <= 2 and 0 <= a < P
        z2 = (-c2 + int(e[i]) + P * int(sp[i])) % two_k
        h = ((z2 - a) * Pinv) % two_k
        hs = h - two_k if h >> (k - 1) else h
        out0.append(a + P * hs)
        p1 = int(p1_raw[i])
        assert 0 <= p1 < 1 << M.bit_length()
        m = (p1 >= M // 2) + (p1 >= M + M // 2)
        out1.append(p1 - m * M)
        if stats is not None:
            stats.setdefault("adds", []).append(adds)
            stats.setdefault("aX", []).append(aX)
            stats.setdefault("e", []).append(int(e[i]))
            stats.setdefault("h", []).append(h)
            stats.setdefault("hs", []).append(hs)
            stats.setdefault("m", []).append(m)
    return out0, out1


def h_windows(k):
    return sorted({v % (1 << k) for v in (0, 1, (1 << (k - 1)) - 1, 1 << (k - 1), (1 << (k - 1)) + 1, (1 << k) - 1)})


def p1_windows(P, k):
    M = P << k
    Mh, top = M // 2, 1 << M.bit_length()
    return [v for v in (0, Mh - 1, Mh, Mh + 1, M - 1, M, M + 1, M + Mh - 1, M + Mh, top - 1) if 0 <= v < top]


def carry_windows(k):
    """hs = +-(2^(64 j) - 1): the product P hs carries (borrows) across word boundary j"""
    return [s * ((1 << (64 * j)) - 1) for j in range(1, (k - 1) // 64 + 1) for s in (1, -1) if (1 << (64 * j)) - 1 < 1 << (k - 1)]


def window_inputs(P, k, n, sp=None, seed=0):
    """(p1, e, sp) for the secret sk = 1 (X = p1 coefficient by coefficient, every p1 being below P'/2).  With v = -p1 + e + P sp = a + P h
    and p1 = aX + P t:  h = sp - t - adds (mod 2^k), so t is chosen for the wanted (aX, e, h).  `sp`: the hidden polynomial to use (the
    gathered form: the image of sk = 1 is 1); None draws one of k-bit coefficients."""
    rng = random.Random(1000 * k + seed)
    two_k, M = 1 << k, P << k
    sp = [rng.randrange(-(two_k // 2), two_k // 2 + 1) for _ in range(n)] if sp is None else [int(v) for v in sp]
    want = []                                                             # (aX, e, h) or ("p1", value)
    for aX in list(range(12)) + list(range(P - 11, P)):
        for e in (11, -11):
            want.append((aX, e, rng.randrange(two_k)))
    want += [(rng.randrange(P), rng.randrange(-11, 12), h) for h in h_windows(k)]
    want += [(rng.randrange(P), rng.randrange(-11, 12), hs % two_k) for hs in carry_windows(k)]
    want += [("p1", v) for v in p1_windows(P, k)]
    assert len(want) <= n, "%d windows need n >= %d" % (len(want), len(want))
    while len(want) < n:
        want.append((rng.randrange(P), rng.randrange(-11, 12), rng.randrange(two_k)))
    order = list(range(n))
    rng.shuffle(order)
    p1, e = [0] * n, [0] * n
    for i, w in zip(order, want):
        if w[0] == "p1":
            p1[i], e[i] = w[1], rng.randrange(-11, 12)
            continue
        aX, ev, h = w
        adds = 0 if ev - aX >= 0 else (1 if ev - aX + P >= 0 else 2)
        t = (sp[i] - adds - h) % two_k
        p1[i], e[i] = aX + P * t, ev
        assert p1[i] < M
    return p1, e, sp


def windows_missing(P, k, stats, p1):
    """the windows of the issue that `stats` (from structured) and p1 do not show; empty when window_inputs did its job"""
    missing = []
    seen = set(zip(stats["aX"], (v > 0 for v in stats["e"])))
    for aX in list(range(12)) + list(range(P - 11, P)):
        if (aX, True) not in seen or (aX, False) not in seen:
            missing.append("aX = %d with e of both signs" % aX)
    if set(stats["adds"]) != {0, 1, 2}:
        missing.append("0, 1 and 2 additions of P: saw %s" % sorted(set(stats["adds"])))
    for h in h_windows(k):
        if h not in stats["h"]:
            missing.append("h = %d" % h)
    for v in p1_windows(P, k):
        if v not in p1:
            missing.append("p1 = %d" % v)
    for hs in carry_windows(k):
        if hs not in stats["hs"]:
            missing.append("hs = %d" % hs)
    M = P << k
    if not {(v >= M // 2) + (v >= M + M // 2) for v in p1_windows(P, k)} <= set(stats["m"]):
        missing.append("p1 losing M as often as its windows ask: saw %s" % sorted(set(stats["m"])))
    return missing
