"""Integer model of the modular multiplies with the (c+1) correction folded into mad addends that were zero
(gpqhe_amd/csrc/modarith.hpp: mulmod_split injects K = 2^64 + 31c - 1 == -(c+1), mulmod_raw_t injects c+1) and of every
butterfly class built on them: the results are congruent to the product with nothing left to add, every intermediate fits
the register it lives in, the lazy ranges close as the header states them, and the table check of the wide class rejects
exactly the entries whose fold would outgrow 32 bits.  CPU only: this proves the algebra, on a restatement.  The HIP text of the
primitives is run on the device at the edges of these ranges by tests/test_modarith_device_gpu.py; the kernels are compared with the
oracle word for word in tests/test_inject_gpu.py."""
import random

import pytest

M64 = (1 << 64) - 1
SPLIT_CMAX = 306000000   # GPQ_SPLIT_CMAX
WIDE_CMAX = 134217000    # GPQ_WIDE_CMAX
FOLD_CMAX = 319000000    # GPQ_FOLD_CMAX


class ThOverflow(Exception):
    """th of the split multiply does not fit 32 bits: what the table check exists to rule out"""


def mulmod_split(a, wx, wy, c):
    """mulmod_split(): returns T' == a*w (mod p) for (wx, wy) = (p - w, p - w*2^31 mod p); asserts what the device code relies on"""
    al, ah = a & 0x7FFFFFFF, a >> 31
    assert ah < (1 << 32)
    kinj = 31 * c - 1                                          # PrimeK::kinj, the addend of the first mad
    t0 = al * (wx & 0xFFFFFFFF) + kinj
    assert t0 <= M64
    t0 += ah * (wy & 0xFFFFFFFF)
    assert t0 <= M64
    t1 = al * (wx >> 32) + ((t0 >> 32) | (1 << 32))            # carry word with PrimeK::one in its high dword: + 2^64 in t
    assert t1 <= M64
    t1 += ah * (wy >> 32)
    assert t1 <= M64
    assert (t1 << 32) | (t0 & 0xFFFFFFFF) == al * wx + ah * wy + (1 << 64) + kinj
    th = t1 >> 27
    if th >= (1 << 32):
        raise ThOverflow
    ntl = ((~t0) & 0xFFFFFFFF) | (((~t1) & 0x7FFFFFF) << 32)
    r = c * th + ntl                                           # the fold: one mad
    assert r <= M64
    return r


def mulmod_raw(a, w, c):
    """mulmod_raw_t / mulmod_lazy (the 7-mad form) with c+1 in the addend of its first mad; every register bound asserted"""
    p = (1 << 59) + c
    a0, a1, w0, w1 = a & 0xFFFFFFFF, a >> 32, w & 0xFFFFFFFF, w >> 32
    m00 = a0 * w0 + c + 1
    assert m00 <= M64
    mid = a0 * w1 + (m00 >> 32)
    assert mid <= M64
    mid += a1 * w0
    assert mid <= M64
    hi = a1 * w1 + (mid >> 32)
    assert hi <= M64
    x = (hi << 64) | ((mid & 0xFFFFFFFF) << 32) | (m00 & 0xFFFFFFFF)
    assert x == a * w + c + 1
    xh, xl = x >> 59, x & ((1 << 59) - 1)
    assert xh <= M64
    t0 = c * (xh & 0xFFFFFFFF)
    t1 = c * (xh >> 32) + (t0 >> 32)
    assert t0 <= M64 and t1 <= M64
    t = c * xh
    assert (t1 << 32) | (t0 & 0xFFFFFFFF) == t
    th = t >> 59
    assert th < (1 << 32)
    r = c * th + xl
    assert r <= M64
    r += (1 << 59) - 1 - (t & ((1 << 59) - 1))
    assert r <= M64 and r % p == a * w % p
    return r


def pairs(p, w):
    return p - w, p - ((w << 31) % p)


def fits_wide(p, wx, wy):
    """the model's table check (split_entry_fits_wide): the largest al*X + ah*Y + K over the multiplicands of the wide class, a <= 8p - 1"""
    c = p - (1 << 59)
    amax = 8 * p - 1
    ah, al = amax >> 31, amax & 0x7FFFFFFF
    top = al * wx + ah * wy
    below = 0x7FFFFFFF * wx + (ah - 1) * wy
    return max(top, below) + (1 << 64) + 31 * c - 1 < (1 << 91)


def is_prime(m):
    if m < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if m % q == 0:
            return m == q
    d, s = m - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):   # deterministic below 3.3 * 10^24
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def chain_cs(logn, count):
    """c = p - 2^59 of the reference's prime chain (src/precomp.c:358, :372-376): p steps by 2n from 2^59 + 1"""
    out, p = [], (1 << 59) + 1
    while len(out) < count:
        p += 2 << logn
        while not is_prime(p):
            p += 2 << logn
        out.append(p - (1 << 59))
    return out


CHAIN16, CHAIN17 = chain_cs(16, 58), chain_cs(17, 57)       # dimub of the largest contexts the suite builds
WIDE_CS = sorted({1, WIDE_CMAX - 1} | {c for c in CHAIN16 + CHAIN17 if c < WIDE_CMAX})
SPLIT_CS = sorted({1, WIDE_CMAX - 1, SPLIT_CMAX - 1} | {c for c in CHAIN16 + CHAIN17 if c < SPLIT_CMAX})
FOLD_CS = sorted({1, FOLD_CMAX - 1} | set(CHAIN16 + CHAIN17))


def twiddles(p, rnd, k):
    """random, w <= 2^34 and p - w <= 2^34"""
    small = [1, 2, 3, 4, 5, 1 << 28, (1 << 28) + 1, 1 << 34, (1 << 34) - 1] + [rnd.randrange(1, (1 << 34) + 1) for _ in range(k)]
    return small + [p - w for w in small] + [rnd.randrange(1, p) for _ in range(2 * k)]


def multiplicands(p, rnd, top, k):
    """0, 1, 2^62 - 1, 2^62, the class's stated maximum, random"""
    edge = [0, 1, (1 << 62) - 1, 1 << 62, top, top - 1, p - 1, p, (1 << 61) - 1, 1 << 61, (top >> 31 << 31) - 1]
    return [a for a in edge if 0 <= a <= top] + [rnd.randrange(top + 1) for _ in range(k)]


def test_chains_are_the_ones_the_classes_were_cut_for():
    assert len(CHAIN16) == 58 and len(CHAIN17) == 57
    assert max(CHAIN16 + CHAIN17) < SPLIT_CMAX                  # modarith.hpp: every prime of the chains up to n = 2^17
    assert any(c >= WIDE_CMAX for c in CHAIN17)                 # ... and n = 2^17 leaves the wide class part of the way


@pytest.mark.parametrize("c", FOLD_CS)
def test_general_multiply_is_congruent_with_nothing_to_add(c):
    """mulmod_raw_t: a < 8p times w < p (twiddles), and the operand pairs of the middle kernels (left < 2p or < 4p, right < 6p):
    the result is the product mod p, below 3.42p (< 4p), with every column and both folds inside their registers."""
    p = (1 << 59) + c
    rnd = random.Random(c)
    for a in multiplicands(p, rnd, 8 * p - 1, 40):
        for w in twiddles(p, rnd, 4):
            r = mulmod_raw(a, w, c)
            assert r < 4 * p and 100 * r < 342 * p
    left = 2 * p - 1 if c >= WIDE_CMAX else 4 * p - 1              # TwTraits::left of the split / wide class
    if c < SPLIT_CMAX:
        for a, b in [(left, 6 * p - 1), (left, 0), (0, 6 * p - 1), (1, 1)] + [(rnd.randrange(left + 1), rnd.randrange(6 * p)) for _ in range(500)]:
            assert mulmod_raw(a, b, c) < 4 * p
        assert 2 * mulmod_raw(left, 6 * p - 1, c) < 8 * p          # d1 = sum of two products enters inv_from8


@pytest.mark.parametrize("c", SPLIT_CS)
def test_split_class_multiply_and_butterflies(c):
    """Split class: multiplicands below 6p need no table check (th <= 3.5 * 2^30 + 33 for ANY entry); product below 3p; forward
    data stays below 6p, inverse below 3p, gs_last canonicalises with two conditional subtractions."""
    p = (1 << 59) + c
    rnd = random.Random(c + 1)
    ws = twiddles(p, rnd, 5)
    for wx in (p - 1, 1, p):
        for wy in (p - 1, 1, p):
            assert mulmod_split(6 * p - 1, wx, wy, c) < 3 * p       # any pair at all: the worst th
    for w in ws:
        wx, wy = pairs(p, w)
        for a in multiplicands(p, rnd, 6 * p - 1, 20):
            t = mulmod_split(a, wx, wy, c)
            assert t < 3 * p and t % p == a * w % p
        for _ in range(20):
            x, y = (rnd.choice([0, 1, p, 3 * p - 1, 3 * p, 6 * p - 1, rnd.randrange(6 * p)]) for _ in range(2))
            t = mulmod_split(y, wx, wy, c)                          # ct_bfly(TwS)
            xs = x - 3 * p if x >= 3 * p else x
            x2, y2 = xs + t, xs + 3 * p - t
            assert x2 < 6 * p and 0 < y2 < 6 * p and x2 % p == (x + y * w) % p and y2 % p == (x - y * w) % p
            x, y = x % (3 * p), y % (3 * p)                         # gs_bfly_split
            v, d = x + y, x + 3 * p - y
            assert 0 < d < 6 * p
            x2, y2 = (v - 3 * p if v >= 3 * p else v), mulmod_split(d, wx, wy, c)
            assert x2 < 3 * p and y2 < 3 * p and x2 % p == (x + y) % p and y2 % p == (x - y) * w % p
            for val, arg in ((x + y, v), (x - y, d)):               # gs_last: canon4
                t = mulmod_split(arg, wx, wy, c)
                t = t - 2 * p if t >= 2 * p else t
                t = t - p if t >= p else t
                assert t == val * w % p


@pytest.mark.parametrize("c", WIDE_CS)
def test_wide_class_multiply_and_butterflies(c):
    """Wide class: every multiplicand up to 8p - 1 through entries that pass the table check: th fits, product below 2p;
    ct_bfly_wide A (x, y < 6p -> x' < 8p, y' in (0, 8p)) and B (x, y < 8p -> below 6p); gs_bfly_wide with and without its
    subtraction; gs_last canonicalises with one subtraction of p."""
    p = (1 << 59) + c
    assert 8 * p - 1 <= (1 << 62) + (1 << 31) - 2
    rnd = random.Random(c + 2)
    for w in twiddles(p, rnd, 5):
        wx, wy = pairs(p, w)
        if not fits_wide(p, wx, wy):
            continue
        for a in multiplicands(p, rnd, 8 * p - 1, 20):
            t = mulmod_split(a, wx, wy, c)
            assert t < 2 * p and t % p == a * w % p
        for _ in range(20):
            edge = [0, 1, p, 4 * p - 1, 4 * p, 6 * p - 1, (1 << 62) - 1, 1 << 62, 8 * p - 1]
            for kind, lim in (("A", 6 * p), ("B", 8 * p)):
                x, y = (rnd.choice(edge + [rnd.randrange(lim)]) % lim for _ in range(2))
                t = mulmod_split(y, wx, wy, c)
                xs = x - 4 * p if kind == "B" and x >= 4 * p else x
                x2, y2 = xs + t, xs + 2 * p - t
                assert x2 % p == (x + y * w) % p and y2 % p == (x - y * w) % p and y2 > 0
                assert (x2 < 8 * p and y2 < 8 * p) if kind == "A" else (x2 < 6 * p and y2 < 6 * p)
            for both_product_legs in (False, True):
                lim = 2 * p if both_product_legs else 4 * p
                x, y = (rnd.choice(edge + [rnd.randrange(lim)]) % lim for _ in range(2))
                v, d = x + y, x + 4 * p - y
                assert 0 < d < 8 * p
                x2 = v if both_product_legs else (v - 4 * p if v >= 4 * p else v)
                y2 = mulmod_split(d, wx, wy, c)
                assert x2 < 4 * p and y2 < 2 * p and x2 % p == (x + y) % p and y2 % p == (x - y) * w % p
            x, y = rnd.randrange(4 * p), rnd.randrange(4 * p)       # gs_last(TwW)
            for val, arg in ((x + y, x + y), (x - y, x + 4 * p - y)):
                t = mulmod_split(arg, wx, wy, c)
                assert t < 2 * p and (t - p if t >= p else t) == val * w % p


def seven_mad_butterflies(x, y, w, c):
    p = (1 << 59) + c
    t = mulmod_raw(y, w, c)                                         # ct_bfly(uint64_t): x, y < 8p
    xs = x - 4 * p if x >= 4 * p else x
    x2, y2 = xs + t, xs + 4 * p - t
    assert x2 < 8 * p and 0 < y2 < 8 * p and x2 % p == (x + y * w) % p and y2 % p == (x - y * w) % p
    x, y = x % (4 * p), y % (4 * p)                                 # gs_bfly(uint64_t): x, y < 4p
    v, d = x + y, x + 4 * p - y
    x2, y2 = (v - 4 * p if v >= 4 * p else v), mulmod_raw(d, w, c)
    assert x2 < 4 * p and y2 < 4 * p and x2 % p == (x + y) % p and y2 % p == (x - y) * w % p
    for val, arg in ((x + y, v), (x - y, d)):                       # gs_last: canon4
        t = mulmod_raw(arg, w, c)
        t = t - 2 * p if t >= 2 * p else t
        t = t - p if t >= p else t
        assert t == val * w % p


@pytest.mark.parametrize("c", sorted(set(FOLD_CS) | {SPLIT_CMAX}))
def test_seven_mad_butterflies(c):
    p = (1 << 59) + c
    rnd = random.Random(c + 3)
    for w in twiddles(p, rnd, 3):
        for _ in range(25):
            x, y = (rnd.choice([0, 1, p, 4 * p - 1, 4 * p, 8 * p - 1, (1 << 62) - 1, 1 << 62, rnd.randrange(8 * p)]) for _ in range(2))
            seven_mad_butterflies(x, y, w, c)


def entries_to_judge(p, rnd):
    out = []
    for w in twiddles(p, rnd, 15) + list(range(1, 40)) + [q * (1 << 28) + j for q in (1, 2, 5, 6, 7, 13, 14, 15, 21, 22, 23, 24, 30) for j in (0, 1, 2, 3, 4)] + [(1 << 28) + k for k in range(-3, 4)]:
        out.append(pairs(p, w))
    out += [(p - 1, p - 1), (p, p), (p - 1, 1), (1, p - 1), (p - (1 << 33), p - (1 << 31)), (p - 4, p - (1 << 33))]
    return out


def overflows(p, wx, wy):
    """does ANY multiplicand of the wide class drive th past 32 bits?  (searched where the sum is largest, and beside it)"""
    c = p - (1 << 59)
    amax = 8 * p - 1
    tops = [amax, amax - 1, (amax >> 31 << 31) - 1, (amax >> 31 << 31), (1 << 62) - 1, 1 << 62, (1 << 62) - (1 << 31) - 1]
    for a in tops:
        try:
            mulmod_split(a, wx, wy, c)
        except ThOverflow:
            return True
    return False


@pytest.mark.parametrize("c", WIDE_CS)
def test_table_check_rejects_exactly_the_overflowing_entries(c):
    """The predicate is the exact bound: an entry fails it if and only if some multiplicand up to 8p - 1 makes th outgrow 32 bits.
    w = 1, 2, 3 are such entries (w + w*2^31 < 2c + 15 * 2^29), and so are w = q 2^28 + j for j = 1, 2, 3 and small q (there w*2^31 mod p
    = j 2^31 - q c is small again); a random twiddle never is.  The library's exported predicate
    (gpq_debug_split_entry_fits_wide: what upload_tables runs over every entry of a wide limb) agrees on the whole list."""
    from gpqhe_amd import _native
    lib = _native.load()
    p = (1 << 59) + c
    rnd = random.Random(c + 4)
    entries = entries_to_judge(p, rnd)
    rejected = 0
    for wx, wy in entries:
        ok = fits_wide(p, wx, wy)
        assert ok == (not overflows(p, wx, wy)), (wx, wy)
        assert lib.gpq_debug_split_entry_fits_wide(p, wx, wy) == int(ok), (wx, wy)
        rejected += not ok
    for w in (1, 2, 3):
        assert not fits_wide(p, *pairs(p, w))
    assert fits_wide(p, *pairs(p, 4)) and fits_wide(p, *pairs(p, p - 1))
    assert 3 <= rejected < len(entries) // 3
    assert not fits_wide(p, *pairs(p, (1 << 28) + 1)) and fits_wide(p, *pairs(p, 1 << 28)) and fits_wide(p, *pairs(p, 60 * (1 << 28) + 1))   # q (2^28 - c) + 2^31 > 15 * 2^29 + 2c from q = 45 on, for every c of the class
    # outside the wide class the symbol says so, it does not guess
    assert lib.gpq_debug_split_entry_fits_wide((1 << 59) + WIDE_CMAX, 1, 1) == -1
    assert lib.gpq_debug_split_entry_fits_wide(p, p + 1, 1) == -1
