"""Coefficients placed in the ROUNDING WINDOWS of the relinearisation tail (src/he-mult.c:67-77, src/he-automorphism.c:68-76), for whole
gpq_he_mul / gpq_he_swk / gpq_he_mul_rs / gpq_he_rot_hoisted calls.  No GPU, no torch: Python integers and (for the keys) the CPU oracle.

THE CONSTRUCTION.  The key switch of the constant polynomial 1 with the key NTT(X) returns X: with a ciphertext whose c1 is 1 (he_mul:
a1 = b1 = 1, hence d2 = 1; he_swk / he_rot: d1 = 1) and a key that is the forward transform of chosen residues, the tail is handed exactly
the integers chosen here, while dense d0, d1 become its addends.

THE MODEL (TailModel) restates the tail's fixed-point estimate from its definition (bridge_tables.hpp, get_tail_direct's comment), never from a
kernel's output:  y_d = x_d (Pi_B/p_d)^-1 mod p_d,  weight_d = floor(Pi' 2^104 / p_d),  V = sum y_d weight_d,  frac = V mod 2^104  -- an
underestimate of 2^104 (x mod P)/P by less than dimP 2^60.  A coefficient is IN A WINDOW when bits 102..66 of frac are all ones: bit 103
clear = within 2^-38 below 1/2 (mpi_rdiv's decision), set = within 2^-38 below 1 (the estimate may have borrowed from floor(x/P)).  The
model only says WHERE an input lies (which classes are populated, which waves are clean); expected outputs never come from it.

THE CLASSES of r = x mod P, x = q P + r (mod Pi_B):  half-1, half, half+1, half+2 (half = floor(P/2): the tie rounds down, the estimate is
below 1/2 while the truth is on or above it);  0 (error exactly 0, outside), 1, 2 (the estimate borrows), P-1, P-2;  and three ladders --
geometric sweeps classified with the model, because an edge sits at window +- err P and err depends on x:  half + k (truth above 1/2,
estimate on either side), half - floor(P 2^-38) + k (lower edge of the window below 1/2), P - floor(P 2^-38) + k (lower edge of the window
below 1).  From each sweep the members nearest to the edge on both sides are kept.  The classes are crossed with the quotients
q in {hq, hq-1, -hq, -hq-1 (r != 0), 0, -1, random}, hq = floor(Pi'/2): the wrap corner, where the centring of x -- not of q -- decides.
For gpq_he_mul_rs: r = half+1 with q chosen from the known addend d so that rdiv(x, P) + d has low s bits 2^(s-1)-1, 2^(s-1), 2^(s-1)+1:
a wrong first rounding flips the second one.
"""
import random

import numpy as np

FRAC_BITS = 104
POINT_CLASSES = ("half-1", "half", "half+1", "half+2", "0", "1", "2", "P-1", "P-2")
LADDERS = ("half+k", "lower-edge+k", "upper-edge+k")
RS_CLASSES = ("rs-tie-1", "rs-tie", "rs-tie+1")
Q_CLASSES = ("hq", "hq-1", "-hq", "-hq-1", "0", "-1", "random")
IN_WINDOW = {"half-1": True, "half": True, "half+1": True, "half+2": True, "0": False, "1": True, "2": True, "P-1": True, "P-2": True,
             "rs-tie-1": True, "rs-tie": True, "rs-tie+1": True}


def _prod(v):
    r = 1
    for x in v:
        r *= int(x)
    return r


class TailModel:
    """the one-product tail's estimate of 2^104 x / P over the basis primes[:dimB], P = prod primes[:dimP]"""

    def __init__(self, primes, dimP, dimB):
        self.p = [int(x) for x in primes[:dimB]]
        self.dimP, self.dimB = dimP, dimB
        self.P, self.PiB = _prod(self.p[:dimP]), _prod(self.p)
        self.Piq = self.PiB // self.P
        self.half, self.hq = self.P // 2, self.Piq // 2
        self.inv = [pow((self.PiB // p) % p, -1, p) for p in self.p]
        self.weight = [(self.Piq << FRAC_BITS) // p for p in self.p]
        # the underestimate, in units of r = x mod P: sum over the limbs of P of y_d {Pi' 2^104 / p_d} < dimP max(p) units of 2^-104
        self.err_r = (dimP * max(self.p[:dimP]) * self.P >> FRAC_BITS) + 1
        self.win_r = self.P >> 38                                     # the window's width in units of r

    def frac(self, x):
        v = 0
        for p, i, w in zip(self.p, self.inv, self.weight):
            v += ((x % p) * i % p) * w
        return v & ((1 << FRAC_BITS) - 1)

    @staticmethod
    def in_window(frac):
        """bits 102..66 all ones: top38 == 2^37 - 1 (bit 103 clear) or 2^38 - 1 (bit 103 set)"""
        return (frac >> 66) & ((1 << 37) - 1) == (1 << 37) - 1

    def window(self, x):
        """0: outside; 1: within 2^-38 below 1/2; 2: within 2^-38 below 1"""
        f = self.frac(x)
        return 0 if not self.in_window(f) else 1 + (f >> 103)


class CrtModel:
    """the plain CRT fast paths of gpq_rns_reconstruct over primes[:dim]: frac = sum y_d floor(2^F / p_d) mod 2^F, y_d = x_d (P/p_d)^-1 mod p_d,
    an underestimate of x / P; the centring of x cannot be decided within 2^-window_bits below 1/2.
    (F, window_bits) = (104, 38): the matrix-core kernel; (128, 61): bridge_reconstruct_low."""

    def __init__(self, primes, dim, frac_bits, window_bits):
        self.p = [int(x) for x in primes[:dim]]
        self.P = _prod(self.p)
        self.half = self.P // 2
        self.F, self.wb = frac_bits, window_bits
        self.inv = [pow((self.P // p) % p, -1, p) for p in self.p]
        self.weight = [(1 << frac_bits) // p for p in self.p]
        self.err_r = (dim * max(self.p) * self.P >> frac_bits) + 1
        self.win_r = self.P >> window_bits

    def frac(self, x):
        v = 0
        for p, i, w in zip(self.p, self.inv, self.weight):
            v += ((x % p) * i % p) * w
        return v & ((1 << self.F) - 1)

    def in_window(self, frac):
        return frac >> (self.F - self.wb) == (1 << (self.wb - 1)) - 1


def _geometric(limit):
    """1, 2, 3, 4, 6, 8, 12, 16, ... up to limit: two steps per octave"""
    out, k = [], 1
    while k <= limit:
        out.append(k)
        if k > 1 and k + (k >> 1) <= limit:
            out.append(k + (k >> 1))
        k <<= 1
    return out


def _sweep(span, steps_fine=8):
    """k on a geometric ladder up to `span`, denser (steps_fine per octave) in its last 8 octaves: an edge sits at err P, a few times below
    the bound `span` is made from"""
    ks = set(_geometric(span))
    lo = max(span >> 8, 1)
    for j in range(8 * steps_fine + 1):
        ks.add(min(span, max(1, lo * int(2 ** (j / steps_fine) * (1 << 20)) >> 20)))
    return sorted(ks)


def _span(M):
    """how far a ladder goes from its base: twice the bound of the estimate's error, and never so far that a candidate leaves the window
    (or reaches it) on its other side"""
    return min(2 * M.err_r, M.win_r // 2)


def _nearest_to_edge(cand, side, inside_below):
    """cand = [(k, .., inside)] of one sweep: the `side` candidates nearest to the modelled edge on each side of it.  Inside and outside
    candidates interleave around the edge (err depends on x).  inside_below: the window lies below the edge (half + k), else above it."""
    ins, outs = [c for c in cand if c[-1]], [c for c in cand if not c[-1]]
    assert len(ins) >= side and len(outs) >= side, "the sweep found one side only"
    if inside_below:
        return sorted(ins, key=lambda c: -c[0])[:side] + sorted(outs, key=lambda c: c[0])[:side]
    return sorted(ins, key=lambda c: c[0])[:side] + sorted(outs, key=lambda c: -c[0])[:side]


class Crafted:
    """one crafted polynomial: xs[i] in [0, Pi_B); cls[i] = (class, q class) for the crafted indices; win[i] = the model's window (1, 2) for
    the coefficients inside one"""

    def __init__(self, xs, cls, win):
        self.xs, self.cls, self.win = xs, cls, win

    def counts(self):
        c = {}
        for name, _ in self.cls.values():
            c[name] = c.get(name, 0) + 1
        return c

    def slab(self, primes, dimB):
        """residues [dimB][n] of the coefficients: what the key switch must deliver"""
        return np.array([x % int(primes[d]) for d in range(dimB) for x in self.xs], dtype=np.uint64)


def members_per_class(n, rs):
    """(members of a point class, members of a ladder on each side of its edge) such that at most n/16 coefficients are crafted"""
    budget, extra = n // 16, 3 if rs else 0
    for m, side in ((4, 4), (4, 3), (3, 2), (2, 2), (2, 1)):
        if (len(POINT_CLASSES) + extra) * m + 2 * side * len(LADDERS) <= budget:
            return m, side
    raise ValueError("n = %d has no room for every class twice" % n)


def layout(n, count, seed, dirty_groups=None):
    """`count` distinct indices: 0, 63, 64, n-1 first, the rest scattered inside at most half of the n/64 groups (groups 0, 1, the last one
    and others picked by seed), so that clean groups -- waves without a flag -- sit next to flagged ones"""
    rng = random.Random(seed)
    groups = n // 64
    if dirty_groups is None:
        others = list(range(2, groups - 1))
        rng.shuffle(others)
        dirty_groups = [0, 1, groups - 1] + others[:max(0, groups // 2 - 3)]
    assert len(set(dirty_groups)) <= groups // 2
    idx = [0, 63, 64, n - 1]
    pool = [g * 64 + j for g in dirty_groups for j in range(64) if g * 64 + j not in idx]
    rng.shuffle(pool)
    idx += pool[:count - 4]
    assert len(idx) == count and len(set(idx)) == count
    return idx


def build(model, n, seed, rs=None):
    """One crafted polynomial over `model` (TailModel).  rs = (s, addend): log2 Delta of gpq_he_mul_rs and the tail's addend d[i] (centred
    ints) for this polynomial: adds the second-rounding classes.  The crafted coefficients go where layout() says.
    Asserts, with the model, every condition the tests rely on."""
    rng = random.Random(seed)
    M, P, PiB, half, hq = model, model.P, model.PiB, model.half, model.hq
    m, side = members_per_class(n, rs is not None)

    def quotient(qc, r):
        if qc == "hq":
            return hq
        if qc == "hq-1":
            return hq - 1
        if qc == "-hq":
            return -hq
        if qc == "-hq-1":
            return -hq - 1 if r else -hq                   # (the most negative representable x)
        if qc == "0":
            return 0
        if qc == "-1":
            return -1
        return rng.randrange(-hq + 2, hq - 2)

    qturn = [seed % len(Q_CLASSES)]

    def next_q():
        qturn[0] += 1
        return Q_CLASSES[qturn[0] % len(Q_CLASSES)]

    crafted = []                                           # (class, q class, x)
    point_r = {"half-1": half - 1, "half": half, "half+1": half + 1, "half+2": half + 2, "0": 0, "1": 1, "2": 2, "P-1": P - 1, "P-2": P - 2}
    for name in POINT_CLASSES:
        for _ in range(m):
            qc = next_q()
            r = point_r[name]
            crafted.append((name, qc, (quotient(qc, r) * P + r) % PiB))
    # the ladders: a sweep of r = base + k, every candidate with a quotient class of its own, classified by the model; kept: the members
    # nearest to the edge, `side` inside the window and `side` outside
    span = _span(M)
    for name, base, signs in (("half+k", half, (1,)), ("lower-edge+k", half - M.win_r, (-1, 1)), ("upper-edge+k", P - M.win_r, (-1, 1))):
        cand = []
        for sgn in signs:
            for k in _sweep(span):
                if name == "half+k" and k < 3:
                    continue                               # (half+1, half+2 are classes of their own)
                qc = next_q()
                r = base + sgn * k
                x = (quotient(qc, r) * P + r) % PiB
                cand.append((sgn * k, qc, x, M.window(x) != 0))
        for c in _nearest_to_edge(cand, side, inside_below=name == "half+k"):
            crafted.append((name, c[1], c[2]))
    idx = layout(n, len(crafted) + (3 * m if rs else 0), seed)
    if rs is not None:
        s, addend = rs
        at = idx[len(crafted):len(crafted) + 3 * m]
        for j, i in enumerate(at):
            name, target = RS_CLASSES[j % 3], ((1 << (s - 1)) + (j % 3) - 1) % (1 << s)
            q0 = rng.randrange(-hq // 2, hq // 2)
            q = q0 - ((q0 + 1 + addend[i] - target) % (1 << s))        # rdiv(q P + half + 1, P) = q + 1
            assert (q + 1 + addend[i]) % (1 << s) == target
            crafted.append((name, "from-addend", (q * P + half + 1) % PiB))
    assert len(idx) >= len(crafted)
    xs = [rng.randrange(PiB) for _ in range(n)]
    cls = {}
    for i, (name, qc, x) in zip(idx, crafted):
        xs[i] = x
        cls[i] = (name, qc)
    win = {}
    for i, x in enumerate(xs):
        w = M.window(x)
        if w:
            win[i] = w
    check(M, Crafted(xs, cls, win), n, rs is not None)
    return Crafted(xs, cls, win)


def check(model, c, n, rs):
    """the conditions of the construction, stated with the model"""
    counts = c.counts()
    for name in POINT_CLASSES + LADDERS + (RS_CLASSES if rs else ()):
        assert counts.get(name, 0) >= 2, "class %s has %d members" % (name, counts.get(name, 0))
    for i, (name, _) in c.cls.items():
        if name in IN_WINDOW:
            assert (i in c.win) == IN_WINDOW[name], "%s at %d: modelled %s a window" % (name, i, "inside" if i in c.win else "outside")
    for name in LADDERS:
        sides = {i in c.win for i, (k, _) in c.cls.items() if k == name}
        assert sides == {True, False}, "%s: one side of the edge only" % name
    assert {c.win[i] for i in c.win} == {1, 2}, "both windows must be populated"
    assert len(c.cls) * 16 <= n, "%d of %d coefficients are crafted" % (len(c.cls), n)
    assert all(i in c.cls for i in (0, 63, 64, n - 1))
    assert all(i in c.cls for i in c.win), "a random coefficient fell into a window"
    dirty = {i // 64 for i in c.win}
    assert 2 * len(dirty) <= n // 64, "%d of %d groups hold an in-window coefficient" % (len(dirty), n // 64)
    assert len({q for _, q in c.cls.values()} & set(Q_CLASSES)) == len(Q_CLASSES), "a quotient class is missing"


def crt_ladder(model, count_side=3):
    """for the plain CRT fast paths (CrtModel): x = half + k (truth above 1/2, the estimate on either side) and half - floor(P 2^-w) + k
    (across the lower edge of the window), classified by the model: the members nearest to each edge on both sides, then a few points.
    Returns [(x, inside)]."""
    M = model
    span = _span(M)
    out = [(x, M.in_window(M.frac(x))) for x in (M.half - 1, M.half, M.half + 1, M.half + 2, 0, 1, M.P - 1)]
    for base, signs in ((M.half, (1,)), (M.half - M.win_r, (-1, 1))):
        cand = [(sgn * k, base + sgn * k, M.in_window(M.frac(base + sgn * k))) for sgn in signs for k in _sweep(span)]
        out += [(x, w) for _, x, w in _nearest_to_edge(cand, count_side, inside_below=base == M.half)]
    return out


def _smod(r, q):
    """mpi_smod, src/types.c:108-113"""
    r %= q
    return r - q if r >= q // 2 else r


def closed_form(model, xs, d, ql):
    """src/he-mult.c:67-77 on the chosen integers themselves: smod(rdiv(x, P) + d, q_l) with x = smod(smod(xs, Pi_B), P q_l) (src/poly.c:109-120),
    mpi_rdiv = floor plus one when the remainder is above floor(P/2) (src/types.c:115-128); d = None adds nothing"""
    P, out = model.P, []
    for i, x in enumerate(xs):
        x = _smod(_smod(x, model.PiB), P * ql)
        q, r = divmod(x, P)
        v = q + (1 if r > P // 2 else 0)
        out.append(_smod((v + (d[i] if d is not None else 0)) % ql, ql))
    return out


def sparse_negacyclic(a, terms, ql):
    """smod(a * b mod x^n + 1, q_l) for b given by its non-zero terms {index: value}"""
    n = len(a)
    r = [0] * n
    for j, v in terms.items():
        for i in range(n):
            if i + j < n:
                r[i + j] += a[i] * v
            else:
                r[i + j - n] -= a[i] * v
    return [_smod(x, ql) for x in r]
