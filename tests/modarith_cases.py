"""Domain -> post-condition table and directed operands for the inline device primitives of gpqhe_amd/csrc/modarith.hpp, of
gs_last / TwTraits / ref_fqmul (ntt_kernels.hpp) and of horner59 (bridge_kernels.hpp), one row per op of libgpqhe_modprobe.so
(gpqhe_amd/csrc/modarith_probe.hip).  Shared by tests/test_modarith_device_gpu.py, which runs the HIP text on these operands, and
tests/test_modarith_probe_cover.py, which runs the generator against the bounds with no device.

Every domain and bound is the header's own, quoted in the row (`quote`).  A post-condition is either `exact` (the output equals
the integer) or a congruence with a range: output == value (mod p) and lo <= output < hi.  Nothing here has a tolerance.

The class limits 2^59 + 257, 2^59 + GPQ_*_CMAX - 1 are not prime and need not be: every identity the primitives rest on
(2^59 == -c mod p, the folds, the conditional subtractions) holds for any odd modulus of the shape 2^59 + c; a modular inverse
is needed of 2^31 only.  The limits themselves are parsed out of modarith.hpp."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpqhe_amd", "csrc")
PROBE_PATH = os.path.join(ROOT, "gpqhe_amd", "libgpqhe_modprobe.so")

M64 = (1 << 64) - 1
B59 = 1 << 59
M59 = B59 - 1
NRANDOM = 1 << 13


def header_limit(name):
    with open(os.path.join(CSRC, "modarith.hpp")) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)u\b" % name, f.read(), re.M)
    assert m, "modarith.hpp no longer defines %s as a plain number" % name
    return int(m.group(1))


FOLD_CMAX, SPLIT_CMAX, WIDE_CMAX = header_limit("GPQ_FOLD_CMAX"), header_limit("GPQ_SPLIT_CMAX"), header_limit("GPQ_WIDE_CMAX")
CLASS_CMAX = {"fold": FOLD_CMAX, "split": SPLIT_CMAX, "wide": WIDE_CMAX}     # a class admits c < its limit
REAL_CHAINS = ((7, 5), (13, 20), (17, 45))    # (logn, limbs): the first and the last prime of each; the last of (17, 45) has the largest real c


# ---------------------------------------------------------------------------------------------------------------------------
# moduli
# ---------------------------------------------------------------------------------------------------------------------------
class Modulus:
    def __init__(self, p, label, table=()):
        self.p, self.c, self.label, self.table = p, p - B59, label, tuple(table)

    def admits(self, klass):
        return self.c < CLASS_CMAX[klass]

    def __repr__(self):
        return self.label


_MODULI = None


def moduli():
    """Real primes with ten multipliers of their own tables (eight twiddles, n^-1, winv[1] n^-1, all in standard form), then the limits."""
    global _MODULI
    if _MODULI is None:
        from oracle.oracle import OracleCtx
        out, seen = [], set()
        for logn, dim in REAL_CHAINS:
            o = OracleCtx(logn, dim)
            n = 1 << logn
            for d in (0, dim - 1):
                p = o.p[d]
                if p in seen:
                    continue
                seen.add(p)
                r_inv = pow(1 << 64, -1, p)                                   # the oracle's tables are in Montgomery form
                z, zi = o.zetas(d), o.zetas(d, inverse=True)
                tw = [int(z[i]) * r_inv % p for i in (1, 2, 3, n // 2, n - 1)] + [int(zi[i]) * r_inv % p for i in (1, 2, n - 1)]
                ninv = o.const("ninv", d) * r_inv % p
                assert ninv * n % p == 1 and tw[0] * tw[0] % p == p - 1 and tw[0] * tw[5] % p == 1 and all(pow(w, 2 * n, p) == 1 for w in tw)
                out.append(Modulus(p, "logn%d_limb%d_c%d" % (logn, d, p - B59), tw + [ninv, tw[5] * ninv % p]))
        for c, label in ((257, "c257"), (WIDE_CMAX - 1, "wide_cmax-1"), (SPLIT_CMAX - 1, "split_cmax-1"), (FOLD_CMAX - 1, "fold_cmax-1")):
            out.append(Modulus(B59 + c, label))
        _MODULI = out
    return _MODULI


# ---------------------------------------------------------------------------------------------------------------------------
# integer models of the primitives as the headers write them (for the generator's self-check only: the device output is never
# compared with these, so another correct formulation of a primitive passes the device test)
# ---------------------------------------------------------------------------------------------------------------------------
class ThOverflow(Exception):
    """th of a fold does not fit 32 bits"""


def pair_of(p, w):
    return p - w, p - ((w << 31) % p)


def model_mul7(a, w, p):
    """mulmod_raw_t: T' = xl + c*th + (2^59 - 1 - tl) for x = a*w + (c+1)"""
    c = p - B59
    a0, a1, w0, w1 = a & 0xFFFFFFFF, a >> 32, w & 0xFFFFFFFF, w >> 32
    m00 = a0 * w0 + c + 1
    mid = a0 * w1 + (m00 >> 32)
    assert m00 <= M64 and mid <= M64
    mid += a1 * w0
    hi = a1 * w1 + (mid >> 32)
    assert mid <= M64 and hi <= M64
    x = a * w + c + 1
    assert x == (hi << 64) | ((mid & 0xFFFFFFFF) << 32) | (m00 & 0xFFFFFFFF)
    xh, xl = x >> 59, x & M59
    assert xh <= M64
    t = c * xh
    th, tl = t >> 59, t & M59
    if th >> 32:
        raise ThOverflow
    r = c * th + xl + (M59 - tl)
    assert r <= M64
    return r


def split_fold(a, X, Y, p):
    """t = al*X + ah*Y + K of mulmod_split as (th, tl)"""
    c = p - B59
    al, ah = a & 0x7FFFFFFF, a >> 31
    assert ah >> 32 == 0
    t0 = al * (X & 0xFFFFFFFF) + 31 * c - 1 + ah * (Y & 0xFFFFFFFF)
    t1 = al * (X >> 32) + ((t0 >> 32) | (1 << 32)) + ah * (Y >> 32)
    assert t0 <= M64 and t1 <= M64
    t = al * X + ah * Y + (1 << 64) + 31 * c - 1
    assert t == (t1 << 32) | (t0 & 0xFFFFFFFF)
    return t >> 59, t & M59


def model_split(a, X, Y, p):
    th, tl = split_fold(a, X, Y, p)
    if th >> 32:
        raise ThOverflow
    r = (p - B59) * th + (M59 - tl)
    assert r <= M64
    return r


def model_horner(r, d, p):
    c = p - B59
    t = c * r
    th, tl = t >> 59, t & M59
    assert th >> 32 == 0
    out = c * th + d + c + 1 + (M59 - tl)
    assert out <= M64
    return out


def model_canon_fold(v, p):
    r = (v & M59) - (p - B59) * (v >> 59)
    return r + p if r < 0 else r


def csub(x, m):
    return x - m if x >= m else x


def canon(x, p, top):
    """canon8 (top = 4) / canon4 (top = 2) as the header composes them"""
    while top:
        x = csub(x, top * p)
        top >>= 1
    return x


def fits_wide(p, X, Y):
    """split_entry_fits_wide restated: the largest al*X + ah*Y + K over a <= 8p - 1 stays below 2^91"""
    amax = 8 * p - 1
    ah, al = amax >> 31, amax & 0x7FFFFFFF
    return max(al * X + ah * Y, 0x7FFFFFFF * X + (ah - 1) * Y) + (1 << 64) + 31 * (p - B59) - 1 < (1 << 91)


def wide_extremal_multiplicands(p):
    """the two points split_entry_fits_wide evaluates: the top multiplicand, and the largest one below its ah (al all ones)"""
    amax = 8 * p - 1
    return amax, (((amax >> 31) - 1) << 31) | 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------
# directed operands
# ---------------------------------------------------------------------------------------------------------------------------
def directed_values(p, top):
    """Multiplicands / data words in [0, top]: the edges of every lazy range, of the 32- and 31-bit splits and of 2^59."""
    v = {0, 1, top, top - 1}
    for m in (1, 2, 3, 4, 6, 8):
        v.update((m * p - 1, m * p, m * p + 1))
    v.update((B59 - 1, B59, 1 << 60, (1 << 61) - 1, 1 << 61, 3 << 60, (3 << 60) + (1 << 31) - 1, (1 << 62) - 1, 1 << 62, (1 << 62) + (1 << 31) - 2))
    ah = top >> 31
    v.update(((ah << 31) | 0x7FFFFFFF, ah << 31, ((ah - 1) << 31) | 0x7FFFFFFF, (ah - 1) << 31))      # low 31 bits all ones / all zero
    v.update((((top >> 32) << 32) | 0xFFFFFFFF, (((top >> 32) - 1) << 32) | 0xFFFFFFFF))               # low 32 bits all ones
    return sorted(x for x in v if 0 <= x <= top)


def wide_family(p):
    """w = q 2^28 + j, j = 1, 2, 3: the multipliers whose pair (X, Y) is within ~2^33 of (p, p) (modarith.hpp, split-twiddle comment)"""
    return [(q << 28) + j for q in range(46) for j in (1, 2, 3)]


def multipliers(mod):
    p = mod.p
    i31 = pow(1 << 31, -1, p)                                                 # w * 2^31 mod p == 1, and == p - 1 for p - i31
    base = [1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 32) - 1, 1 << 32, B59 - 1, i31, p - i31]
    assert (i31 << 31) % p == 1 and ((p - i31) << 31) % p == p - 1
    out, seen = [], set()
    for w in base + list(mod.table) + wide_family(p):
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def constructed_mul7(mod, atop):
    """(a, w) pairs of the 7-mad multiply with a chosen xh = (a*w + c + 1) >> 59 -- the fold's tl = c*xh mod 2^59 is 0, 1 or 2^59 - 1
    -- and pairs with xl = (a*w + c + 1) mod 2^59 equal to 0 and 2^59 - 1.  c is odd, so it has an inverse mod 2^59."""
    p, c = mod.p, mod.c
    cinv = pow(c, -1, B59)
    out = []
    w = B59 - c - 1                                                            # a*w + c + 1 < (xh + 1) 2^59 for a = ceil(xh 2^59 / w)
    for delta in (0, 1, M59):
        xh0 = cinv * delta % B59
        for j in range(9):
            xh = xh0 + j * B59
            a = -(-(xh << 59) // w)
            if a > atop:
                break
            assert (a * w + c + 1) >> 59 == xh and c * xh % B59 == delta
            if j in (0, 1) or -(-((xh + B59) << 59) // w) > atop:
                out.append((a, w))
    w = B59 - c - 2                                                            # odd
    winv = pow(w, -1, B59)
    for xl in (0, M59):
        a = (xl - c - 1) * winv % B59
        assert (a * w + c + 1) % B59 == xl and a <= atop
        out.append((a, w))
    return out


def constructed_split(mod):
    """(a, w) pairs of the split multiply whose fold t = al*X + ah*Y + K has tl = 0, 1 and 2^59 - 1: ah = 0 and X = (tl - K) / al mod 2^59"""
    p, c = mod.p, mod.c
    K = (1 << 64) + 31 * c - 1
    out = []
    for al in (1, 0x7FFFFFFF):
        for tl in (0, 1, M59):
            X = (tl - K) * pow(al, -1, B59) % B59
            if 0 < X < p:
                assert (al * X + K) % B59 == tl
                out.append((al, p - X))
    return out


def xy_for_diff(d, kp, p, top):
    """x, y <= top with x + kp*p - y == d, twice: the smallest such pair, and the one with the largest sum"""
    if not kp * p - top <= d <= kp * p + top:
        return []
    x, y = (d - kp * p, 0) if d >= kp * p else (0, kp * p - d)
    s = min(top - x, top - y)
    return [(x, y), (x + s, y + s)]


def xy_for_sum(s, top):
    if s > 2 * top:
        return []
    x = min(s, top)
    return [(x, s - x), (s // 2, s - s // 2)]


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
class Tuples:
    """Operands of one (row, modulus) case.  x, y: data words; w, v: the multipliers as integers (v: the second constant of the 7-mad
    gs_last); w0, w1: the words the probe is handed (w and v, or the pair X, Y of w); ndirected: tuples [0, ndirected) are directed."""

    def __init__(self):
        self.x, self.y, self.w, self.v, self.w0, self.w1, self.ndirected = [], [], [], [], [], [], 0

    def __len__(self):
        return len(self.x)

    def at(self, i):
        return dict(x=self.x[i], y=self.y[i], w=self.w[i], v=self.v[i], w0=self.w0[i], w1=self.w1[i], kind="directed" if i < self.ndirected else "random")


class Row:
    def __init__(self, name, klass, shape, quote, ref, post, model, xtop=None, ytop=None, tw=None, wtop=None, kp=None, name_suffix=""):
        self.op, self.name, self.klass, self.shape, self.quote = name, name + name_suffix, klass, shape, quote
        self.ref, self.post, self.model = ref, post, model
        self.xtop, self.ytop, self.tw, self.wtop, self.kp = xtop, ytop, tw, wtop, kp
        self.results = len(post)

    def __repr__(self):
        return self.name

    def bounds(self, mod, j):
        """None for an exact output, else (lo, hi): lo <= output < hi"""
        if self.post[j] is None:
            return None
        lo, hi = self.post[j]
        return lo(mod.p, mod.c), hi(mod.p, mod.c)

    # -- operands ---------------------------------------------------------------------------------------------------------
    def _raw_tuples(self, mod, rng, nrandom):
        """(x, y, w, v) lists: directed, then random"""
        p = mod.p
        xtop = self.xtop(p) if self.xtop else 0
        ytop = self.ytop(p) if self.ytop else 0
        if self.tw is None:
            ws = [0]
        elif self.tw == "var":                                                # variable * variable: the multiplier is a data word too
            ws = sorted(set(directed_values(p, self.wtop(p)) + [w for w in multipliers(mod)[:10]]))
        else:
            ws = multipliers(mod)
        wtop = self.wtop(p) if self.wtop else p - 1
        d = []
        if self.shape == "mul":
            xs = directed_values(p, xtop)
            d += [(a, 0, w, 0) for a in xs for w in ws]
            if self.tw in ("7", "var"):
                d += [(a, 0, w, 0) for a, w in constructed_mul7(mod, xtop)]
            else:
                d += [(a, 0, w, 0) for a, w in constructed_split(mod)]
        elif self.shape == "ct":                                              # the multiplicand is y; x walks its own edges alongside
            xs, ys = directed_values(p, xtop), directed_values(p, ytop)
            d += [(xs[(5 * i + j) % len(xs)], y, w, 0) for i, y in enumerate(ys) for j, w in enumerate(ws)]
            d += [(x, y, ws[(i + 3 * j) % len(ws)], 0) for i, x in enumerate(xs) for j, y in enumerate((0, 1, ytop))]
        elif self.shape in ("gs", "last"):                                    # the multiplicand is d = x + kp*p - y (and x + y for gs_last)
            assert xtop == ytop
            xy = []
            for dv in directed_values(p, self.kp * p + xtop):
                xy += xy_for_diff(dv, self.kp, p, xtop)
            for s in directed_values(p, 2 * xtop):
                xy += xy_for_sum(s, xtop)
            xy = sorted(set(xy))
            d += [(x, y, w, ws[(i + j + 1) % len(ws)]) for i, (x, y) in enumerate(xy) for j, w in enumerate(ws)]
        elif self.shape == "unary":
            d += [(x, 0, 0, 0) for x in directed_values(p, xtop)]
        elif self.shape == "add":
            e = [0, 1, 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1, p, B59 - 1, B59, (1 << 32) - 1, 1 << 32]
            d += [(x, y, 0, 0) for x in e for y in e]
        elif self.shape == "horner":
            ds = [0, 1, 2, mod.c, mod.c + 1, (1 << 32) - 1, 1 << 32, 1 << 58, M59 - 1, M59]
            d += [(r, dd, 0, 0) for r in directed_values(p, xtop) for dd in ds]
            cinv = pow(mod.c, -1, B59)
            for tl in (0, 1, M59):                                            # the fold's tl = c*r mod 2^59
                for j in range(4):
                    r = cinv * tl % B59 + j * B59
                    if r <= xtop:
                        assert mod.c * r % B59 == tl
                        d += [(r, dd, 0, 0) for dd in (0, 1, M59)]
        else:
            raise ValueError(self.shape)
        # uniform over [0, top] by a 128-bit multiply-shift (bias below 2^-63; randint is several times slower)
        bits, nx, ny, nw = rng.getrandbits, xtop + 1, (ytop + 1 if self.ytop else 1), (wtop if self.tw else 1)
        r = [((bits(128) * nx) >> 128, (bits(128) * ny) >> 128, (1 + ((bits(128) * nw) >> 128)) if self.tw else 0, (1 + ((bits(128) * (p - 1)) >> 128)) if self.tw else 0)
             for _ in range(nrandom)]
        return d, r

    def tuples(self, mod, nrandom=NRANDOM):
        """The case's operands.  Wide rows drop the directed pairs the table check rejects (the multiply is not defined for them) and
        list them in .rejected; a random pair is never rejected (asserted)."""
        key = (self.name, mod.p, nrandom)
        if key in _TUPLES:
            return _TUPLES[key]
        p = mod.p
        rng = random.Random("%s/%d" % (self.name, p))
        d, r = self._raw_tuples(mod, rng, nrandom)
        t = Tuples()
        t.rejected = []
        pairs = {}
        for part, is_random in ((d, False), (r, True)):
            for x, y, w, v in part:
                if self.tw in ("S", "W"):
                    if w not in pairs:
                        pairs[w] = pair_of(p, w) + (self.tw != "W" or fits_wide(p, *pair_of(p, w)),)
                    w0, w1, ok = pairs[w]
                    if not ok:
                        assert not is_random, "a random pair fails split_entry_fits_wide: w = %d, p = %d" % (w, p)
                        continue
                else:
                    w0, w1 = w, v
                t.x.append(x); t.y.append(y); t.w.append(w); t.v.append(v); t.w0.append(w0); t.w1.append(w1)
            if not is_random:
                t.ndirected = len(t.x)
        t.rejected = sorted(w for w, (_, _, ok) in pairs.items() if not ok)
        _TUPLES[key] = t
        return t

    def in_domain(self, mod, t, i):
        p = mod.p
        ok = 0 <= t.x[i] <= (self.xtop(p) if self.xtop else 0) and 0 <= t.y[i] <= (self.ytop(p) if self.ytop else 0)
        if self.tw:
            ok = ok and (0 if self.tw == "var" else 1) <= t.w[i] <= (self.wtop(p) if self.wtop else p - 1)
        if self.tw in ("S", "W"):
            ok = ok and (t.w0[i], t.w1[i]) == pair_of(p, t.w[i]) and (self.tw == "S" or fits_wide(p, t.w0[i], t.w1[i]))
        return ok

    # -- the post-condition -----------------------------------------------------------------------------------------------
    def expected(self, mod, t):
        """per output: the exact integers (exact outputs: the value itself; others: its residue mod p)"""
        p = mod.p
        vals = [self.ref(p, x, y, w, v) for x, y, w, v in zip(t.x, t.y, t.w, t.v)]
        return [[e[j] if self.post[j] is None else e[j] % p for e in vals] for j in range(self.results)]

    def violations(self, mod, t, outs):
        """Indices of the tuples whose outputs (lists of ints, one per result) break the post-condition."""
        p = mod.p
        bad = set()
        for j, exp in enumerate(self.expected(mod, t)):
            got = outs[j]
            b = self.bounds(mod, j)
            if b is None:
                if got != exp:
                    bad.update(i for i in range(len(exp)) if got[i] != exp[i])
            else:
                lo, hi = b
                bad.update(i for i in range(len(exp)) if got[i] % p != exp[i] or not lo <= got[i] < hi)
        return sorted(bad)


_TUPLES = {}


def _p(m):
    return lambda p: m * p - 1


def _lt(m):
    """[0, m p)"""
    return (lambda p, c: 0, lambda p, c: m * p)


def _open(m):
    """(0, m p)"""
    return (lambda p, c: 1, lambda p, c: m * p)


BELOW_3_42P = (lambda p, c: 0, lambda p, c: -(-342 * p // 100))              # T' < 3.42p  <=>  T' < ceil(3.42p)
Q_RAW = "mulmod_lazy(a, w): a < 8p, w < p   ->  result in [0, 3.42p), == a*w (mod p)"
Q_SPLIT = "For a multiplicand a < 6p:  ah <= 3*2^29,  th <= 3.5*2^30 + 33,  T' <= c*th + 2^59 - 1 < 3p   for c < GPQ_SPLIT_CMAX"
Q_WIDE = "The split multiply only needs th < 2^32 ... the table check (split_entry_fits_wide) covers the injected constant, and then t = T' <= c (2^32 - 1) + 2^59 - 1 < 2p          for c <= 2^27.  8p - 1 = 2^62 + 8c - 1 is a legal multiplicand"

_mul_ref = lambda p, x, y, w, v: (x * w,)
_ct_ref = lambda p, x, y, w, v: (x + y * w, x - y * w)
_gs_ref = lambda p, x, y, w, v: (x + y, (x - y) * w)


def _ct_model(mul, kx, ky):
    """x' = csub(x, kx p) + t, y' = csub(x, kx p) + ky p - t  (kx = 0: no subtraction)"""
    def f(p, x, y, w0, w1):
        t = mul(y, w0, w1, p)
        xs = csub(x, kx * p) if kx else x
        return xs + t, xs + ky * p - t
    return f


def _gs_model(mul, kp, ks):
    def f(p, x, y, w0, w1):
        v = x + y
        return (csub(v, ks * p) if ks else v), mul(x + kp * p - y, w0, w1, p)
    return f


_m7 = lambda a, w0, w1, p: model_mul7(a, w0, p)
_ms = lambda a, w0, w1, p: model_split(a, w0, w1, p)


def _unary(name, klass, quote, top, fn, post=None, model=None):
    """exact when post is None: output == fn(p, x); else output == x (mod p) inside post.  model: the header's own composition when it differs from fn"""
    m = model or fn
    return Row(name, klass, "unary", quote, (lambda p, x, y, w, v: (fn(p, x),)) if post is None else (lambda p, x, y, w, v: (x,)),
               (post,), lambda p, x, y, w0, w1: (m(p, x),), xtop=_p(top))


_canon4, _canon8, _fold = (lambda p, x: canon(x, p, 2)), (lambda p, x: canon(x, p, 4)), (lambda p, x: model_canon_fold(x, p))

ROWS = [
    # ---- multiplies ---------------------------------------------------------------------------------------------------------
    Row("mulmod_raw_t<false>", "fold", "mul", Q_RAW, _mul_ref, (BELOW_3_42P,), lambda p, x, y, w0, w1: (model_mul7(x, w0, p),), xtop=_p(8), tw="7"),
    Row("mulmod_raw_t<true>", "fold", "mul", Q_RAW, _mul_ref, (BELOW_3_42P,), lambda p, x, y, w0, w1: (model_mul7(x, w0, p),), xtop=_p(8), tw="7"),
    # the variable * variable products of the middle kernels (mulmod_lazy = mulmod_raw_t<false>; ntt_kernels.hpp, TwTraits::left / right)
    Row("mulmod_raw_t<false>", "fold", "mul", "TwTraits<uint64_t>: a forward-range value as the left (< 2p) / right (< 4p) operand of a variable*variable mulmod_lazy; inv_from4: a value < 4p",
        _mul_ref, (_lt(4),), lambda p, x, y, w0, w1: (model_mul7(x, w0, p),), xtop=_p(2), tw="var", wtop=_p(4), name_suffix=" [left < 2p, right < 4p]"),
    Row("mulmod_raw_t<false>", "split", "mul", "TwTraits<TwS>: left < 2p, right < 6p as it comes: 12 p^2, th < 12 c < 2^32 for c < GPQ_SPLIT_CMAX, and the product leaves below 4p (12 c^2 < 1.95 * 2^59)",
        _mul_ref, (_lt(4),), lambda p, x, y, w0, w1: (model_mul7(x, w0, p),), xtop=_p(2), tw="var", wtop=_p(6), name_suffix=" [left < 2p, right < 6p]"),
    Row("mulmod_raw_t<false>", "wide", "mul", "TwTraits<TwW>: products (mulmod_lazy wants a*b < 2^122.8): left < 4p, right < 6p as it comes: 24 p^2 = 2^122.6; inv_from4: a product (< 4p) enters the inverse stages as it is",
        _mul_ref, (_lt(4),), lambda p, x, y, w0, w1: (model_mul7(x, w0, p),), xtop=_p(4), tw="var", wtop=_p(6), name_suffix=" [left < 4p, right < 6p]"),
    Row("mulmod_split<TwS>", "split", "mul", Q_SPLIT, _mul_ref, (_lt(3),), lambda p, x, y, w0, w1: (model_split(x, w0, w1, p),), xtop=_p(6), tw="S"),
    Row("mulmod_split<TwW>", "wide", "mul", Q_WIDE, _mul_ref, (_lt(2),), lambda p, x, y, w0, w1: (model_split(x, w0, w1, p),), xtop=_p(8), tw="W"),
    # ---- forward butterflies --------------------------------------------------------------------------------------------------
    Row("ct_bfly(uint64_t)", "fold", "ct", "in: x,y < 8p ; out: x,y < 8p.  x' = xs + t < 8p,  y' = xs + 4p - t in (0, 8p)",
        _ct_ref, (_lt(8), _open(8)), _ct_model(_m7, 4, 4), xtop=_p(8), ytop=_p(8), tw="7"),
    Row("ct_bfly(TwS)", "split", "ct", "Cooley-Tukey, split twiddle.  in: x,y < 6p ; out: x,y < 6p.  x' = xr + t < 6p,  y' = xr + 3p - t in (0, 6p)",
        _ct_ref, (_lt(6), _open(6)), _ct_model(_ms, 3, 3), xtop=_p(6), ytop=_p(6), tw="S"),
    Row("ct_bfly_wide<true>", "wide", "ct", 's even "B": subtract 4p.      in: x, y < 8p          out: x\' = xr + t < 6p, y\' = xr + 2p - t in (0, 6p)',
        _ct_ref, (_lt(6), _open(6)), _ct_model(_ms, 4, 2), xtop=_p(8), ytop=_p(8), tw="W"),
    Row("ct_bfly_wide<false>", "wide", "ct", 's odd  "A": no subtraction.   in: x, y < 6p          out: x\' = x + t < 8p,  y\' = x + 2p - t in (0, 8p); tests/test_lazy_ranges.py: y\' <= 8p - c - 2',
        _ct_ref, (_lt(8), (lambda p, c: 1, lambda p, c: 8 * p - c - 1)), _ct_model(_ms, 0, 2), xtop=_p(6), ytop=_p(6), tw="W"),
    # ---- inverse butterflies --------------------------------------------------------------------------------------------------
    Row("gs_bfly(uint64_t)", "fold", "gs", "Gentleman-Sande butterfly.  in: x,y < 4p ; out: x,y < 4p",
        _gs_ref, (_lt(4), _lt(4)), _gs_model(_m7, 4, 4), xtop=_p(4), ytop=_p(4), tw="7", kp=4),
    Row("gs_bfly_split<TwS>", "split", "gs", "Gentleman-Sande, split twiddle.  in: x,y < 3p ; out: x,y < 3p.",
        _gs_ref, (_lt(3), _lt(3)), _gs_model(_ms, 3, 3), xtop=_p(3), ytop=_p(3), tw="S", kp=3),
    Row("gs_bfly_wide<true>", "wide", "gs", "inverse data lives in [0, 4p): d = x + 4p - y in (0, 8p): a legal multiplicand, so the product leg y' = T' < 2p;   sum leg x' = v - [v >= 4p] 4p < 4p",
        _gs_ref, (_lt(4), _lt(2)), _gs_model(_ms, 4, 4), xtop=_p(4), ytop=_p(4), tw="W", kp=4),
    Row("gs_bfly_wide<false>", "wide", "gs", "a butterfly whose two inputs are BOTH product legs of the stage before (each < 2p) has v < 4p already and needs no conditional subtraction (CSUB = false)",
        _gs_ref, (_lt(4), _lt(2)), _gs_model(_ms, 4, 0), xtop=_p(2), ytop=_p(2), tw="W", kp=4),
    # ---- last inverse stage: canonical outputs --------------------------------------------------------------------------------
    Row("gs_last(LastK<uint64_t>)", "fold", "last", "Last inverse stage with the n^-1 scaling folded in, canonical outputs.  in: x,y < 4p.",
        lambda p, x, y, w, v: ((x + y) * w % p, (x - y) * v % p), (None, None),
        lambda p, x, y, w0, w1: (canon(model_mul7(x + y, w0, p), p, 2), canon(model_mul7(x + 4 * p - y, w1, p), p, 2)), xtop=_p(4), ytop=_p(4), tw="7", kp=4),
    Row("gs_last(LastK<TwS>)", "split", "last", "gs_last(LastK<TwS>): in: x,y < 3p; products < 3p",
        lambda p, x, y, w, v: ((x + y) * w % p, (x - y) * w % p), (None, None),
        lambda p, x, y, w0, w1: (canon(model_split(x + y, w0, w1, p), p, 2), canon(model_split(x + 3 * p - y, w0, w1, p), p, 2)), xtop=_p(3), ytop=_p(3), tw="S", kp=3),
    Row("gs_last(LastK<TwW>)", "wide", "last", "gs_last(LastK<TwW>): in: x,y < 4p; s < 8p: a legal multiplicand for the wide class; products < 2p",
        lambda p, x, y, w, v: ((x + y) * w % p, (x - y) * w % p), (None, None),
        lambda p, x, y, w0, w1: (csub(model_split(x + y, w0, w1, p), p), csub(model_split(x + 4 * p - y, w0, w1, p), p)), xtop=_p(4), ytop=_p(4), tw="W", kp=4),
    # ---- conditional subtractions: x - m [x >= m], on both sides of m and up to the top of the widest lazy range ---------------
    _unary("csub1", "fold", "x - m if x >= m else x, for m = p, 2p, 4p", 8, lambda p, x: csub(x, p)),
    _unary("csub2", "fold", "x - m if x >= m else x, for m = p, 2p, 4p", 8, lambda p, x: csub(x, 2 * p)),
    _unary("csub3", "fold", "the split class subtracts 3p (forward data < 6p, inverse data < 3p)", 8, lambda p, x: csub(x, 3 * p)),
    _unary("csub4", "fold", "x - m if x >= m else x, for m = p, 2p, 4p", 8, lambda p, x: csub(x, 4 * p)),
    # ---- canonicalising ops: the exact residue in [0, p) ----------------------------------------------------------------------
    _unary("canon4", "fold", "value < 4p -> [0,p)", 4, lambda p, x: x % p, model=_canon4),
    _unary("canon8", "fold", "value < 8p -> [0,p)", 8, lambda p, x: x % p, model=_canon8),
    _unary("canon_fold", "fold", "v mod p for v < 16p without compares", 16, lambda p, x: x % p, model=_fold),
    Row("mulmod_canon", "fold", "mul", "Exact a*b mod p for canonical a,b", lambda p, x, y, w, v: (x * w % p,), (None,),
        lambda p, x, y, w0, w1: (canon(model_mul7(x, w0, p), p, 2),), xtop=_p(1), tw="7"),
    Row("mulmod_canon_lazy", "fold", "mul", "Exact a*b mod p for a < 8p, b canonical.", lambda p, x, y, w, v: (x * w % p,), (None,),
        lambda p, x, y, w0, w1: (canon(model_mul7(x, w0, p), p, 2),), xtop=_p(8), tw="7"),
    Row("addmod_canon", "fold", "add", "Exact a+b mod p for a, b in [0, p]", lambda p, x, y, w, v: ((x + y) % p,), (None,),
        lambda p, x, y, w0, w1: (canon(x + y, p, 2),), xtop=lambda p: p, ytop=lambda p: p),
    Row("ref_fqmul", "fold", "mul", "fqmul(a, zeta) of src/ntt.c:32-35 is a * zeta_std mod p in [0, p) for every 64-bit a", lambda p, x, y, w, v: (x * w % p,), (None,),
        lambda p, x, y, w0, w1: (canon(model_mul7(x % p if x >= 8 * p else x, w0, p), p, 2),), xtop=lambda p: M64, tw="7"),
    Row("horner59", "fold", "horner", "r*2^59 + d (mod p), lazily: r < 4p, d < 2^59 -> (0, 4p).", lambda p, x, y, w, v: (x * B59 + y,), (_open(4),),
        lambda p, x, y, w0, w1: (model_horner(x, y, p),), xtop=_p(4), ytop=lambda p: M59),
    # ---- TwTraits members that are not the identity ---------------------------------------------------------------------------
    _unary("TwTraits<uint64_t>::canon_fwd", "fold", "forward data < 8p", 8, lambda p, x: x % p, model=_canon8),
    _unary("TwTraits<uint64_t>::canon_inv", "fold", "inverse data < 4p", 4, lambda p, x: x % p, model=_canon4),
    _unary("TwTraits<uint64_t>::inv_from8", "fold", "into the inverse range (< 4p) from a value < 8p", 8, lambda p, x: csub(x, 4 * p), _lt(4)),
    _unary("TwTraits<uint64_t>::left", "fold", "a forward-range value (< 8p) as the left (< 2p) operand", 8, lambda p, x: csub(csub(x, 4 * p), 2 * p), _lt(2)),
    _unary("TwTraits<uint64_t>::right", "fold", "a forward-range value (< 8p) as the right (< 4p) operand", 8, lambda p, x: csub(x, 4 * p), _lt(4)),
    _unary("TwTraits<TwS>::canon_fwd", "split", "forward data < 6p", 6, lambda p, x: x % p, model=_fold),
    _unary("TwTraits<TwS>::canon_inv", "split", "inverse data < 3p", 3, lambda p, x: x % p, model=_canon4),
    _unary("TwTraits<TwS>::inv_from4", "split", "into the inverse range (< 3p) from a value < 4p", 4, lambda p, x: csub(x, 2 * p), _lt(3)),
    _unary("TwTraits<TwS>::inv_from8", "split", "into the inverse range (< 3p) from a value < 8p", 8, lambda p, x: csub(csub(x, 4 * p), 2 * p), _lt(3)),
    _unary("TwTraits<TwS>::left", "split", "left < 2p from forward data (< 6p)", 6, lambda p, x: csub(csub(x, 4 * p), 2 * p), _lt(2)),
    _unary("TwTraits<TwW>::canon_fwd", "wide", "forward data < 6p after a finished transform (< 8p inside one)", 8, lambda p, x: x % p, model=_fold),
    _unary("TwTraits<TwW>::canon_inv", "wide", "inverse data < 4p", 4, lambda p, x: x % p, model=_canon4),
    _unary("TwTraits<TwW>::inv_from8", "wide", "into the inverse range (< 4p) from a value < 8p", 8, lambda p, x: csub(x, 4 * p), _lt(4)),
    _unary("TwTraits<TwW>::left", "wide", "left < 4p from forward data (< 6p after a finished transform)", 6, lambda p, x: csub(x, 4 * p), _lt(4)),
]

# Device functions of modarith.hpp that have no op of their own, and why.  (gs_bfly has one for its 7-mad form; its TwS / TwW overloads are
# one-line aliases of gs_bfly_split<TwS> and gs_bfly_wide<true>, which have theirs.)
HELPERS = {
    "mad_u64": "one v_mad_u64_u32: every multiply above is built from it",
    "pack64": "two dwords into a word: inside every multiply",
    "not_low27": "the complement of tl's high dword: inside every multiply",
    "pin_consts": "runs at the probe kernel's entry, as in the real kernels",
    "csub_by": "csub1 .. csub4 are its four instantiations",
    "mulmod_raw": "one-line alias of mulmod_raw_t<false>",
    "mulmod_lazy": "one-line alias of mulmod_raw_t<false>",
}
# what the probe calls a primitive that is overloaded or a template
PROBED_AS = {
    "mulmod_raw_t": ["mulmod_raw_t<false>", "mulmod_raw_t<true>"],
    "mulmod_split": ["mulmod_split<TwS>", "mulmod_split<TwW>"],
    "ct_bfly": ["ct_bfly(uint64_t)", "ct_bfly(TwS)"],
    "ct_bfly_wide": ["ct_bfly_wide<true>", "ct_bfly_wide<false>"],
    "gs_bfly": ["gs_bfly(uint64_t)"],
    "gs_bfly_split": ["gs_bfly_split<TwS>"],
    "gs_bfly_wide": ["gs_bfly_wide<true>", "gs_bfly_wide<false>"],
    "gs_last": ["gs_last(LastK<uint64_t>)", "gs_last(LastK<TwS>)", "gs_last(LastK<TwW>)"],
}


def cases():
    """(row, modulus) for every modulus the row's class admits"""
    return [(r, m) for r in ROWS for m in moduli() if m.admits(r.klass)]
