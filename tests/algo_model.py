"""The evaluators of src/he-algo.c:131-458 -- he_inv, he_sqrt, he_sigmoid, he_log, he_exp -- once more, in Python, call for call, over an abstract
set of operations (the reference's own calls): alloc, copy, neg, add, addpt, subpt, moddown, mul, rs, mulpt_const, mulpt.  A ciphertext is a `Ct`
(two coefficient vectors, l, nu, B) that the operations fill in; three implementations run the same text:

  BigintOps    the restated reference (oracle/bigint_ref.py around the C oracle), Python integers, the reference's l / nu / B formulas;
  LazyOps      the same, but every additive call (copy, neg, add, addpt, subpt, moddown) only extends a signed sum, and ONE mpi_smod at the level
               the chain has reached is taken when a product, a rescale or the caller needs the words -- what gpq_he_lin_const computes;
  RefOps       the EXECUTED reference through oracle/ref.py's per-call slots (values parked in Python between calls: the driver has 8 slots).

tests/test_algo_model.py pins the three to each other; the GPU tests run the same text once more over separate device calls and compare the
evaluators (gpq_he_inv, ...) with it word for word.  TEST INFRASTRUCTURE ONLY."""
import math
import struct
from fractions import Fraction

from oracle import bigint_ref as br

KINDS = ("inv", "sqrt", "sigmoid", "log", "exp")

# The slab shapes the evaluators are pinned at away from (logn 7, q_L = 2^200, Delta = 2^30, the top level, W = 4):
# cell -> (logn, logqL, logDelta, levels below the top the input sits at, W, batch, [(kind, iter)]).  tests/test_algo_model.py runs the collapse at every
# one without a device, tests/test_he_algo_shapes_gpu.py the library.
SLAB_SHAPES = {
    "A": (7, 200, 30, 2, 4, 2, [("inv", 2), ("sqrt", 2), ("sigmoid", 0), ("log", 0), ("exp", 0)]),   # logql != logqL in every operation; ends at 2^20
    "B": (7, 200, 20, 2, 4, 2, [("inv", 3), ("sqrt", 3), ("exp", 2)]),                               # a third iteration; another scale
    "C": (7, 300, 59, 0, 5, 2, [("inv", 1), ("sqrt", 1), ("sigmoid", 0), ("log", 0), ("exp", 0)]),   # constants next to INT64_MAX; depth 4 ends at 2^64
    "D": (7, 200, 4, 40, 1, 2, [("log", 0), ("inv", 2), ("sigmoid", 0)]),                            # W = 1; constants that round to 0
    "E1": (7, 438, 30, 0, 7, 2, [("sigmoid", 0), ("inv", 2)]),                                       # 8/16/24 limbs, fewer with every level
    "E2": (7, 438, 30, 8, 4, 2, [("log", 0), ("exp", 1)]),                                           # P sized for q_L far above q_l = 2^198
    "F": (7, 850, 30, 0, 14, 2, [("inv", 1)]),                                                       # a 16-word P
    "G": (13, 200, 30, 1, 4, 3, [("sqrt", 1), ("log", 0)]),                                          # a two-pass ring below the top
}


def primes_for(logn, logq):
    """an upper bound of dimevk (src/precomp.c:407) for q_L = 2^logq that needs no prime: the chain's primes have at most 60 bits, so P has at
    most 60 per limb.  A probe context of this many primes (at least the 12 every other test probes with) answers gpq_he_dims for the shape."""
    dimP = (logq + 1 + logn) // 59 + 1
    return max(12, ((logq + 1) + (60 * dimP + logq + 1) + logn) // 59 + 1)


def depth(kind, iter=0):
    return {"inv": iter + 1, "sqrt": 2 * iter, "sigmoid": 4, "log": 4, "exp": 4 + iter}[kind]


def const_int(re, logdelta):
    """he_const_pt's integer (src/he-encode.c:119-125) for Delta = 2^logdelta: round half away from zero of the exact product"""
    v = Fraction(re) * (1 << logdelta)
    a = (abs(v) * 2 + 1) // 2
    return int(-a if v < 0 else a)


def const_plaintext(n, a):
    m = [0] * n
    m[0] = a
    return m


class Ct:
    __slots__ = ("c", "l", "nu", "B")

    def __init__(self, c=None, l=0, nu=0.0, B=0.0):
        self.c, self.l, self.nu, self.B = c, l, nu, B


# ---------------------------------------------------------------------------
# the sequences (ops.alloc() = he_alloc_ct; constants are the reference's C double expressions, IEEE doubles here as there)
# ---------------------------------------------------------------------------
def he_inv(ops, ct, iter):                                  # src/he-algo.c:131-164
    tmp, an, bn, out = ops.alloc(), ops.alloc(), ops.alloc(), ops.alloc()
    ops.copy(tmp, ct)                                       # :145
    ops.neg(tmp)                                            # :146
    ops.addpt(an, tmp, 2)                                   # :147
    ops.moddown(an)                                         # :148
    ops.addpt(bn, tmp, 1)                                   # :149
    for _ in range(iter):
        ops.mul(bn, bn, bn)                                 # :151
        ops.rs(bn)
        ops.addpt(tmp, bn, 1)                               # :153
        ops.mul(an, an, tmp)                                # :154
        ops.rs(an)
    ops.copy(out, an)                                       # :157
    return out


def he_sqrt(ops, ct, iter):                                 # :166-206
    tmp, an, bn, out = ops.alloc(), ops.alloc(), ops.alloc(), ops.alloc()
    ops.copy(an, ct)                                        # :184
    ops.subpt(bn, ct, 1)                                    # :185
    for _ in range(iter):
        ops.mulpt_const(tmp, bn, 0.5)                       # :188
        ops.rs(tmp)
        ops.subpt(tmp, tmp, 1)                              # :190
        ops.neg(tmp)
        ops.moddown(an)                                     # :192
        ops.mul(an, an, tmp)                                # :193
        ops.rs(an)
        ops.subpt(tmp, bn, 3)                               # :196
        ops.mulpt_const(tmp, tmp, 0.25)                     # :197
        ops.rs(tmp)
        ops.mul(bn, bn, bn)                                 # :199
        ops.rs(bn)
        ops.mul(bn, bn, tmp)                                # :201
        ops.rs(bn)
    ops.copy(out, an)                                       # :205
    return out


def he_sigmoid(ops, ct):                                    # :208-277
    ct2, ct4, ct8, ct3x, ct13, ct7x, ct57, ct9x, out = (ops.alloc() for _ in range(9))
    ops.mul(ct2, ct, ct); ops.rs(ct2)                       # :223-224
    ops.mul(ct4, ct2, ct2); ops.rs(ct4)                     # :226-227
    ops.mul(ct8, ct4, ct4); ops.rs(ct8)                     # :229-230
    ops.mulpt_const(ct3x, ct, -1. / 48); ops.rs(ct3x)       # :232-234
    ops.addpt(ct13, ct2, (1. / 4) / (-1. / 48))             # :236-237
    ops.mul(ct13, ct3x, ct13); ops.rs(ct13)                 # :238-239
    ops.moddown(ct13); ops.moddown(ct13)                    # :240-241
    ops.mulpt_const(ct7x, ct, -17. / 80640); ops.rs(ct7x)   # :243-245
    ops.addpt(ct57, ct2, (1. / 480) / (-17. / 80640))       # :247-248
    ops.mul(ct57, ct7x, ct57); ops.rs(ct57)                 # :249-250
    ops.mul(ct57, ct4, ct57); ops.rs(ct57)                  # :251-252
    ops.moddown(ct57)                                       # :253
    ops.mulpt_const(ct9x, ct, 31. / 1451520); ops.rs(ct9x)  # :255-257
    ops.moddown(ct9x); ops.moddown(ct9x)                    # :258-259
    ops.mul(ct9x, ct9x, ct8); ops.rs(ct9x)                  # :260-261
    ops.add(out, ct13, ct57)                                # :263
    ops.add(out, out, ct9x)                                 # :264
    ops.addpt(out, out, 1. / 2)                             # :265-266
    return out


def _log_half(ops, acc, x, ct2, ct4, ct8, tmp, k6, k4, k2, k0, kx):
    ops.copy(acc, ct8)                                      # :301 / :327
    ops.mulpt_const(tmp, ct2, k6); ops.rs(tmp)              # :302-304
    ops.mul(tmp, tmp, ct4); ops.rs(tmp)                     # :305-306
    ops.add(acc, acc, tmp)                                  # :307
    ops.mulpt_const(tmp, ct4, k4); ops.rs(tmp)              # :308-310
    ops.add(acc, acc, tmp)                                  # :311
    ops.mulpt_const(tmp, ct2, k2); ops.rs(tmp)              # :312-314
    ops.moddown(tmp)                                        # :315
    ops.add(acc, acc, tmp)                                  # :316
    ops.addpt(acc, acc, k0)                                 # :317-318
    ops.mulpt_const(tmp, x, kx); ops.rs(tmp)                # :319-321 / :345-347
    while tmp.l > acc.l:                                    # :322-323 (two he_moddown) / :348 (one)
        ops.moddown(tmp)
    ops.mul(acc, tmp, acc); ops.rs(acc)                     # :324-325


def he_log(ops, ct):                                        # :279-361
    ct2, ct4, ct8, ctodd, cteven, tmp, out = (ops.alloc() for _ in range(7))
    ops.mul(ct2, ct, ct); ops.rs(ct2)                       # :292-293
    ops.mul(ct4, ct2, ct2); ops.rs(ct4)                     # :295-296
    ops.mul(ct8, ct4, ct4); ops.rs(ct8)                     # :298-299
    _log_half(ops, ctodd, ct, ct2, ct4, ct8, tmp, 9. / 7., 9. / 5., 9. / 3., 9, 1. / 9.)                 # :300-325
    _log_half(ops, cteven, ct2, ct2, ct4, ct8, tmp, 10. / 8., 10. / 6., 10. / 4., 10. / 2, -1. / 10.)    # :326-350
    ops.add(out, ctodd, cteven)                             # :352
    return out


def he_exp(ops, ct, iter, m):                               # :364-458; m = he_ecd of the constant vector a / 2^iter (:444-448), nu = Delta
    act, ct2, ct4, ct01, ct23, ct0123, ct45, ct67, ct4567, out = (ops.alloc() for _ in range(10))
    ops.mulpt(act, ct, m); ops.rs(act)                      # :449-450
    ops.mul(ct2, act, act); ops.rs(ct2)                     # :379-380
    ops.mul(ct4, ct2, ct2); ops.rs(ct4)                     # :382-383
    ops.addpt(ct01, act, 1.0)                               # :385-386
    ops.mulpt_const(ct01, ct01, 1.0); ops.rs(ct01)          # :387-388
    ops.moddown(ct01)                                       # :389
    ops.addpt(ct23, act, 3.0)                               # :391-392
    ops.mulpt_const(ct23, ct23, 1.0 / 6); ops.rs(ct23)      # :393-395
    ops.mul(ct23, ct2, ct23); ops.rs(ct23)                  # :396-397
    ops.add(ct0123, ct01, ct23)                             # :399
    ops.moddown(ct0123)                                     # :400
    ops.addpt(ct45, act, 5.0)                               # :402-403
    ops.mulpt_const(ct45, ct45, 1.0 / 120); ops.rs(ct45)    # :404-406
    ops.moddown(ct45)                                       # :407
    ops.addpt(ct67, act, 7.0)                               # :409-410
    ops.mulpt_const(ct67, ct67, 1.0 / 5040); ops.rs(ct67)   # :411-413
    ops.mul(ct67, ct2, ct67); ops.rs(ct67)                  # :414-415
    ops.add(ct4567, ct45, ct67)                             # :417
    ops.mul(ct4567, ct4, ct4567); ops.rs(ct4567)            # :418-419
    ops.add(out, ct0123, ct4567)                            # :421
    for _ in range(iter):
        ops.mul(out, out, out); ops.rs(out)                 # :453-454
    return out


def run(kind, ops, ct, iter=0, m=None):
    if kind == "inv":
        return he_inv(ops, ct, iter)
    if kind == "sqrt":
        return he_sqrt(ops, ct, iter)
    if kind == "sigmoid":
        return he_sigmoid(ops, ct)
    if kind == "log":
        return he_log(ops, ct)
    return he_exp(ops, ct, iter, m)


# ---------------------------------------------------------------------------
# the restated reference
# ---------------------------------------------------------------------------
def brs_bound(n):
    return math.sqrt(n / 3.) * (3 + 8 * math.sqrt(64))      # src/precomp.c:416


class BigintOps:
    """o = oracle.OracleCtx; rlk = (p0, p1) NTT-domain key slabs of dimevk limbs; Bmult = the reference's table by level (zeros: B is then not the
    reference's, and nobody compares it)"""

    def __init__(self, o, logn, logqL, logdelta, rlk, Bmult=None, Brs=None):
        self.o, self.logn, self.n, self.logqL, self.s, self.rlk = o, logn, 1 << logn, logqL, logdelta, rlk
        self.L = logqL // logdelta
        self.Delta = float(1 << logdelta)
        self.Bmult = Bmult if Bmult is not None else [0.0] * (self.L + 1)
        self.Brs = brs_bound(self.n) if Brs is None else Brs

    def logql(self, l):
        return self.logqL - (self.L - l) * self.s

    def q(self, l):
        return 1 << self.logql(l)

    def alloc(self):
        return Ct()

    def value(self, ct):
        """the coefficient vectors as they stand"""
        return ct.c

    def _set(self, dst, c, l, nu, B):
        dst.c, dst.l, dst.nu, dst.B = (list(c[0]), list(c[1])), l, nu, B

    def copy(self, dst, src):                               # he_copy_ct, src/he-mem.c:88-97
        self._set(dst, self.value(src), src.l, src.nu, src.B)

    def neg(self, ct):                                      # src/he-add.c:125-142
        ct.c = br.he_neg(self.value(ct), self.q(ct.l))

    def add(self, dst, a, b):                               # :32-53
        assert a.l == b.l
        self._set(dst, br.he_add(self.value(a), self.value(b), self.q(a.l)), a.l, a.nu if a.nu >= b.nu else b.nu, a.B + b.B)

    def _pt(self, dst, src, re, f):
        m = const_plaintext(self.n, const_int(re, self.s))
        self._set(dst, f(self.value(src), m, self.q(src.l)), src.l, src.nu if src.nu >= self.Delta else self.Delta, src.B)

    def addpt(self, dst, src, re):                          # :80-100
        self._pt(dst, src, re, br.he_addpt)

    def subpt(self, dst, src, re):                          # :102-123
        self._pt(dst, src, re, br.he_subpt)

    def moddown(self, ct):                                  # src/he-rescale.c:56-70
        q = self.q(ct.l - 1)
        ct.c = tuple([br.mpi_smod(v, q) for v in c] for c in self.value(ct))
        ct.l -= 1

    def rs(self, ct):                                       # src/he-rescale.c:33-54
        q, D = self.q(ct.l - 1), 1 << self.s
        ct.c = tuple([br.mpi_smod(br.mpi_rdiv(v, D), q) for v in c] for c in self.value(ct))
        ct.l, ct.nu, ct.B = ct.l - 1, ct.nu / self.Delta, ct.B / self.Delta + self.Brs

    def mul(self, dst, a, b):                               # src/he-mult.c:88-156
        assert a.l == b.l
        l, lq, n = a.l, self.logql(a.l), self.n
        dimP, dimA, dimB, _ = br.he_dims(self.logn, self.o.p, self.logqL, lq)
        c = br.he_mul(self.o, self.value(a), self.value(b), self.rlk[0][:dimB * n], self.rlk[1][:dimB * n], dimP, dimA, dimB, lq)
        nu = a.nu * b.nu                                    # :93, stored before :94-95 read the operands' nu: a destination that is an operand
        nu1, nu2 = (nu if dst is a else a.nu), (nu if dst is b else b.nu)      # hands them the NEW nu
        B = nu1 * b.B + nu2 * a.B + a.B * b.B + self.Bmult[l]
        self._set(dst, c, l, nu, B)

    def mulpt_dim(self, l):
        return (self.logql(l) + 1 + self.s + self.logn) // 59 + 1          # src/he-mult.c:168 with pt->nu = Delta

    def mulpt(self, dst, src, m):                           # src/he-mult.c:159-196, pt->nu = Delta
        c = br.he_mulpt(self.o, self.value(src), m, self.mulpt_dim(src.l), self.logql(src.l))
        self._set(dst, c, src.l, src.nu * self.Delta, src.B * self.Delta)

    def mulpt_const(self, dst, src, re):                    # he_const_pt, then he_mulpt by the DENSE plaintext through the RNS path
        self.mulpt(dst, src, const_plaintext(self.n, const_int(re, self.s)))


class Lin:
    """a signed sum of coefficient-vector pairs plus the integer a at coefficient 0 of c0, not reduced yet"""

    def __init__(self, terms, a):
        self.terms, self.a = terms, a

    def scaled(self, sign):
        return Lin([(sign * s, c) for s, c in self.terms], sign * self.a)

    def plus(self, other):
        return Lin(self.terms + other.terms, self.a + other.a)


class LazyOps(BigintOps):
    """BigintOps with every additive call deferred: the collapse of src/he-add.c:32-140, he_moddown and he_copy_ct into one sum and one mpi_smod"""

    def __init__(self, *args, **kw):
        BigintOps.__init__(self, *args, **kw)
        self.most_terms = 0
        self.sums = 0                                       # sums that were materialised: each is at most one gpq_he_lin_const of an evaluator

    def _lin(self, ct):
        return ct.c if isinstance(ct.c, Lin) else Lin([(1, ct.c)], 0)

    def value(self, ct):
        if isinstance(ct.c, Lin):
            lin, q, n = ct.c, self.q(ct.l), self.n
            self.most_terms = max(self.most_terms, len(lin.terms))
            self.sums += 1
            c0 = [br.mpi_smod(sum(s * c[0][i] for s, c in lin.terms) + (lin.a if i == 0 else 0), q) for i in range(n)]
            c1 = [br.mpi_smod(sum(s * c[1][i] for s, c in lin.terms), q) for i in range(n)]
            ct.c = (c0, c1)
        return ct.c

    def copy(self, dst, src):
        dst.c, dst.l, dst.nu, dst.B = self._lin(src), src.l, src.nu, src.B

    def neg(self, ct):
        ct.c = self._lin(ct).scaled(-1)

    def add(self, dst, a, b):
        assert a.l == b.l
        dst.c, dst.l, dst.nu, dst.B = self._lin(a).plus(self._lin(b)), a.l, a.nu if a.nu >= b.nu else b.nu, a.B + b.B

    def _pt(self, dst, src, re, f):
        a = const_int(re, self.s) * (1 if f is br.he_addpt else -1)
        dst.c, dst.l, dst.nu, dst.B = self._lin(src).plus(Lin([], a)), src.l, src.nu if src.nu >= self.Delta else self.Delta, src.B

    def moddown(self, ct):
        ct.c, ct.l = self._lin(ct), ct.l - 1


# ---------------------------------------------------------------------------
# the executed reference
# ---------------------------------------------------------------------------
def _f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


class RefOps:
    """R = oracle.ref.Ref after init() and evk_set('rlk', ..).  A Ct's value lives in Python between calls (exactly: integers, and the doubles as
    their bits); each call loads its operands into the driver's slots -- the same slot for the same Ct, so that a destination that is an operand
    is one to the reference too -- runs the reference's function and reads the destination back."""

    def __init__(self, R, logdelta):
        self.R, self.n, self.s, self.Delta = R, R.n, logdelta, float(1 << logdelta)

    def alloc(self):
        return Ct()

    def value(self, ct):
        return ct.c

    def _slots(self, *cts):
        ids, slot = {}, []
        for ct in cts:
            if id(ct) not in ids:
                ids[id(ct)] = len(ids)
                if ct.c is not None:
                    self.R.ct_set(ids[id(ct)], ct.c, ct.l, ct.nu, ct.B)
            slot.append(ids[id(ct)])
        return slot

    def _get(self, dst, k):
        c, l, nu, B = self.R.ct_get(k)
        dst.c, dst.l, dst.nu, dst.B = c, l, _f(nu), _f(B)

    def copy(self, dst, src):
        dst.c, dst.l, dst.nu, dst.B = (list(src.c[0]), list(src.c[1])), src.l, src.nu, src.B

    def neg(self, ct):
        k, = self._slots(ct)
        self.R.he_neg(k); self._get(ct, k)

    def add(self, dst, a, b):
        d, x, y = self._slots(dst, a, b)
        self.R.he_add(d, x, y); self._get(dst, d)

    def _pt(self, dst, src, m, call):
        d, x = self._slots(dst, src)
        self.R.pt_set(0, m, self.Delta)
        call(d, x, 0); self._get(dst, d)

    def addpt(self, dst, src, re):
        self._pt(dst, src, const_plaintext(self.n, const_int(re, self.s)), self.R.he_addpt)

    def subpt(self, dst, src, re):
        self._pt(dst, src, const_plaintext(self.n, const_int(re, self.s)), self.R.he_subpt)

    def moddown(self, ct):
        k, = self._slots(ct)
        self.R.he_moddown(k); self._get(ct, k)

    def rs(self, ct):
        k, = self._slots(ct)
        self.R.he_rs(k); self._get(ct, k)

    def mul(self, dst, a, b):
        d, x, y = self._slots(dst, a, b)
        self.R.he_mul(d, x, y); self._get(dst, d)

    def mulpt(self, dst, src, m):
        self._pt(dst, src, m, self.R.he_mulpt)

    def mulpt_const(self, dst, src, re):
        self._pt(dst, src, const_plaintext(self.n, const_int(re, self.s)), self.R.he_mulpt)
