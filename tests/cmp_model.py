"""he_cmp_core / he_cmp / he_cmppt of src/he-algo.c:460-548 in Python, call for call, over the abstract operations of tests/algo_model.py (the
nested he_inv is algo_model's own text), plus the one operation they add: he_addpt by an arbitrary DENSE plaintext (src/he-add.c:80-100), given
to each of the three implementations by subclassing.  tests/test_cmp_model.py pins the three to each other; the GPU tests run the same text
over separate device calls and compare gpq_he_cmp / gpq_he_cmppt with it word for word.  TEST INFRASTRUCTURE ONLY."""
import math

from oracle import bigint_ref as br
from tests import algo_model as am


def rounds(alpha):
    """he_cmp's t (src/he-algo.c:519-520), the C double expression; defined for 1 <= alpha <= 52"""
    return int(math.log2(alpha / math.log2(1 + math.pow(2, -alpha))))


def depth(iter, t):
    return (3 + iter) * (1 + t)


def he_cmp_core(ops, an, ct, iter, t, dead_bn=True):        # :460-507; dead_bn False: the bn nobody reads afterwards is not computed
    bn, inv = ops.alloc(), ops.alloc()
    ops.copy(inv, an)                                       # :466
    ops.mulpt_const(inv, inv, 0.5)                          # :473
    ops.rs(inv)
    ops.copy(inv, am.he_inv(ops, inv, iter))                # :475  he_inv(&inv, &inv, ..): its he_copy_ct into the destination
    ops.mulpt_const(an, ct, 0.5)                            # :477
    ops.rs(an)
    for _ in range(iter + 1):
        ops.moddown(an)                                     # :479-480
    ops.mul(an, an, inv)                                    # :482
    ops.rs(an)
    if dead_bn or t:
        ops.subpt(bn, an, 1)                                # :485
        ops.neg(bn)                                         # :486
    for r in range(t):
        ops.mul(an, an, an)                                 # :489
        ops.rs(an)
        ops.mul(bn, bn, bn)                                 # :491
        ops.rs(bn)
        ops.add(inv, an, bn)                                # :493
        ops.copy(inv, am.he_inv(ops, inv, iter))            # :494
        for _ in range(iter + 1):
            ops.moddown(an)                                 # :495-496
        ops.mul(an, an, inv)                                # :497
        ops.rs(an)
        if dead_bn or r + 1 < t:
            ops.subpt(bn, an, 1)                            # :499
            ops.neg(bn)                                     # :500
    return an


def he_cmp(ops, ct1, ct2, iter, t, dead_bn=True):           # :514-530 with t in place of alpha
    an, out = ops.alloc(), ops.alloc()
    ops.add(an, ct1, ct2)                                   # :525
    he_cmp_core(ops, an, ct1, iter, t, dead_bn)
    ops.copy(out, an)                                       # :527
    return out


def he_cmppt(ops, ct, m, pt_nu, iter, t, dead_bn=True):     # :532-548; m = pt->m's integers, pt_nu = pt->nu
    an, out = ops.alloc(), ops.alloc()
    ops.addpt_dense(an, ct, m, pt_nu)                       # :543
    he_cmp_core(ops, an, ct, iter, t, dead_bn)
    ops.copy(out, an)                                       # :545
    return out


class BigintOps(am.BigintOps):
    def addpt_dense(self, dst, src, m, pt_nu):              # src/he-add.c:80-100
        self._set(dst, br.he_addpt(self.value(src), m, self.q(src.l)), src.l, src.nu if src.nu >= pt_nu else pt_nu, src.B)


class LazyOps(am.LazyOps):
    def addpt_dense(self, dst, src, m, pt_nu):              # one more term of the sum: (m, 0)
        lin = self._lin(src).plus(am.Lin([(1, (list(m), [0] * self.n))], 0))
        dst.c, dst.l, dst.nu, dst.B = lin, src.l, src.nu if src.nu >= pt_nu else pt_nu, src.B


class RefOps(am.RefOps):
    def addpt_dense(self, dst, src, m, pt_nu):
        d, x = self._slots(dst, src)
        self.R.pt_set(0, m, pt_nu)
        self.R.he_addpt(d, x, 0)
        self._get(dst, d)
