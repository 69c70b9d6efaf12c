"""What the evaluator tests on the device share (tests/test_he_algo_gpu.py, tests/test_he_algo_shapes_gpu.py, tests/test_he_algo_settings_gpu.py):
DeviceOps, tests/algo_model.py's operations as separate public calls on the big slabs of a whole batch, and Env, one shape's context, oracle, key,
plaintext, inputs and what the separate calls make of them.  An Env may start `down` levels below the top (logql0 = logqL - down logDelta: the
INPUT's modulus, which every call then gets next to logqL) and may use slabs of any width W >= ceil(logql0 / 64).  A plain module: nothing here
is collected."""
import copy
import random

import numpy as np

from gpqhe_amd import ints_to_big, to_device
from tests import algo_model as am

GUARD_WORDS = 4096


def _torch():
    import torch
    return torch


class DeviceOps:
    """tests/algo_model.py's operations as separate public calls on the big slabs of a whole batch; a Ct's value is a pair of device tensors"""

    def __init__(self, env):
        self.e, self.g = env, env.g
        self.logn, self.n, self.logqL, self.s, self.W = env.logn, env.g.n, env.logq, env.logdelta, env.W
        self.L = env.logq // env.logdelta
        self.Delta = float(1 << env.logdelta)

    logql = am.BigintOps.logql
    mulpt_dim = am.BigintOps.mulpt_dim

    def alloc(self):
        return am.Ct()

    def value(self, ct):
        return ct.c

    def _dense(self, a):
        """he_const_pt's plaintext as a dense big slab, once per ciphertext of the batch"""
        one = ints_to_big(am.const_plaintext(self.n, a), self.W)
        return to_device(np.concatenate([one] * self.e.batch))

    def copy(self, dst, src):
        dst.c, dst.l = (src.c[0].clone(), src.c[1].clone()), src.l

    def _smod(self, c, l):
        self.g.he_rs(c[0], c[1], self.W, 0, self.logql(l))

    def neg(self, ct):
        ct.c = tuple(self.g.big_addsub(_torch().empty_like(x), x, None, self.W, 2) for x in ct.c)
        self._smod(ct.c, ct.l)

    def add(self, dst, a, b):
        assert a.l == b.l
        c = tuple(self.g.big_addsub(_torch().empty_like(x), x, y, self.W, 0) for x, y in zip(a.c, b.c))
        self._smod(c, a.l)
        dst.c, dst.l = c, a.l

    def _pt(self, dst, src, re, mode):
        c = (self.g.big_addsub(_torch().empty_like(src.c[0]), src.c[0], self._dense(am.const_int(re, self.s)), self.W, mode), src.c[1].clone())
        self._smod(c, src.l)
        dst.c, dst.l = c, src.l

    def addpt(self, dst, src, re):
        self._pt(dst, src, re, 0)

    def subpt(self, dst, src, re):
        self._pt(dst, src, re, 1)

    def moddown(self, ct):
        ct.c = (ct.c[0].clone(), ct.c[1].clone())
        ct.l -= 1
        self._smod(ct.c, ct.l)

    def rs(self, ct):
        ct.c = (ct.c[0].clone(), ct.c[1].clone())
        self.g.he_rs(ct.c[0], ct.c[1], self.W, self.s, self.logql(ct.l - 1))
        ct.l -= 1

    def mul(self, dst, a, b):
        assert a.l == b.l
        torch = _torch()
        dimP, dimA, dimB, _ = self.g.he_dims(self.logqL, self.logql(a.l))
        c = (torch.empty_like(a.c[0]), torch.empty_like(a.c[0]))
        self.g.he_mul(c[0], c[1], a.c[0], a.c[1], b.c[0], b.c[1], self.e.rlk[0], self.e.rlk[1], self.W, self.logql(a.l), dimA, dimB, dimP)
        dst.c, dst.l = c, a.l

    def _mulpt(self, dst, src, mdev):
        torch = _torch()
        c = (torch.empty_like(src.c[0]), torch.empty_like(src.c[0]))
        self.g.he_mulpt(c[0], c[1], src.c[0], src.c[1], mdev, self.W, self.logql(src.l), self.mulpt_dim(src.l))
        dst.c, dst.l = c, src.l

    def mulpt(self, dst, src, m):
        self._mulpt(dst, src, _torch().cat([m] * self.e.batch))

    def mulpt_const(self, dst, src, re):
        self._mulpt(dst, src, self._dense(am.const_int(re, self.s)))


class Env:
    """one ring: context, oracle, key, plaintext, input sets centred mod 2^logql0 and what the separate calls make of them"""

    def __init__(self, engine_ctx, oracle_ctx, logn, logq, logdelta, batch, seed, down=0, W=None, sets="AB"):
        from oracle import bigint_ref as br
        self.logn, self.logq, self.logdelta, self.batch, self.down = logn, logq, logdelta, batch, down
        self.logql0 = logq - down * logdelta
        assert self.logql0 >= 1
        probe = engine_ctx(logn, am.primes_for(logn, logq))
        dimevk = probe.he_dims(logq, logq)[3]
        self.dimevk = dimevk
        self.g, self.o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
        assert br.he_dims(logn, self.o.p, logq, logq)[3] == dimevk
        n = self.g.n
        self.W = (logq + 63) // 64 if W is None else W
        assert self.W >= (self.logql0 + 63) // 64
        self.dimpt = (self.logql0 + 1 + logdelta + logn) // 59 + 1
        rng = random.Random(seed)
        self.rlk_host = (self.o.gen(seed * 100 + 1, dimevk), self.o.gen(seed * 100 + 2, dimevk))
        self.rlk = tuple(to_device(k) for k in self.rlk_host)
        self.m_host = [rng.randrange(-(1 << logdelta), 1 << logdelta) for _ in range(n)]
        self.m = to_device(ints_to_big(self.m_host, self.W))
        h = 1 << (self.logql0 - 1)
        self.cts, self.dev = {}, {}
        for which in sets:
            cts = [[[rng.randrange(-h, h) for _ in range(n)] for _ in range(2)] for _ in range(batch)]
            cts[0][0][:6] = [0, -1, h - 1, -h, 1, -(h - 1)]
            self.cts[which] = cts
            self.dev[which] = tuple(to_device(np.concatenate([ints_to_big(ct[c], self.W) for ct in cts])) for c in range(2))
        self._separate = {}

    def on(self, g):
        """the same inputs (shared, read-only) on another context of the same ring and primes; what the separate calls make of them there is its own"""
        assert g.n == self.g.n
        e = copy.copy(self)
        e.g, e._separate = g, {}
        return e

    def separate(self, kind, iter, which):
        """the sequence as separate public calls -> (c0, c1) tensors; made once"""
        key = (kind, iter, which)
        if key not in self._separate:
            ops = DeviceOps(self)
            d = self.dev[which]
            out = am.run(kind, ops, am.Ct((d[0].clone(), d[1].clone()), ops.L - self.down), iter, self.m)
            assert out.l == ops.L - self.down - am.depth(kind, iter)
            _torch().cuda.synchronize()
            self._separate[key] = out.c
        return self._separate[key]

    def restated(self, kind, iter, which, k):
        """the sequence on the restated reference (Python integers) for ciphertext k of set `which` -> (c0, c1) lists"""
        ops = am.BigintOps(self.o, self.logn, self.logq, self.logdelta, self.rlk_host)
        ct = self.cts[which][k]
        out = am.run(kind, ops, am.Ct((ct[0], ct[1]), ops.L - self.down), iter, self.m_host)
        c = ops.value(out)
        return list(c[0]), list(c[1])

    def workspace_bytes(self, kind, iter):
        return self.g.he_algo_workspace_bytes(kind, self.W, self.logq, self.logql0, self.logdelta, iter, self.batch)

    def workspace(self, kind, iter, logql=None):
        """exactly the declared size, and a guard behind it"""
        torch = _torch()
        nbytes = self.g.he_algo_workspace_bytes(kind, self.W, self.logq, logql or self.logql0, self.logdelta, iter, self.batch)
        assert nbytes and nbytes % 8 == 0, self.g.lib.gpq_last_error().decode()
        ws = torch.full((nbytes // 8 + GUARD_WORDS,), 0x6B6B6B6B, dtype=torch.int64, device="cuda")
        return ws, nbytes // 8

    def call(self, kind, iter, c0, c1, o0, o1, ws):
        g = self.g
        return g.he_algo_call(kind, o0, o1, c0, c1, self.rlk[0], self.rlk[1], self.W, self.logq, self.logql0, self.logdelta, iter, ws, self.m, self.dimpt)
