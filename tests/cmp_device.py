"""What the comparison tests on the device share (tests/test_he_cmp_gpu.py, tests/test_he_cmp_settings_gpu.py): tests/cmp_model.py's text over
separate public calls (tests/algo_device.py's DeviceOps plus the dense he_addpt), and CmpEnv, one shape's inputs -- four sets of ciphertexts
(A and B are one call's two inputs, C and D another's) and two dense plaintexts -- with what the separate calls and the restated reference
make of them.  A plain module: nothing here is collected."""
import random

from gpqhe_amd import ints_to_big, to_device
from tests import algo_model as am
from tests import cmp_model as cm
from tests.algo_device import GUARD_WORDS, DeviceOps, Env

PAIRS = {"AB": ("A", "B", "m1"), "CD": ("C", "D", "m2")}    # a call's first input, second input, plaintext


def _torch():
    import torch
    return torch


class CmpDeviceOps(DeviceOps):
    def addpt_dense(self, dst, src, m, pt_nu):              # m: ONE polynomial's big slab on the device
        torch = _torch()
        c = (self.g.big_addsub(torch.empty_like(src.c[0]), src.c[0], torch.cat([m] * self.e.batch), self.W, 0), src.c[1].clone())
        self._smod(c, src.l)
        dst.c, dst.l = c, src.l


class CmpEnv(Env):
    def __init__(self, engine_ctx, oracle_ctx, logn, logq, logdelta, batch, seed, down=0, W=None):
        Env.__init__(self, engine_ctx, oracle_ctx, logn, logq, logdelta, batch, seed, down, W, sets="ABCD")
        rng = random.Random(seed + 1000)
        h = 1 << (self.logql0 - 1)
        self.pt_host = {k: [rng.randrange(-h, h) for _ in range(self.g.n)] for k in ("m1", "m2")}      # about logql bits
        self.pt_host["m1"][:3] = [h - 1, -h, 0]
        self.pt_host["one"] = am.const_plaintext(self.g.n, am.const_int(1, logdelta))                  # he_const_pt(1)
        self.pt = {k: to_device(ints_to_big(v, self.W)) for k, v in self.pt_host.items()}
        self._sep = {}

    def _run(self, ops, fn, iter, t, a, b, m):
        L = ops.L - self.down
        if fn == "cmp":
            return cm.he_cmp(ops, am.Ct(a, L), am.Ct(b, L), iter, t)
        return cm.he_cmppt(ops, am.Ct(a, L), m, ops.Delta, iter, t)

    def separate(self, fn, iter, t, pair="AB", pt=None):
        """the sequence as separate public calls -> (c0, c1) tensors; made once"""
        key = (fn, iter, t, pair, pt)
        if key not in self._sep:
            a, b, m = PAIRS[pair]
            ops = CmpDeviceOps(self)
            clone = lambda d: (d[0].clone(), d[1].clone())
            out = self._run(ops, fn, iter, t, clone(self.dev[a]), clone(self.dev[b]), self.pt[pt or m])
            assert out.l == ops.L - self.down - cm.depth(iter, t)
            _torch().cuda.synchronize()
            self._sep[key] = out.c
        return self._sep[key]

    def restated(self, fn, iter, t, k, pair="AB", pt=None):
        """the sequence on the restated reference (Python integers) for ciphertext k -> (c0, c1) lists"""
        a, b, m = PAIRS[pair]
        ops = cm.BigintOps(self.o, self.logn, self.logq, self.logdelta, self.rlk_host)
        out = self._run(ops, fn, iter, t, tuple(self.cts[a][k]), tuple(self.cts[b][k]), self.pt_host[pt or m])
        c = ops.value(out)
        return list(c[0]), list(c[1])

    def cmp_workspace(self, fn, iter, t):
        """exactly the declared size, and a guard behind it"""
        torch = _torch()
        nbytes = self.g.he_cmp_workspace_bytes(fn == "cmppt", self.W, self.logq, self.logql0, self.logdelta, iter, t, self.batch)
        assert nbytes and nbytes % 8 == 0, self.g.lib.gpq_last_error().decode()
        ws = torch.full((nbytes // 8 + GUARD_WORDS,), 0x6B6B6B6B, dtype=torch.int64, device="cuda")
        return ws, nbytes // 8

    def other(self, fn, pair="AB", pt=None):
        a, b, m = PAIRS[pair]
        return self.dev[b] if fn == "cmp" else self.pt[pt or m]

    def cmp_call(self, fn, iter, t, c0, c1, other, o0, o1, ws):
        return self.g.he_cmp_call(o0, o1, c0, c1, other, self.rlk[0], self.rlk[1], self.W, self.logq, self.logql0, self.logdelta, iter, t, ws)
