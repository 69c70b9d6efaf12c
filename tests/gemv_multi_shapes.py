"""Inputs of tests/test_he_gemv_multi_gpu.py: random ciphertexts, several matrices' diagonals and the rotation keys he_gemv needs, all made on
the host with numpy (the parts of tests/test_he_gemv_planned_gpu.py's Shape that several plans on one ciphertext need)."""
import numpy as np
import torch

from gpqhe_amd import gemv_steps, to_device

LOGDELTA = 30


def dimpt_of(logql, logn):
    return (logql + 1 + LOGDELTA + logn) // 59 + 1           # src/he-mult.c:168 with nu = 2^LOGDELTA


class MultiShape:
    def __init__(self, engine_ctx, logn, logq, slots, batch, seed=None, limbs=0):
        self.logn, self.logq, self.slots, self.batch = logn, logq, slots, batch
        self.n, self.W = 1 << logn, logq // 64 + 1
        self.dimP, _, self.dimB, _ = engine_ctx(logn, 20).he_dims(logq, logq)
        self.dimpt = dimpt_of(logq, logn)
        self.g = engine_ctx(logn, max(self.dimB, self.dimpt, limbs))
        self.rng = np.random.default_rng(logn if seed is None else seed)
        self.n1, self.n2 = gemv_steps(slots)
        p = self.g.p
        self.keys = [None] * slots
        for r in sorted(set(range(self.n1)) | {i * self.n1 for i in range(self.n2)}):
            self.keys[r] = tuple(to_device(np.concatenate([self.rng.integers(0, p[d], size=self.n, dtype=np.uint64) for d in range(self.dimB)])) for _ in range(2))

    def diagonals(self, bits=LOGDELTA, zero=()):
        """slots diagonals of small positive coefficients below 2^bits, drawn anew at every call; those listed in `zero` are zero"""
        dg = np.zeros((self.slots, self.W, self.n), dtype=np.uint64)
        dg[:, 0] = self.rng.integers(-(1 << 62), 1 << 62, size=(self.slots, self.n), dtype=np.int64).view(np.uint64) >> np.uint64(64 - bits)
        for k in zero:
            dg[k] = 0
        return to_device(dg.reshape(-1))

    def plan(self, diag):
        return self.g.gemv_plan(diag, self.slots, self.W, self.logq, self.dimpt)

    def ciphertexts(self, batch=None):
        batch, W, n = batch or self.batch, self.W, self.n
        cts = np.zeros((2, batch, W, n), dtype=np.uint64)
        top = self.logq - 1 - 64 * (W - 1)
        cts[:, :, : W - 1] = self.rng.integers(0, 1 << 63, size=(2, batch, W - 1, n), dtype=np.uint64) * np.uint64(2)
        cts[:, :, W - 1] = self.rng.integers(-(1 << top), 1 << top, size=(2, batch, n), dtype=np.int64).view(np.uint64)
        return to_device(cts[0].reshape(-1)), to_device(cts[1].reshape(-1))

    def k0(self, only=None):
        return [k[0] if k is not None and (only is None or r in only) else None for r, k in enumerate(self.keys)]

    def k1(self, only=None):
        return [k[1] if k is not None and (only is None or r in only) else None for r, k in enumerate(self.keys)]

    def planned(self, plan, c0, c1):
        out0, out1 = torch.empty_like(c0), torch.empty_like(c1)
        self.g.he_gemv_planned(out0, out1, c0, c1, plan, self.k0(), self.k1(), self.W, LOGDELTA, self.dimB, self.dimP)
        return out0, out1

    def multi(self, ms, c0, c1, only=None):
        outs0 = [torch.full_like(c0, -1) for _ in range(ms.count)]
        outs1 = [torch.full_like(c1, -1) for _ in range(ms.count)]
        self.g.he_gemv_multi(outs0, outs1, c0, c1, ms, self.k0(only), self.k1(only), self.W, LOGDELTA, self.dimB, self.dimP)
        return outs0, outs1


def same(a, b, what=""):
    torch.cuda.synchronize()
    for name, x, y in (("c0", a[0], b[0]), ("c1", a[1], b[1])):
        bad = torch.nonzero(x != y).flatten()
        assert bad.numel() == 0, "%s %s: %d words differ, first at %s" % (what, name, bad.numel(), bad[:4].tolist())


def counts(g, fn):
    torch.cuda.synchronize()
    g.profile(True)
    try:
        fn()
        return {k: v[1] for k, v in g.profile_collect().items()}
    finally:
        g.profile(False)
