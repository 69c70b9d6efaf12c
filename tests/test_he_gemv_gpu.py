"""gpq_he_gemv: he_gemv (src/he-algo.c:47-93) followed by he_rs, on big slabs.

* against the reference's loop restated with oracle/bigint_ref (he_swk o poly_rot, he_mulpt, he_add, then mpi_rdiv + mpi_smod), for
  slots 1 .. 16 at logn 10 - 12, dense diagonals and he_ecd-shaped sparse ones, batch 1 and 2;
* word for word against the same loop spelled with the slab entry points (gpq_poly_rot, gpq_he_swk, gpq_he_mulpt, gpq_big_add, gpq_he_rs)
  at the reference's default shape (logn 14, q = 2^438, slots 16) and at logn 16, q = 2^850, slots 64."""
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import big_to_ints, gemv_steps, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref

pytestmark = pytest.mark.gpu
LOGDELTA = 30


def test_baby_and_giant_steps_follow_the_reference():
    assert [gemv_steps(s) for s in (1, 2, 4, 8, 16, 32, 64)] == [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]


def _diag(rng, n, slots, sparse, bits):
    if sparse:                                   # what he_ecd makes of a slot vector: 2 slots non-zero terms at stride n / (2 slots)
        v = [0] * n
        for t in range(2 * slots):
            v[t * (n // (2 * slots))] = rng.randrange(-(1 << bits), 1 << bits)
        return v
    return [rng.randrange(-(1 << bits), 1 << bits) for _ in range(n)]


def _dimpt(logql, logn):
    return (logql + 1 + LOGDELTA + logn) // 59 + 1           # src/he-mult.c:168 with nu = 2^LOGDELTA


def _ref_gemv(o, ct, diags, keys, slots, dimP, dimB, dimpt, logql):
    """the loop itself lives in oracle/bigint_ref.py, where tests/test_ref_functions.py pins it to the executed reference's he_gemv"""
    assert ref.gemv_steps(slots) == gemv_steps(slots)
    return ref.ref_gemv(o, ct, diags, keys, slots, dimP, dimB, dimpt, logql, LOGDELTA)


@pytest.mark.parametrize("logn,slots,batch,sparse", [(10, 1, 2, True), (10, 2, 1, False), (12, 4, 1, True), (10, 8, 2, False),
                                                     (11, 16, 1, False), (10, 16, 2, True)])
def test_gemv_matches_reference_loop(engine_ctx, oracle_ctx, logn, slots, batch, sparse):
    logq = 120
    dimP, _, dimB, dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
    dimpt = _dimpt(logq, logn)
    g, o = engine_ctx(logn, max(dimevk, dimpt)), oracle_ctx(logn, max(dimevk, dimpt))
    n, W = g.n, (logq + 63) // 64
    rng = random.Random(logn * 1000 + slots * 10 + batch)
    h = 1 << (logq - 1)
    cts = [([rng.randrange(-h, h) for _ in range(n)], [rng.randrange(-h, h) for _ in range(n)]) for _ in range(batch)]
    diags = [_diag(rng, n, slots, sparse, LOGDELTA) for _ in range(slots)]
    hkeys = [(o.gen(8000 + 2 * r, dimB), o.gen(8001 + 2 * r, dimB)) for r in range(slots)]
    dk = [(to_device(a), to_device(b)) for a, b in hkeys]
    c0 = to_device(np.concatenate([ints_to_big(ct[0], W) for ct in cts]))
    c1 = to_device(np.concatenate([ints_to_big(ct[1], W) for ct in cts]))
    dg = to_device(np.concatenate([ints_to_big(d, W) for d in diags]))
    out0, out1 = torch.empty_like(c0), torch.empty_like(c1)
    g.he_gemv(out0, out1, c0, c1, dg, [k[0] for k in dk], [k[1] for k in dk], slots, W, logq, LOGDELTA, dimB, dimP, dimpt)
    got0, got1 = big_to_ints(to_host(out0), W, n), big_to_ints(to_host(out1), W, n)
    for k in range(batch):
        e0, e1 = _ref_gemv(o, cts[k], diags, hkeys, slots, dimP, dimB, dimpt, logq)
        assert got0[k] == e0, "ciphertext %d: c0" % k
        assert got1[k] == e1, "ciphertext %d: c1" % k


def _slab_loop(g, c0, c1, diags, keys, slots, W, logql, dimB, dimP, dimpt):
    """src/he-algo.c:47-93 spelled with the per-call slab entry points, then he_rs"""
    n1, n2 = gemv_steps(slots)
    lib, s = g.lib, g._stream()
    bigs = c0.numel()
    batch = bigs // (W * g.n)
    P = g._ptr

    def rot(a0, a1, r):
        d0, d1 = torch.empty_like(a0), torch.empty_like(a1)
        g.poly_rot(d0, a0, W, r)
        g.poly_rot(d1, a1, W, r)
        o0, o1 = torch.empty_like(a0), torch.empty_like(a1)
        g.he_swk(o0, o1, d0, d1, keys[r][0], keys[r][1], W, logql, dimB, dimP)
        return o0, o1

    def add(acc, x):
        for a, b in zip(acc, x):
            assert lib.gpq_big_add(g.h, P(a), P(a), P(b), W, logql, batch, s) == 0

    outer = None
    for i in range(n2):
        inner = None
        for j in range(n1):
            r0, r1 = rot(c0, c1, j)
            m = diags[(i * n1 + j) * W * g.n:(i * n1 + j + 1) * W * g.n].repeat(batch)
            p0, p1 = torch.empty_like(r0), torch.empty_like(r1)
            g.he_mulpt(p0, p1, r0, r1, m, W, logql, dimpt)
            if inner is None:
                inner = (p0, p1)
            else:
                add(inner, (p0, p1))
        gi = rot(inner[0], inner[1], i * n1)
        if outer is None:
            outer = gi
        else:
            add(outer, gi)
    g.he_rs(outer[0], outer[1], W, LOGDELTA, logql - LOGDELTA)
    return outer


@pytest.mark.timeout(900)
@pytest.mark.parametrize("logn,logq,slots", [(14, 438, 16), (16, 850, 64)])
def test_gemv_equals_slab_loop_at_reference_shapes(engine_ctx, logn, logq, slots):
    n, W = 1 << logn, logq // 64 + 1
    dimP, _, dimB, dimevk = engine_ctx(logn, 20).he_dims(logq, logq)
    dimpt = _dimpt(logq, logn)
    g = engine_ctx(logn, max(dimB, dimpt))
    rng = np.random.default_rng(logn)
    h = 1 << 62
    words = lambda count: np.zeros((count, W, n), dtype=np.uint64)   # big slabs of zeros
    cts = words(2)
    top = logq - 1 - 64 * (W - 1)
    cts[:, : W - 1] = rng.integers(0, 1 << 63, size=(2, W - 1, n), dtype=np.uint64) * np.uint64(2)
    cts[:, W - 1] = rng.integers(-(1 << top), 1 << top, size=(2, n), dtype=np.int64).view(np.uint64)
    c0, c1 = to_device(cts[0].reshape(-1)), to_device(cts[1].reshape(-1))
    dg = words(slots)
    dg[:, 0] = rng.integers(-h, h, size=(slots, n), dtype=np.int64).view(np.uint64) >> np.uint64(64 - LOGDELTA)   # small positive
    dg = to_device(dg.reshape(-1))
    n1, n2 = gemv_steps(slots)
    p = g.p
    keys = [None] * slots
    for r in sorted(set(range(n1)) | {i * n1 for i in range(n2)}):
        keys[r] = tuple(to_device(np.concatenate([rng.integers(0, p[d], size=n, dtype=np.uint64) for d in range(dimB)])) for _ in range(2))
    out0, out1 = torch.empty_like(c0), torch.empty_like(c1)
    g.he_gemv(out0, out1, c0, c1, dg, [k and k[0] for k in keys], [k and k[1] for k in keys], slots, W, logq, LOGDELTA, dimB, dimP, dimpt)
    e0, e1 = _slab_loop(g, c0, c1, dg, keys, slots, W, logq, dimB, dimP, dimpt)
    torch.cuda.synchronize()
    for name, a, b in (("c0", out0, e0), ("c1", out1, e1)):
        bad = torch.nonzero(a != b).flatten()
        assert bad.numel() == 0, "%s: %d words differ, first at %s" % (name, bad.numel(), bad[:4].tolist())
    assert len(set(to_host(out0[:n]).tolist())) > n // 2
