"""gpq_he_rot_hoisted: he_rot (src/he-automorphism.c:101-115) of one batch by several amounts with c1 decomposed and transformed once.

* against oracle/bigint_ref (poly_rot + he_swk restated) on single-pass (logn 7, 10, 12) and two-pass (13, 14) rings;
* word for word against gpq_poly_rot x 2 + gpq_he_swk on the device at n = 2^16 / q_l = 2^850 and n = 2^17 / 44 limbs, over several
  launch groups, both cache policies;
* the launch counts that make it a hoist: decompose and forward strided pass once per launch group, the permuted mid kernel per rotation;
* argument checks."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import big_to_ints, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref

pytestmark = pytest.mark.gpu


def _centred(rng, logq, n):
    h = 1 << (logq - 1)
    vals = [rng.randrange(-h, h) for _ in range(n)]
    vals[:4] = [0, -1, h - 1, -h]
    return vals


def _dense(rng, W, n, logq):
    """dense centred words: uniform in [-q/2, q/2)"""
    w = rng.integers(0, 1 << 63, size=(W, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(W, n), dtype=np.uint64)
    top = logq - 1 - 64 * (W - 1)
    w[W - 1] = rng.integers(-(1 << top), 1 << top, size=n, dtype=np.int64).view(np.uint64)
    return w.reshape(-1)


def _composed(g, c0, c1, rots, keys, W, logq, dimB, dimP):
    """the reference's spelling on the device: poly_rot of both polynomials, then he_swk with the rotation's key; rotation-major"""
    outs0, outs1 = [], []
    for r, rot in enumerate(rots):
        d0, d1 = torch.empty_like(c0), torch.empty_like(c1)
        g.poly_rot(d0, c0, W, rot)
        g.poly_rot(d1, c1, W, rot)
        o0, o1 = torch.empty_like(c0), torch.empty_like(c1)
        g.he_swk(o0, o1, d0, d1, keys[r][0], keys[r][1], W, logq, dimB, dimP)
        outs0.append(o0)
        outs1.append(o1)
    return torch.cat(outs0), torch.cat(outs1)


ROTSETS = {1: [40], 3: [0, 3, 3], 16: [0, 1, 2, 3, 40, 5, 6, 7, 7, 9, 10, 11, 12, 13, 14, 1000]}


@pytest.mark.parametrize("logn", [7, 10, 12, 13, 14])
@pytest.mark.parametrize("nrot,batch", [(1, 3), (3, 1), (16, 3)])
def test_hoisted_matches_reference(engine_ctx, oracle_ctx, logn, nrot, batch):
    logq = 120
    dimP, _, dimB, dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    n, W = g.n, (logq + 63) // 64
    rng = random.Random(logn * 100 + nrot)
    rots = ROTSETS[nrot]
    hkeys = {rot: (o.gen(6000 + 2 * rot, dimevk)[: dimB * n], o.gen(6001 + 2 * rot, dimevk)[: dimB * n]) for rot in set(rots)}
    dkeys = {rot: (to_device(a), to_device(b)) for rot, (a, b) in hkeys.items()}
    keys = [dkeys[r] for r in rots]
    cts = [(_centred(rng, logq, n), _centred(rng, logq, n)) for _ in range(batch)]
    c0 = to_device(np.concatenate([ints_to_big(ct[0], W) for ct in cts]))
    c1 = to_device(np.concatenate([ints_to_big(ct[1], W) for ct in cts]))
    out0 = torch.empty(nrot * c0.numel(), dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    g.he_rot_hoisted(out0, out1, c0, c1, rots, [k[0] for k in keys], [k[1] for k in keys], W, logq, dimB, dimP)
    e0, e1 = _composed(g, c0, c1, rots, keys, W, logq, dimB, dimP)
    assert torch.equal(out0, e0) and torch.equal(out1, e1), "hoisted and poly_rot + he_swk differ"
    got0, got1 = big_to_ints(to_host(out0), W, n), big_to_ints(to_host(out1), W, n)
    # the restated reference on a few (rotation, ciphertext) pairs: the first and last of each, and the duplicate / large rotations
    picks = sorted({0, nrot - 1} | {r for r, rot in enumerate(rots) if rot in (40, 1000) or rots.count(rot) > 1})
    ks = sorted({0, batch - 1})
    if logn >= 13:                                   # (the restatement's CRT is pure Python)
        picks, ks = picks[:2], ks[-1:]
    for r in picks:
        for k in ks:
            d0, d1 = ref.poly_rot(cts[k][0], rots[r]), ref.poly_rot(cts[k][1], rots[r])
            x0, x1 = ref.he_swk(o, d0, d1, *hkeys[rots[r]], dimP, dimB, logq)
            assert got0[r * batch + k] == x0, "rotation %d (rot %d), ciphertext %d: c0" % (r, rots[r], k)
            assert got1[r * batch + k] == x1, "rotation %d (rot %d), ciphertext %d: c1" % (r, rots[r], k)


@pytest.mark.parametrize("logn,logq,limbs", [(16, 850, 45), (17, 835, 44)])
@pytest.mark.parametrize("nt,classes", [(0, None), (1, None), (-1, (0, 0)), (-1, (0, 64))])
def test_hoisted_equals_device_composition_at_full_size(engine_ctx, logn, logq, limbs, nt, classes):
    """classes: gpq_set_limb_classes on a context of its own -- (0, 0) runs the 7-mad instantiations on every limb, (0, all) the split-twiddle
    ones (no wide-split limbs), so that keyswitch_rot_mid8x2 and the hoisted forward transform run in every butterfly class"""
    import gpqhe_amd
    n, W = 1 << logn, logq // 64 + 1
    dimP, _, dimB, dimevk = engine_ctx(logn, 20).he_dims(logq, logq)
    assert dimB == limbs
    g = engine_ctx(logn, dimB) if classes is None else gpqhe_amd.PolyContext(logn, dimB)
    if classes is not None:
        g.set_limb_classes(*classes)
    rng = np.random.default_rng(logn + nt)
    batch, rots = 5, [0, 5, 40, 5]
    c0 = to_device(np.concatenate([_dense(rng, W, n, logq) for _ in range(batch)]))
    c1 = to_device(np.concatenate([_dense(rng, W, n, logq) for _ in range(batch)]))
    p = g.p
    kk = {rot: tuple(to_device(np.concatenate([rng.integers(0, p[d], size=n, dtype=np.uint64) for d in range(dimB)])) for _ in range(2)) for rot in set(rots)}
    keys = [kk[r] for r in rots]
    out0 = torch.empty(len(rots) * c0.numel(), dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    try:
        g.set_chunk(2)                                   # three launch groups, the last one odd
        g.set_nt_policy(nt)
        g.he_rot_hoisted(out0, out1, c0, c1, rots, [k[0] for k in keys], [k[1] for k in keys], W, logq, dimB, dimP)
        e0, e1 = _composed(g, c0, c1, rots, keys, W, logq, dimB, dimP)
        torch.cuda.synchronize()
    finally:
        g.set_chunk(32)
        g.set_nt_policy(-1)
        if classes is not None:
            torch.cuda.synchronize()
            g.close()
    for name, a, b in (("c0", out0, e0), ("c1", out1, e1)):
        bad = torch.nonzero(a != b).flatten()
        assert bad.numel() == 0, "%s: %d words differ, first at %s" % (name, bad.numel(), bad[:4].tolist())
    assert len(set(to_host(out0[:n]).tolist())) > n // 2        # not degenerate


@pytest.mark.parametrize("logn", [10, 13])
def test_device_permutation_is_the_host_index_table(engine_ctx, oracle_ctx, logn):
    """The kernels compute sigma on the fly; here the expectation is built from gpq_automorphism_index itself: the oracle's transform of
    the UNROTATED decomposed c1, permuted by the host table, times the key, inverse transform, the reference's tail with poly_rot(c0)."""
    import gpqhe_amd
    logq = 120
    dimP, _, dimB, dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    n, W = g.n, (logq + 63) // 64
    rng = random.Random(logn)
    c0i, c1i = _centred(rng, logq, n), _centred(rng, logq, n)
    rots = [3, 40, 1000]
    hk = [(o.gen(9000 + 2 * r, dimB), o.gen(9001 + 2 * r, dimB)) for r in rots]
    out0 = torch.empty(len(rots) * W * n, dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    g.he_rot_hoisted(out0, out1, to_device(ints_to_big(c0i, W)), to_device(ints_to_big(c1i, W)), rots, [to_device(k[0]) for k in hk],
                     [to_device(k[1]) for k in hk], W, logq, dimB, dimP)
    got0, got1 = big_to_ints(to_host(out0), W, n), big_to_ints(to_host(out1), W, n)
    X = o.ntt_slab(ref._slab(o, c1i, dimB), dimB)
    for r, rot in enumerate(rots):
        sigma = gpqhe_amd.automorphism_index(logn, pow(5, rot, 1 << 64) % (2 * n)).astype(np.int64)
        hats = []
        for key in hk[r]:
            prod = np.concatenate([o.rns_mul(X[d * n:(d + 1) * n][sigma], key[d * n:(d + 1) * n], d) for d in range(dimB)])
            hats.append(o.ntt_slab(prod, dimB, inverse=True))
        e0, e1 = ref.he_relin_tail(o, hats[0], hats[1], ref.poly_rot(c0i, rot), None, dimP, dimB, 1 << logq)
        assert got0[r] == e0 and got1[r] == e1, "rotation %d" % rot


def test_hoist_runs_the_shared_work_once_per_launch_group(engine_ctx, oracle_ctx):
    logn, logq = 14, 438
    dimP, _, dimB, dimevk = engine_ctx(logn, 20).he_dims(logq, logq)
    g, o = engine_ctx(logn, dimB), oracle_ctx(logn, dimB)
    n, W, batch = g.n, logq // 64 + 1, 3
    rng = np.random.default_rng(5)
    c0 = to_device(np.concatenate([_dense(rng, W, n, logq) for _ in range(batch)]))
    c1 = to_device(np.concatenate([_dense(rng, W, n, logq) for _ in range(batch)]))
    k0, k1 = to_device(o.gen(7000, dimB)), to_device(o.gen(7001, dimB))
    rots = [1, 2, 3, 4, 5, 6, 7, 8]
    out0 = torch.empty(len(rots) * c0.numel(), dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    try:
        g.set_chunk(2)                                   # two launch groups
        torch.cuda.synchronize()
        g.profile(True)
        g.he_swk(out0[: c0.numel()], out1[: c0.numel()], c0, c1, k0, k1, W, logq, dimB, dimP)
        one = g.profile_collect()
        g.he_rot_hoisted(out0, out1, c0, c1, rots, [k0] * 8, [k1] * 8, W, logq, dimB, dimP)
        hoisted = g.profile_collect()
    finally:
        g.profile(False)
        g.set_chunk(32)
    cnt = lambda prof, k: prof.get(k, (0, 0))[1]
    assert cnt(one, "bridge_decompose") > 0 and cnt(one, "strided_fwd") > 0 and cnt(one, "keyswitch_mid") > 0
    assert cnt(hoisted, "bridge_decompose") == cnt(one, "bridge_decompose"), (one, hoisted)
    assert cnt(hoisted, "strided_fwd") == cnt(one, "strided_fwd"), (one, hoisted)
    assert cnt(hoisted, "keyswitch_rot_mid") == 8 * cnt(one, "keyswitch_mid"), (one, hoisted)
    assert cnt(hoisted, "strided_inv") == 8 * cnt(one, "strided_inv"), (one, hoisted)
    assert cnt(hoisted, "keyswitch_mid") == 0


def test_bad_arguments_are_rejected(engine_ctx):
    logn, logq = 10, 120
    dimP, _, dimB, dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
    g = engine_ctx(logn, dimevk)
    lib, n, W = g.lib, g.n, (logq + 63) // 64
    c = torch.zeros(W * n, dtype=torch.int64, device="cuda")
    out0 = torch.zeros(3 * W * n, dtype=torch.int64, device="cuda")       # rotation-major: 3 rotations x batch 1, each
    out1 = torch.zeros(3 * W * n, dtype=torch.int64, device="cuda")
    key = torch.zeros(dimB * n, dtype=torch.int64, device="cuda")
    ws = torch.zeros(lib.gpq_he_rot_hoisted_workspace_bytes(g.h, W, dimB, dimP, 3, 1) // 8 + 8, dtype=torch.int64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    rots = (C.c_uint * 3)(0, 1, 2)

    def call(nrot=3, keys0=None, Wc=W, o0=None, src=None):
        k0 = keys0 if keys0 is not None else (C.c_void_p * 3)(*[key.data_ptr()] * 3)
        k1 = (C.c_void_p * 3)(*[key.data_ptr()] * 3)
        return lib.gpq_he_rot_hoisted(g.h, P(out0 if o0 is None else o0), P(out1), P(c if src is None else src), P(c), rots, k0, k1, nrot, Wc, logq,
                                      dimB, dimP, 1, P(ws), None)

    assert call() == 0
    torch.cuda.synchronize()
    assert call(nrot=0) == -1
    assert call(keys0=(C.c_void_p * 3)(key.data_ptr(), None, key.data_ptr())) == -1
    assert b"NULL" in lib.gpq_last_error()
    assert call(Wc=1) == -1
    assert call(src=out0[W * n:]) == -1               # an input inside an output range (rotation 1 would read what rotation 0 wrote)
    assert b"alias" in lib.gpq_last_error()
    assert call(o0=out1) == -1                        # the two outputs overlapping
    assert lib.gpq_he_rot_hoisted_workspace_bytes(g.h, W, dimB, dimP, 0, 1) == 0
