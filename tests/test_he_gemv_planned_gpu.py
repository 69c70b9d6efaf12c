"""gpq_he_gemv_planned: he_gemv (src/he-algo.c:47-93) + he_rs for a fixed matrix held by a gpq_gemv_plan.

* against the reference's loop restated with oracle/bigint_ref, for the shapes tests/test_he_gemv_gpu.py runs gpq_he_gemv at;
* word for word against gpq_he_gemv at the reference's default shape (logn 14, q = 2^438, slots 16) and at logn 16, q = 2^850, slots 64, over
  several launch groups, at non-square slots, for one plan applied to several batches and across streams;
* sparse matrices: what is zero is neither rotated nor multiplied, and needs no key;
* launch counts: the product stage transforms once per call, sums in the NTT domain, reconstructs once per giant step and polynomial;
* bad arguments are refused before anything is launched."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import big_to_ints, gemv_steps, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref

pytestmark = pytest.mark.gpu
LOGDELTA = 30


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
def test_planned_gemv_matches_reference_loop(engine_ctx, oracle_ctx, logn, slots, batch, sparse):
    logq = 120
    dimP, _, dimB, dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
    dimpt = _dimpt(logq, logn)
    g, o = engine_ctx(logn, max(dimevk, dimpt + 1)), oracle_ctx(logn, max(dimevk, dimpt + 1))
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
    with g.gemv_plan(dg, slots, W, logq, dimpt) as plan:
        assert plan.exact
        g.he_gemv_planned(out0, out1, c0, c1, plan, [k[0] for k in dk], [k[1] for k in dk], W, LOGDELTA, dimB, dimP)
        torch.cuda.synchronize()
    got0, got1 = big_to_ints(to_host(out0), W, n), big_to_ints(to_host(out1), W, n)
    for k in range(batch):
        e0, e1 = _ref_gemv(o, cts[k], diags, hkeys, slots, dimP, dimB, dimpt, logq)
        assert got0[k] == e0, "ciphertext %d: c0" % k
        assert got1[k] == e1, "ciphertext %d: c1" % k


class Shape:
    """random ciphertexts, 30-bit diagonals and keys for the rotations he_gemv needs, all made on the host with numpy"""

    def __init__(self, engine_ctx, logn, logq, slots, batch, seed=None, zero_diags=()):
        self.logn, self.logq, self.slots, self.batch = logn, logq, slots, batch
        self.n, self.W = 1 << logn, logq // 64 + 1
        self.dimP, _, self.dimB, _ = engine_ctx(logn, 20).he_dims(logq, logq)
        self.dimpt = _dimpt(logq, logn)
        self.g = engine_ctx(logn, max(self.dimB, self.dimpt))
        self.rng = np.random.default_rng(logn if seed is None else seed)
        self.n1, self.n2 = gemv_steps(slots)
        dg = np.zeros((slots, self.W, self.n), dtype=np.uint64)
        dg[:, 0] = self.rng.integers(-(1 << 62), 1 << 62, size=(slots, self.n), dtype=np.int64).view(np.uint64) >> np.uint64(64 - LOGDELTA)   # small positive
        for k in zero_diags:
            dg[k] = 0
        self.diag = to_device(dg.reshape(-1))
        p = self.g.p
        self.keys = [None] * slots
        for r in sorted(set(range(self.n1)) | {i * self.n1 for i in range(self.n2)}):
            self.keys[r] = tuple(to_device(np.concatenate([self.rng.integers(0, p[d], size=self.n, dtype=np.uint64) for d in range(self.dimB)])) for _ in range(2))

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

    def plan(self):
        return self.g.gemv_plan(self.diag, self.slots, self.W, self.logq, self.dimpt)

    def baseline(self, c0, c1):
        out0, out1 = torch.empty_like(c0), torch.empty_like(c1)
        self.g.he_gemv(out0, out1, c0, c1, self.diag, self.k0(), self.k1(), self.slots, self.W, self.logq, LOGDELTA, self.dimB, self.dimP, self.dimpt)
        return out0, out1

    def planned(self, plan, c0, c1, only=None):
        out0, out1 = torch.empty_like(c0), torch.empty_like(c1)
        self.g.he_gemv_planned(out0, out1, c0, c1, plan, self.k0(only), self.k1(only), self.W, LOGDELTA, self.dimB, self.dimP)
        return out0, out1


def _same(a, b, what=""):
    torch.cuda.synchronize()
    for name, x, y in (("c0", a[0], b[0]), ("c1", a[1], b[1])):
        bad = torch.nonzero(x != y).flatten()
        assert bad.numel() == 0, "%s %s: %d words differ, first at %s" % (what, name, bad.numel(), bad[:4].tolist())


@pytest.mark.timeout(900)
@pytest.mark.parametrize("logn,logq,slots", [(14, 438, 16), (16, 850, 64)])
def test_planned_equals_gemv_at_reference_shapes(engine_ctx, logn, logq, slots):
    sh = Shape(engine_ctx, logn, logq, slots, 2)
    c0, c1 = sh.ciphertexts()
    with sh.plan() as plan:
        assert plan.exact and plan.live == slots and plan.dim == sh.dimpt and plan.bytes == slots * plan.dim * sh.n * 8
        got = sh.planned(plan, c0, c1)
        _same(got, sh.baseline(c0, c1))
    assert len(set(to_host(got[0][: sh.n]).tolist())) > sh.n // 2        # not degenerate


@pytest.mark.parametrize("slots", [8, 32])
def test_several_launch_groups_and_non_square_slots(engine_ctx, slots):
    sh = Shape(engine_ctx, 13, 120, slots, 5)
    c0, c1 = sh.ciphertexts()
    expect = sh.baseline(c0, c1)
    try:
        sh.g.set_chunk(2)                                    # three launch groups, the last one odd
        with sh.plan() as plan:
            got = sh.planned(plan, c0, c1)
            _same(got, expect)
    finally:
        sh.g.set_chunk(32)


def test_one_plan_many_batches_and_streams(engine_ctx):
    sh = Shape(engine_ctx, 13, 120, 16, 3)
    g = sh.g
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan = sh.plan()                                     # queued on `side`
    main = torch.cuda.current_stream()
    assert g.lib.gpq_stream_wait(C.c_void_p(main.cuda_stream), C.c_void_p(side.cuda_stream)) == 0
    try:
        for batch in (3, 1, 2):
            c0, c1 = sh.ciphertexts(batch)
            _same(sh.planned(plan, c0, c1), sh.baseline(c0, c1), "batch %d" % batch)
    finally:
        plan.close()


def _counts(g, fn):
    torch.cuda.synchronize()
    g.profile(True)
    try:
        fn()
        return {k: v[1] for k, v in g.profile_collect().items()}
    finally:
        g.profile(False)


def test_he_idx_shaped_matrix_needs_one_key(engine_ctx):
    """only diagonal 0 is live (he_idx, src/he-algo.c:127-140): one baby rotation and one giant rotation, both by 0 with rk[0]"""
    slots = 16
    sh = Shape(engine_ctx, 13, 120, slots, 2, zero_diags=range(1, slots))
    c0, c1 = sh.ciphertexts()
    g = sh.g
    o0, o1 = torch.empty_like(c0), torch.empty_like(c1)
    swk = _counts(g, lambda: g.he_swk(o0, o1, c0, c1, sh.keys[0][0], sh.keys[0][1], sh.W, sh.logq, sh.dimB, sh.dimP))
    with sh.plan() as plan:
        assert plan.exact and plan.live == 1
        got = []
        cnt = _counts(g, lambda: got.append(sh.planned(plan, c0, c1, only={0})))
        _same(got[0], sh.baseline(c0, c1))
    assert cnt["keyswitch_mid"] == 2 * swk["keyswitch_mid"] and cnt.get("keyswitch_rot_mid", 0) == 0, (swk, cnt)
    assert cnt["gemv_mac"] == 1, cnt


def test_zero_giant_steps_are_skipped(engine_ctx):
    slots = 16
    n1, n2 = gemv_steps(slots)
    zero = [i * n1 + j for i in (1, 3) for j in range(n1)] + [2 * n1 + 2, 2]       # ... and baby rotation 2 is live in no giant step
    sh = Shape(engine_ctx, 13, 120, slots, 2, zero_diags=zero)
    c0, c1 = sh.ciphertexts()
    with sh.plan() as plan:
        assert plan.exact and plan.live == slots - len(zero)
        got = []
        cnt = _counts(sh.g, lambda: got.append(sh.planned(plan, c0, c1, only={0, 1, 3, 2 * n1})))
        _same(got[0], sh.baseline(c0, c1))
    assert cnt["gemv_mac"] == 2, cnt


def test_zero_matrix_needs_no_key(engine_ctx):
    """every diagonal zero: no rotation at all, the outputs are overwritten with what gpq_he_gemv computes from the same zero diagonals"""
    slots = 4
    sh = Shape(engine_ctx, 10, 120, slots, 3, zero_diags=range(slots))
    c0, c1 = sh.ciphertexts()
    expect = sh.baseline(c0, c1)
    out0, out1 = torch.full_like(c0, 0x5A5A5A5A5A5A5A5A), torch.full_like(c1, -3)
    try:
        sh.g.set_chunk(2)                                    # two launch groups, the last one odd
        with sh.plan() as plan:
            assert plan.exact and plan.live == 0 and not any(plan.rotations())
            sh.g.he_gemv_planned(out0, out1, c0, c1, plan, [None] * slots, [None] * slots, sh.W, LOGDELTA, sh.dimB, sh.dimP)
            _same((out0, out1), expect)
    finally:
        sh.g.set_chunk(32)


def test_launch_counts_of_the_product_stage(engine_ctx):
    logn, logq, slots, batch = 14, 438, 16, 2
    sh = Shape(engine_ctx, logn, logq, slots, batch)
    g, n1, n2 = sh.g, sh.n1, sh.n2
    c0, c1 = sh.ciphertexts()
    o0, o1 = torch.empty_like(c0), torch.empty_like(c1)
    r0 = torch.empty(n1 * c0.numel(), dtype=torch.int64, device="cuda")
    r1 = torch.empty_like(r0)
    with sh.plan() as plan:
        slab = torch.zeros(plan.dim * sh.n, dtype=torch.int64, device="cuda")
        # the parts of the call that are not the product stage, each on its own
        swk = _counts(g, lambda: g.he_swk(o0, o1, c0, c1, sh.keys[0][0], sh.keys[0][1], sh.W, logq, sh.dimB, sh.dimP))
        baby = _counts(g, lambda: g.he_rot_hoisted(r0, r1, c0, c1, list(range(n1)), sh.k0()[:n1], sh.k1()[:n1], sh.W, logq, sh.dimB, sh.dimP))
        fwd = _counts(g, lambda: g.poly_ntt(slab, plan.dim))             # one forward transform over the plan's limbs: launches per limb class
        planned = _counts(g, lambda: sh.planned(plan, c0, c1))
        loop = _counts(g, lambda: sh.baseline(c0, c1))
        get = lambda d, k: d.get(k, 0)
        rest = lambda k: get(baby, k) + n2 * get(swk, k)
        # forward transforms of the product stage: once per call, not once per giant step
        for k in ("strided_fwd", "contig_fwd"):
            assert get(planned, k) - rest(k) == get(fwd, k) > 0, (k, planned, baby, swk, fwd)
            assert get(loop, k) - rest(k) >= n2 * get(fwd, k), (k, loop)             # (gpq_he_gemv: mulpt_mid8 counts as contig_fwd)
        assert get(planned, "gemv_mac") == n2 and get(loop, "gemv_mac") == 0
        assert get(planned, "bridge_reconstruct") - rest("bridge_reconstruct") == 2 * n2, (planned, baby, swk)
        assert get(planned, "bridge_decompose") - rest("bridge_decompose") == 2, (planned, baby, swk)
        assert get(planned, "strided_inv") - rest("strided_inv") == n2 * get(fwd, "strided_fwd"), (planned, baby, swk)
        try:
            g.set_chunk(1)                                   # two launch groups
            assert _counts(g, lambda: sh.planned(plan, c0, c1))["gemv_mac"] == 2 * n2
        finally:
            g.set_chunk(32)


def test_bad_arguments_launch_nothing(engine_ctx):
    sh = Shape(engine_ctx, 10, 120, 4, 1)
    g, lib = sh.g, sh.g.lib
    other = engine_ctx(10, max(sh.dimB, sh.dimpt) + 1)
    c0, c1 = sh.ciphertexts()
    out0, out1 = torch.zeros_like(c0), torch.zeros_like(c1)
    P = lambda t: C.c_void_p(t.data_ptr())
    with sh.plan() as plan, other.gemv_plan(sh.diag, sh.slots, sh.W, sh.logq, sh.dimpt) as foreign:
        ws = torch.zeros(lib.gpq_he_gemv_planned_workspace_bytes(g.h, plan.h, sh.W, sh.dimB, sh.dimP, 1) // 8 + 8, dtype=torch.int64, device="cuda")

        def call(o0=out0, src=c0, k0=None, pl=plan, W=sh.W):
            k0 = sh.k0() if k0 is None else k0
            return lib.gpq_he_gemv_planned(g.h, P(o0), P(out1), P(src), P(c1), pl.h, g._key_ptrs(k0), g._key_ptrs(sh.k1()), W, LOGDELTA, sh.dimB, sh.dimP, 1,
                                           P(ws), g._stream())

        assert call() == 0
        torch.cuda.synchronize()
        good = out0.clone()
        out0.zero_()
        g.profile(True)
        try:
            assert call(o0=c0) == -1 and b"alias" in lib.gpq_last_error()
            assert call(o0=out1) == -1 and b"alias" in lib.gpq_last_error()
            missing = sh.k0()
            missing[2] = None                                # giant rotation 1 * n1
            assert call(k0=missing) == -1 and b"NULL" in lib.gpq_last_error()
            assert call(pl=foreign) == -1 and b"another context" in lib.gpq_last_error()
            assert call(W=1) == -1
            assert g.profile_collect() == {}
        finally:
            g.profile(False)
        torch.cuda.synchronize()
        assert not out0.any() and good.any()
