"""gpq_he_gemv_multi: several gpq_gemv_plans applied to the same ciphertexts with the baby rotations, their transforms and the reads of those
transforms shared.  Output t must be, word for word, what gpq_he_gemv_planned writes for plans[t]:

* against k planned calls, on two-pass and single-pass rings, over two launch groups, for 1, 2, NP and NP + 1 plans;
* against the reference's loop restated with oracle/bigint_ref;
* plans with different live sets (the union of the rotations, keys outside it absent, the zero matrix) and with different dims;
* launch counts: the shared stage runs once, the inner sums in ceil(k / NP) launches per giant step;
* bad arguments are refused before anything is launched."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import _native, big_to_ints, gemv_multi_width, gemv_steps, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref
from tests.gemv_multi_shapes import LOGDELTA, MultiShape, counts, dimpt_of, same

pytestmark = pytest.mark.gpu
NP = gemv_multi_width()


def _plans(sh, k, **kw):
    return [sh.plan(sh.diagonals(**kw)) for _ in range(k)]


def _close(plans):
    for p in plans:
        p.close()


@pytest.mark.parametrize("k", sorted({1, 2, NP, NP + 1}))
@pytest.mark.parametrize("logn,slots", [(13, 8), (13, 16), (10, 4)])
def test_multi_equals_k_planned_calls(engine_ctx, logn, slots, k):
    sh = MultiShape(engine_ctx, logn, 120, slots, 3)
    c0, c1 = sh.ciphertexts()
    plans = _plans(sh, k)
    try:
        assert all(p.exact and p.live == slots for p in plans)
        expect = [sh.planned(p, c0, c1) for p in plans]
        try:
            sh.g.set_chunk(2)                                # two launch groups, the last one odd
            with sh.g.gemv_multi(plans) as ms:
                assert ms.count == k and ms.baby == sh.n1 and ms.dim == max(p.dim for p in plans) and ms.bytes > 0
                outs0, outs1 = sh.multi(ms, c0, c1)
                for t in range(k):
                    same((outs0[t], outs1[t]), expect[t], "plan %d of %d" % (t, k))
        finally:
            sh.g.set_chunk(32)
        if k > 1:
            assert not torch.equal(outs0[0], outs0[1])           # the plans are different matrices
    finally:
        _close(plans)


def test_multi_matches_reference_loop(engine_ctx, oracle_ctx):
    logn, logq, slots, batch, k = 10, 120, 4, 2, 2
    dimP, _, dimB, dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
    dimpt = dimpt_of(logq, logn)
    g, o = engine_ctx(logn, max(dimevk, dimpt + 1)), oracle_ctx(logn, max(dimevk, dimpt + 1))
    n, W = g.n, (logq + 63) // 64
    rng = random.Random(4242)
    h = 1 << (logq - 1)
    cts = [([rng.randrange(-h, h) for _ in range(n)], [rng.randrange(-h, h) for _ in range(n)]) for _ in range(batch)]
    diags = [[[rng.randrange(-(1 << LOGDELTA), 1 << LOGDELTA) for _ in range(n)] for _ in range(slots)] for _ in range(k)]
    hkeys = [(o.gen(8000 + 2 * r, dimB), o.gen(8001 + 2 * r, dimB)) for r in range(slots)]
    dk = [(to_device(a), to_device(b)) for a, b in hkeys]
    c0 = to_device(np.concatenate([ints_to_big(ct[0], W) for ct in cts]))
    c1 = to_device(np.concatenate([ints_to_big(ct[1], W) for ct in cts]))
    plans = [g.gemv_plan(to_device(np.concatenate([ints_to_big(d, W) for d in diags[t]])), slots, W, logq, dimpt) for t in range(k)]
    try:
        outs0, outs1 = [torch.empty_like(c0) for _ in range(k)], [torch.empty_like(c1) for _ in range(k)]
        with g.gemv_multi(plans) as ms:
            g.he_gemv_multi(outs0, outs1, c0, c1, ms, [x[0] for x in dk], [x[1] for x in dk], W, LOGDELTA, dimB, dimP)
            torch.cuda.synchronize()
    finally:
        _close(plans)
    assert ref.gemv_steps(slots) == gemv_steps(slots)
    for t in range(k):
        got0, got1 = big_to_ints(to_host(outs0[t]), W, n), big_to_ints(to_host(outs1[t]), W, n)
        for b in range(batch):
            e0, e1 = ref.ref_gemv(o, cts[b], diags[t], hkeys, slots, dimP, dimB, dimpt, logq, LOGDELTA)
            assert got0[b] == e0, "plan %d, ciphertext %d: c0" % (t, b)
            assert got1[b] == e1, "plan %d, ciphertext %d: c1" % (t, b)


def test_different_live_sets_in_one_set(engine_ctx):
    slots = 16
    sh = MultiShape(engine_ctx, 13, 120, slots, 2)
    n1, n2 = sh.n1, sh.n2
    c0, c1 = sh.ciphertexts()
    sparse = [i * n1 + j for i in (1, 3) for j in range(n1)] + [2 * n1 + 2, 2]       # giant steps 1 and 3 zero, baby rotation 2 live nowhere
    plans = [sh.plan(sh.diagonals(zero=range(1, slots))), sh.plan(sh.diagonals(zero=sparse)), sh.plan(sh.diagonals()),
             sh.plan(sh.diagonals(zero=range(slots)))]
    try:
        assert [p.live for p in plans] == [1, slots - len(sparse), slots, 0] and all(p.exact for p in plans)
        expect = [sh.planned(p, c0, c1) for p in plans]
        with sh.g.gemv_multi(plans) as ms:
            union = [int(any(p.rotations()[r] for p in plans)) for r in range(slots)]
            assert ms.rotations() == union and ms.baby == n1
            needed = {r for r in range(slots) if union[r]}
            assert needed == set(range(n1)) | {i * n1 for i in range(n2)}
            outs0, outs1 = sh.multi(ms, c0, c1, only=needed)
            torch.cuda.synchronize()
            assert not outs0[3].any() and not outs1[3].any()
            for t in range(3):
                same((outs0[t], outs1[t]), expect[t], "plan %d" % t)
        with sh.g.gemv_multi(plans[:2]) as ms:
            union = ms.rotations()
            assert union == [int(plans[0].rotations()[r] or plans[1].rotations()[r]) for r in range(slots)]
            needed = {r for r in range(slots) if union[r]}
            assert needed == {0, 1, 3, 2 * n1}                   # rotation 0 is both plans', the others only the second one's
            assert ms.baby == 3
            with pytest.raises(_native.GpqError, match="NULL"):
                sh.multi(ms, c0, c1, only=needed - {3})          # read by the second plan alone
            outs0, outs1 = sh.multi(ms, c0, c1, only=needed)     # rotation 2, n1 and 3 n1: keys of nobody
            for t in range(2):
                same((outs0[t], outs1[t]), expect[t], "plan %d of two" % t)
    finally:
        _close(plans)


def test_a_set_of_zero_matrices(engine_ctx):
    """no plan has a live diagonal: the union of the baby rotations is empty, nothing is rotated or summed, every output is the planned call's"""
    slots, k = 4, NP + 1
    sh = MultiShape(engine_ctx, 10, 120, slots, 3)
    c0, c1 = sh.ciphertexts()
    plans = _plans(sh, k, zero=range(slots))
    try:
        assert all(p.exact and p.live == 0 for p in plans)
        expect = [sh.planned(p, c0, c1) for p in plans]
        try:
            sh.g.set_chunk(2)                                # two launch groups, the last one odd
            with sh.g.gemv_multi(plans) as ms:
                assert ms.count == k and ms.baby == 0 and not any(ms.rotations())
                got = []
                cnt = counts(sh.g, lambda: got.append(sh.multi(ms, c0, c1, only=set())))
                for t in range(k):
                    same((got[0][0][t], got[0][1][t]), expect[t], "plan %d of %d" % (t, k))
        finally:
            sh.g.set_chunk(32)
        assert cnt.get("gemv_mac_multi", 0) == 0 and cnt.get("keyswitch_rot_mid", 0) == 0, cnt
    finally:
        _close(plans)


def test_different_dims_in_one_set(engine_ctx):
    """logn 10, q = 2^135, slots 64: eight 30-bit products need a fourth limb (tests/test_gemv_inner_gpu.py), 8-bit ones fit he_mulpt's three"""
    sh = MultiShape(engine_ctx, 10, 135, 64, 2, limbs=5)
    assert sh.dimpt == 3
    c0, c1 = sh.ciphertexts()
    plans = [sh.plan(sh.diagonals(bits=30)), sh.plan(sh.diagonals(bits=8))]
    try:
        assert all(p.exact for p in plans) and [p.dim for p in plans] == [4, 3]
        expect = [sh.planned(p, c0, c1) for p in plans]
        for order in ((0, 1), (1, 0)):
            with sh.g.gemv_multi([plans[t] for t in order]) as ms:
                assert ms.dim == 4
                outs0, outs1 = sh.multi(ms, c0, c1)
                for at, t in enumerate(order):
                    same((outs0[at], outs1[at]), expect[t], "plan of dim %d at position %d" % (plans[t].dim, at))
    finally:
        _close(plans)


def test_launch_counts_of_the_shared_stage(engine_ctx):
    logn, logq, slots, batch, k = 13, 120, 16, 2, 3
    sh = MultiShape(engine_ctx, logn, logq, slots, batch)
    g, n1, n2 = sh.g, sh.n1, sh.n2
    c0, c1 = sh.ciphertexts()
    o0, o1 = torch.empty_like(c0), torch.empty_like(c1)
    r0 = torch.empty(n1 * c0.numel(), dtype=torch.int64, device="cuda")
    r1 = torch.empty_like(r0)
    plans = _plans(sh, k)
    try:
        with g.gemv_multi(plans) as ms:
            slab = torch.zeros(ms.dim * sh.n, dtype=torch.int64, device="cuda")
            swk = counts(g, lambda: g.he_swk(o0, o1, c0, c1, sh.keys[0][0], sh.keys[0][1], sh.W, logq, sh.dimB, sh.dimP))
            baby = counts(g, lambda: g.he_rot_hoisted(r0, r1, c0, c1, list(range(n1)), sh.k0()[:n1], sh.k1()[:n1], sh.W, logq, sh.dimB, sh.dimP))
            fwd = counts(g, lambda: g.poly_ntt(slab, ms.dim))        # one forward transform over the largest dim: launches per limb class
            multi = counts(g, lambda: sh.multi(ms, c0, c1))
            get = lambda d, key: d.get(key, 0)
            rest = lambda key: get(baby, key) + k * n2 * get(swk, key)
            groups = -(-k // NP)
            assert get(multi, "gemv_mac") == 0, multi
            assert get(multi, "gemv_mac_multi") == n2 * groups, multi
            for key in ("strided_fwd", "contig_fwd"):
                assert get(multi, key) - rest(key) == get(fwd, key) > 0, (key, multi, baby, swk, fwd)
            assert get(multi, "bridge_decompose") - rest("bridge_decompose") == 2, (multi, baby, swk)
            assert get(baby, "keyswitch_rot_mid") > 0
            for key in ("keyswitch_rot_mid", "automorphism_gather"):
                assert get(multi, key) == get(baby, key), (key, multi, baby)
            try:
                g.set_chunk(1)                               # two launch groups
                assert counts(g, lambda: sh.multi(ms, c0, c1))["gemv_mac_multi"] == 2 * n2 * groups
            finally:
                g.set_chunk(32)
    finally:
        _close(plans)


def test_refusals_launch_nothing(engine_ctx):
    sh = MultiShape(engine_ctx, 10, 120, 4, 1)
    g, lib = sh.g, sh.g.lib
    other = engine_ctx(10, max(sh.dimB, sh.dimpt) + 1)
    c0, c1 = sh.ciphertexts()
    outs = [torch.zeros_like(c0) for _ in range(4)]
    P = lambda t: C.c_void_p(t.data_ptr())
    diag = sh.diagonals()
    huge = np.zeros((sh.slots, sh.W, sh.n), dtype=np.uint64)
    huge[:, 0] = np.uint64((1 << 62) - 1)                    # 119 + 62 + 10 + 1 bits against 59 * 3: one product can wrap he_mulpt's basis
    plans = [sh.plan(diag), sh.plan(sh.diagonals())]
    foreign = other.gemv_plan(diag, sh.slots, sh.W, sh.logq, sh.dimpt)
    fewer = g.gemv_plan(diag, 2, sh.W, sh.logq, sh.dimpt)
    lower = g.gemv_plan(diag, sh.slots, sh.W, 100, sh.dimpt)
    inexact = sh.plan(to_device(huge.reshape(-1)))
    ms = g.gemv_multi(plans)
    elsewhere = other.gemv_multi([foreign, foreign])
    try:
        assert foreign.exact and fewer.exact and lower.exact and not inexact.exact
        ws = torch.zeros(lib.gpq_he_gemv_multi_workspace_bytes(g.h, ms.h, sh.W, sh.dimB, sh.dimP, 1) // 8 + 8, dtype=torch.int64, device="cuda")

        def call(o=None, src=c0, k0=None, W=sh.W, ctx=g, s=ms):
            o = outs if o is None else o
            k0 = sh.k0() if k0 is None else k0
            return lib.gpq_he_gemv_multi(ctx.h, g._key_ptrs(o[0::2]), g._key_ptrs(o[1::2]), P(src), P(c1), s.h, g._key_ptrs(k0), g._key_ptrs(sh.k1()), W,
                                         LOGDELTA, sh.dimB, sh.dimP, 1, P(ws), g._stream())

        assert call() == 0
        torch.cuda.synchronize()
        good = [t.clone() for t in outs]
        for t in outs:
            t.zero_()
        torch.cuda.synchronize()
        g.profile(True)
        other.profile(True)
        try:
            for bad, why in (([plans[0], foreign], "another context"), ([plans[0], fewer], "slots"), ([plans[0], lower], "slots"),
                             ([plans[0], inexact], "not exact"), ([], "plans"), ([plans[0]] * 17, "plans")):
                with pytest.raises(_native.GpqError, match=why):
                    g.gemv_multi(bad)
            assert g.gemv_multi([plans[0]] * 16).count == 16
            assert call(o=[c0] + outs[1:]) == -1 and b"alias" in lib.gpq_last_error()
            assert call(o=[outs[0], outs[1], outs[2], outs[0]]) == -1 and b"alias" in lib.gpq_last_error()
            missing = sh.k0()
            missing[2] = None                                # giant rotation 1 * n1
            assert call(k0=missing) == -1 and b"NULL" in lib.gpq_last_error()
            assert call(W=1) == -1
            assert call(ctx=other) == -1 and b"another context" in lib.gpq_last_error()
            assert call(s=elsewhere) == -1 and b"another context" in lib.gpq_last_error()
            assert g.profile_collect() == {} and other.profile_collect() == {}
        finally:
            g.profile(False)
            other.profile(False)
        torch.cuda.synchronize()
        assert not any(t.any() for t in outs) and all(t.any() for t in good)
    finally:
        ms.close()
        elsewhere.close()
        _close(plans + [foreign, fewer, lower, inexact])
