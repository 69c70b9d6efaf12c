"""gpq_gemv_plan_* and gpq_gemv_inner: one giant step's inner sum of he_gemv (src/he-algo.c:65-79) accumulated in the NTT domain, against
Python integers -- the sum over j of oracle.bigint_ref.he_mulpt(rot_j, diag[i n1 + j]) folded with he_add -- on every coefficient:

* random inputs at logn 10 - 12, slots 1 .. 64, batch 1 and 3, he_ecd-shaped sparse and dense diagonals, zero diagonals and zero giant steps;
* the adversarial shape that makes dim > dimpt matter (logn 10, q = 2^135, 30-bit diagonals, slots 64: every single product fits the
  reference's three limbs, the sum of eight does not), and the exactness guard one and two bits further;
* every butterfly class on every limb and both cache policies on two-pass rings (logn 13: eight low stages, logn 17: nine)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import gpqhe_amd
from gpqhe_amd import big_to_ints, gemv_acc_dim, gemv_steps, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref

pytestmark = pytest.mark.gpu
LOGDELTA = 30


def _dimpt(logql, logn):
    return (logql + 1 + LOGDELTA + logn) // 59 + 1           # src/he-mult.c:168 with nu = 2^LOGDELTA


def _diag(rng, n, slots, sparse, bits):
    if sparse:                                   # what he_ecd makes of a slot vector: 2 slots non-zero terms at stride n / (2 slots)
        v = [0] * n
        for t in range(2 * slots):
            v[t * (n // (2 * slots))] = rng.randrange(-(1 << bits) + 1, 1 << bits)
        return v
    return [rng.randrange(-(1 << bits) + 1, 1 << bits) for _ in range(n)]


def _centred(rng, logq, n):
    h = 1 << (logq - 1)
    vals = [rng.randrange(-h, h) for _ in range(n)]
    vals[:4] = [0, -1, h - 1, -h]
    return vals


def _expected(o, rots, diags, dimpt, logql):
    """src/he-algo.c:70-78 for one ciphertext: rots[j] = (c0, c1) of the j-th baby rotation, diags[j] the step's j-th plaintext"""
    inner = None
    for ct, m in zip(rots, diags):
        prod = ref.he_mulpt(o, ct, m, dimpt, logql)
        inner = prod if inner is None else ref.he_add(inner, prod, 1 << logql)
    return inner


def _slabs(rots, W, batch):
    """rots[j][b] = (c0, c1) -> the two rotation-major big slabs"""
    r0 = np.concatenate([ints_to_big(rots[j][b][0], W) for j in range(len(rots)) for b in range(batch)])
    r1 = np.concatenate([ints_to_big(rots[j][b][1], W) for j in range(len(rots)) for b in range(batch)])
    return to_device(r0), to_device(r1)


def _inner(g, plan, R0, R1, giant, W, batch):
    out0 = torch.empty(batch * W * g.n, dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    g.gemv_inner(out0, out1, R0, R1, plan, giant, W)
    torch.cuda.synchronize()
    return big_to_ints(to_host(out0), W, g.n), big_to_ints(to_host(out1), W, g.n)


@pytest.mark.parametrize("logn,slots,batch,sparse,giant", [(10, 1, 1, True, 0), (10, 2, 3, False, 0), (10, 4, 1, False, 1), (11, 8, 3, True, 1),
                                                           (11, 16, 1, False, 3), (10, 32, 3, True, 2), (12, 64, 1, False, 7), (10, 64, 3, True, 0)])
def test_inner_sum_matches_the_integers(engine_ctx, oracle_ctx, logn, slots, batch, sparse, giant):
    logq = 120
    dimpt = _dimpt(logq, logn)
    g, o = engine_ctx(logn, dimpt + 1), oracle_ctx(logn, dimpt + 1)
    n, W = g.n, (logq + 63) // 64
    n1, n2 = gemv_steps(slots)
    rng = random.Random(logn * 1000 + slots * 10 + batch)
    diags = [_diag(rng, n, slots, sparse, LOGDELTA) for _ in range(slots)]
    with g.gemv_plan(to_device(np.concatenate([ints_to_big(d, W) for d in diags])), slots, W, logq, dimpt) as plan:
        assert plan.exact and plan.live == slots and plan.bytes == slots * plan.dim * n * 8
        assert plan.dim == max(dimpt, gemv_acc_dim(logq, max(max(abs(v) for v in d) for d in diags).bit_length(), logn, n1))
        rots = [[(_centred(rng, logq, n), _centred(rng, logq, n)) for _ in range(batch)] for _ in range(n1)]
        R0, R1 = _slabs(rots, W, batch)
        got0, got1 = _inner(g, plan, R0, R1, giant, W, batch)
    for b in range(batch):
        e0, e1 = _expected(o, [rots[j][b] for j in range(n1)], diags[giant * n1:(giant + 1) * n1], dimpt, logq)
        assert got0[b] == e0, "ciphertext %d: c0" % b
        assert got1[b] == e1, "ciphertext %d: c1" % b


def test_zero_diagonals_and_zero_giant_steps(engine_ctx, oracle_ctx):
    logn, logq, slots, batch = 10, 120, 16, 2
    dimpt = _dimpt(logq, logn)
    g, o = engine_ctx(logn, dimpt + 1), oracle_ctx(logn, dimpt + 1)
    n, W = g.n, (logq + 63) // 64
    n1, n2 = gemv_steps(slots)
    rng = random.Random(77)
    diags = [_diag(rng, n, slots, False, LOGDELTA) for _ in range(slots)]
    for k in (0, 2, 3, 4, 5, 6, 7, 9):                       # giant step 1 is zero altogether, step 0 keeps diagonal 1 only, step 2 loses diagonal 9
        diags[k] = [0] * n
    with g.gemv_plan(to_device(np.concatenate([ints_to_big(d, W) for d in diags])), slots, W, logq, dimpt) as plan:
        assert plan.exact and plan.live == slots - 8
        rots = [[(_centred(rng, logq, n), _centred(rng, logq, n)) for _ in range(batch)] for _ in range(n1)]
        R0, R1 = _slabs(rots, W, batch)
        for giant in (0, 1, 2):
            got0, got1 = _inner(g, plan, R0, R1, giant, W, batch)
            for b in range(batch):
                e0, e1 = _expected(o, [rots[j][b] for j in range(n1)], diags[giant * n1:(giant + 1) * n1], dimpt, logq)
                assert got0[b] == e0 and got1[b] == e1, "giant step %d, ciphertext %d" % (giant, b)
            if giant == 1:
                assert not any(got0[0]) and not any(got1[1])


ADV = dict(logn=10, logq=135, slots=64)


def test_the_sum_needs_one_limb_more_than_each_product(engine_ctx, oracle_ctx):
    """All ciphertext coefficients +(2^134 - 1), all diagonal coefficients +(2^30 - 1): coefficient n - 1 of every product is n cmax dmax, below
    half the three-limb modulus, and the eight-term sum is above it -- summed in the reference's three limbs it would wrap."""
    logn, logq, slots = ADV["logn"], ADV["logq"], ADV["slots"]
    dimpt = _dimpt(logq, logn)
    assert dimpt == 3
    g, o = engine_ctx(logn, 5), oracle_ctx(logn, 5)
    n, W = g.n, (logq + 63) // 64
    n1, n2 = gemv_steps(slots)
    cmax, dmax = (1 << 134) - 1, (1 << 30) - 1
    P3 = ref.RnsBasis(o.p[:3]).P
    assert 2 * n * cmax * dmax < P3 < 2 * n1 * n * cmax * dmax
    ct, m = ([cmax] * n, [cmax] * n), [dmax] * n
    with g.gemv_plan(to_device(np.concatenate([ints_to_big(m, W)] * slots)), slots, W, logq, dimpt) as plan:
        assert plan.exact and plan.dim == 4 and plan.live == slots
        R0, R1 = _slabs([[ct]] * n1, W, 1)
        got0, got1 = _inner(g, plan, R0, R1, 5, W, 1)
    prod = ref.he_mulpt(o, ct, m, dimpt, logq)
    assert prod[0][n - 1] == ref.mpi_smod(n * cmax * dmax, 1 << logq)      # the restated reference is exact on these inputs
    e = prod
    for _ in range(n1 - 1):
        e = ref.he_add(e, prod, 1 << logq)
    assert got0[0] == e[0] and got1[0] == e[1]


@pytest.mark.parametrize("bits,exact", [(32, True), (33, False)])
def test_exactness_guard(engine_ctx, oracle_ctx, bits, exact):
    """134 + bits + 10 + 1 against 59 * 3 = 177: 32-bit diagonals still multiply exactly in the reference's basis, 33-bit ones need not"""
    logn, logq, slots = ADV["logn"], ADV["logq"], ADV["slots"]
    dimpt = _dimpt(logq, logn)
    g, o = engine_ctx(logn, 5), oracle_ctx(logn, 5)
    n, W = g.n, (logq + 63) // 64
    n1, n2 = gemv_steps(slots)
    rng = random.Random(bits)
    diags = [_diag(rng, n, slots, False, 30) for _ in range(slots)]
    diags[9][17] = -((1 << bits) - 1)                        # one coefficient of `bits` bits decides
    rots = [[(_centred(rng, logq, n), _centred(rng, logq, n))] for _ in range(n1)]
    R0, R1 = _slabs(rots, W, 1)
    with g.gemv_plan(to_device(np.concatenate([ints_to_big(d, W) for d in diags])), slots, W, logq, dimpt) as plan:
        assert plan.exact == exact and plan.live == slots
        if exact:
            assert plan.dim == 4 and plan.bytes == slots * 4 * n * 8
            got0, got1 = _inner(g, plan, R0, R1, 1, W, 1)
            e0, e1 = _expected(o, [rots[j][0] for j in range(n1)], diags[n1:2 * n1], dimpt, logq)
            assert got0[0] == e0 and got1[0] == e1
            return
        lib, P = g.lib, lambda t: C.c_void_p(t.data_ptr())
        out0, out1 = torch.zeros(W * n, dtype=torch.int64, device="cuda"), torch.zeros(W * n, dtype=torch.int64, device="cuda")
        ws = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
        assert lib.gpq_gemv_inner(g.h, P(out0), P(out1), P(R0), P(R1), plan.h, 1, W, 1, P(ws), None) == -1
        assert b"not exact" in lib.gpq_last_error()
        keys = (C.c_void_p * slots)(*[ws.data_ptr()] * slots)
        assert lib.gpq_he_gemv_planned(g.h, P(out0), P(out1), P(R0), P(R1), plan.h, keys, keys, W, 0, 3, 3, 1, P(ws), None) == -1
        assert b"not exact" in lib.gpq_last_error()
        torch.cuda.synchronize()
        assert not out0.any() and not out1.any()


def test_a_plan_that_does_not_fit_the_context_is_not_exact(engine_ctx):
    logn, logq, slots = ADV["logn"], ADV["logq"], ADV["slots"]
    g = engine_ctx(logn, 3)                                  # the sum needs four limbs
    n, W = g.n, (logq + 63) // 64
    with g.gemv_plan(to_device(np.concatenate([ints_to_big([(1 << 30) - 1] * n, W)] * slots)), slots, W, logq, 3) as plan:
        assert plan.dim == 4 and not plan.exact and plan.bytes == 0


def _dense(rng, W, n, logq):
    w = rng.integers(0, 1 << 63, size=(W, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(W, n), dtype=np.uint64)
    top = logq - 1 - 64 * (W - 1)
    w[W - 1] = rng.integers(-(1 << top), 1 << top, size=n, dtype=np.int64).view(np.uint64)
    return w.reshape(-1)


def _classes_and_policies(engine_ctx, oracle_ctx, logn, slots, batch, giant):
    logq = 120
    dimpt = _dimpt(logq, logn)
    o = oracle_ctx(logn, dimpt + 1)
    n, W = 1 << logn, (logq + 63) // 64
    n1, n2 = gemv_steps(slots)
    rng = np.random.default_rng(logn)
    dg = np.zeros((slots, W, n), dtype=np.uint64)
    dg[:, 0] = rng.integers(-(1 << LOGDELTA) + 1, 1 << LOGDELTA, size=(slots, n), dtype=np.int64).view(np.uint64)
    dg[:, 1:] = (dg[:, :1].view(np.int64) >> 63).view(np.uint64)        # sign extension
    r0 = np.concatenate([_dense(rng, W, n, logq) for _ in range(n1 * batch)])
    r1 = np.concatenate([_dense(rng, W, n, logq) for _ in range(n1 * batch)])
    i0, i1, di = big_to_ints(r0, W, n), big_to_ints(r1, W, n), big_to_ints(dg.reshape(-1), W, n)
    expected = [_expected(o, [(i0[j * batch + b], i1[j * batch + b]) for j in range(n1)], di[giant * n1:(giant + 1) * n1], dimpt, logq) for b in range(batch)]
    for nt, classes in [(0, None), (1, None), (-1, (0, 0)), (-1, (0, 64)), (-1, (64, 64))]:
        g = engine_ctx(logn, dimpt + 1) if classes is None else gpqhe_amd.PolyContext(logn, dimpt + 1)
        try:
            if classes is not None:
                g.set_limb_classes(*classes)
            g.set_nt_policy(nt)
            with g.gemv_plan(to_device(dg.reshape(-1)), slots, W, logq, dimpt) as plan:
                assert plan.exact
                got0, got1 = _inner(g, plan, to_device(r0), to_device(r1), giant, W, batch)
        finally:
            g.set_nt_policy(-1)
            if classes is not None:
                torch.cuda.synchronize()
                g.close()
        for b in range(batch):
            assert got0[b] == expected[b][0] and got1[b] == expected[b][1], "nt %d, classes %s, ciphertext %d" % (nt, classes, b)


def test_every_butterfly_class_and_cache_policy_low8(engine_ctx, oracle_ctx):
    _classes_and_policies(engine_ctx, oracle_ctx, 13, 4, 3, 1)


@pytest.mark.timeout(1800)
def test_every_butterfly_class_and_cache_policy_low9(engine_ctx, oracle_ctx):
    _classes_and_policies(engine_ctx, oracle_ctx, 17, 2, 1, 0)
