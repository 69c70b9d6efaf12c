"""Whole calls at n = 2^15 -- a parameter set of the reference (tests/test_ref_tables.py: (15, 881), (15, 590)) whose transforms take
seven strided stages, which no other file runs a fused middle, a key switch or a bridge call through -- and the same calls at 2^14 and
2^16 with one limb range of every butterfly class inside each transform.

q_L = q_l = 2^200: dimP / dimA / dimB = 4 / 8 / 12 and four-word coefficients, the smallest modulus at which the matrix-core front and the
one-product streaming tail run (tests/test_he_windows_gpu.py has the same limb counts at 2^13).  Batch 3, so that every key-switch middle
runs its pair form and its single form.  The arrangement (1, 2) of gpq_set_limb_classes -- limb 0 wide-split, limb 1 split, limbs
2 .. 11 7-mad -- stands next to the context's own choice; a context with changed classes is the test's own, and once its calls are done
the per-kernel profile proves that the three classes ran (tests/test_inject_gpu.py: assert_the_asked_classes_ran; the bridge's scaled
tables may end the wide range of a context for good, bridge_tables.hpp: apply_scaled_wide_limit).

Expectations are exact Python integers: one operand of every polynomial product has a handful of full-size coefficients
(tests/sparse_ints.py), as in tests/test_he_mul_full_gpu.py.  The hoisted rotation is compared with gpq_poly_rot + gpq_he_swk on the
device under the same arrangement; gpq_he_swk is the call the sparse keys anchor to the integers."""
import contextlib
import random

import numpy as np
import pytest

from gpqhe_amd import gemv_steps, to_device, to_host
from oracle import bigint_ref as ref
from oracle.expect import ints_to_words
from tests.sparse_ints import sparse_mul, sparse_terms
from tests.test_inject_gpu import assert_the_asked_classes_ran

pytestmark = pytest.mark.gpu

LOGQ, W, BATCH = 200, 4, 3
DIMS = {14: (4, 8, 12), 15: (4, 8, 12), 16: (4, 8, 12)}          # ring: (dimP, dimA, dimB) of he_dims(200, 200)
ALL_CLASSES = (1, 2)
# (logn, gpq_set_limb_classes arguments or None for the context's own choice)
RING15 = [(15, None), (15, ALL_CLASSES)]                         # every call of this file
CASES = RING15 + [(14, ALL_CLASSES), (16, ALL_CLASSES)]          # he_mul, he_swk, he_rot_hoisted
LOGDELTA_RS = 40
ROTS = [5, 40]
GEMV_SLOTS, GEMV_GIANT = 4, 1


def _torch():
    import torch
    return torch


@contextlib.contextmanager
def _context(engine_ctx, logn, classes):
    """(device context, (dimP, dimA, dimB)): the session's for the default arrangement, a context of the test's own otherwise"""
    import gpqhe_amd
    torch = _torch()
    dimP, dimA, dimB = DIMS[logn]
    if classes is None:
        g = engine_ctx(logn, dimB)
        assert g.he_dims(LOGQ, LOGQ) == (dimP, dimA, dimB, dimB)
        yield g, DIMS[logn]
        return
    g = gpqhe_amd.PolyContext(logn, dimB)
    try:
        assert g.he_dims(LOGQ, LOGQ) == (dimP, dimA, dimB, dimB)
        g.set_limb_classes(*classes)
        yield g, DIMS[logn]
        torch.cuda.synchronize()
        assert_the_asked_classes_ran(g, np.zeros(dimB << logn, dtype=np.uint64), dimB, classes)
    finally:
        torch.cuda.synchronize()
        g.close()


def _centred(rng, n):
    h = 1 << (LOGQ - 1)
    vals = [rng.randrange(-h, h) for _ in range(n)]
    vals[:4] = [0, -1, h - 1, -h]
    return vals


def _dev(polys):
    return to_device(np.concatenate([ints_to_words(v, W) for v in polys]))


def _key_slab(o, terms, dim):
    """the NTT-domain key slab of the polynomial sum(c X^k)"""
    a = np.zeros(dim * o.n, dtype=np.uint64)
    for d in range(dim):
        for k, c in terms:
            a[d * o.n + k] = c % o.p[d]
    return o.ntt_slab(a, dim)


def _assert_words(what, got, want, n):
    """got: device slab of the batch; want: one list of integers per ciphertext"""
    h, per = to_host(got), W * n
    assert h.size == per * len(want)
    for k, e in enumerate(want):
        bad = np.flatnonzero(h[k * per:(k + 1) * per] != ints_to_words(e, W))
        assert bad.size == 0, "%s of ciphertext %d: %d words differ from the integers, first at %s" % (what, k, bad.size, bad[:4])


_MUL, _SWK, _GEMV = {}, {}, {}


def _mul_case(o, logn):
    """src/he-mult.c:88-156 in integers, once per ring: d0 = c0 c0', d1 = c0 c1' + c1 c0', d2 = c1 c1' (smod q);
    out_i = smod(d_i + rdiv(smod(d2 * rlk.p_i, P q_L), P), q).  ct2 = (c0', c1') and the key polynomials are sparse."""
    if logn in _MUL:
        return _MUL[logn]
    dimP, _, dimB = DIMS[logn]
    n, q = 1 << logn, 1 << LOGQ
    P = ref.RnsBasis(o.p[:dimP]).P
    PqL = P * q
    rng = random.Random(1500 + logn)
    t0, t1 = sparse_terms(rng, n, 5, q >> 1), sparse_terms(rng, n, 5, q >> 1)
    k0, k1 = sparse_terms(rng, n, 6, PqL >> 1), sparse_terms(rng, n, 6, PqL >> 1)
    cts = [(_centred(rng, n), _centred(rng, n)) for _ in range(BATCH)]
    smod, exp0, exp1 = ref.mpi_smod, [], []
    for c0, c1 in cts:
        d0 = [smod(v, q) for v in sparse_mul(c0, t0, n)]
        d2 = [smod(v, q) for v in sparse_mul(c1, t1, n)]
        d1 = [smod(x + y, q) for x, y in zip(sparse_mul(c0, t1, n), sparse_mul(c1, t0, n))]
        exp0.append([smod(a + ref.mpi_rdiv(smod(b, PqL), P), q) for a, b in zip(d0, sparse_mul(d2, k0, n))])
        exp1.append([smod(a + ref.mpi_rdiv(smod(b, PqL), P), q) for a, b in zip(d1, sparse_mul(d2, k1, n))])
    dense = lambda terms: [dict(terms).get(i, 0) for i in range(n)]
    ins = [[ct[0] for ct in cts], [ct[1] for ct in cts], [dense(t0)] * BATCH, [dense(t1)] * BATCH]
    _MUL[logn] = ([np.concatenate([ints_to_words(v, W) for v in polys]) for polys in ins], (_key_slab(o, k0, dimB), _key_slab(o, k1, dimB)), exp0, exp1)
    return _MUL[logn]


def _swk_case(o, logn):
    """src/he-automorphism.c:40-85 in integers, once per ring: out_0 = smod(d0 + rdiv(smod(d1 k0, P q_L), P), q),
    out_1 = smod(rdiv(smod(d1 k1, P q_L), P), q) with sparse key polynomials"""
    if logn in _SWK:
        return _SWK[logn]
    dimP, _, dimB = DIMS[logn]
    n, q = 1 << logn, 1 << LOGQ
    P = ref.RnsBasis(o.p[:dimP]).P
    PqL = P * q
    rng = random.Random(2500 + logn)
    k0, k1 = sparse_terms(rng, n, 6, PqL >> 1), sparse_terms(rng, n, 6, PqL >> 1)
    ds = [(_centred(rng, n), _centred(rng, n)) for _ in range(BATCH)]
    smod = ref.mpi_smod
    exp0 = [[smod(a + ref.mpi_rdiv(smod(b, PqL), P), q) for a, b in zip(d0, sparse_mul(d1, k0, n))] for d0, d1 in ds]
    exp1 = [[smod(ref.mpi_rdiv(smod(b, PqL), P), q) for b in sparse_mul(d1, k1, n)] for _, d1 in ds]
    ins = [np.concatenate([ints_to_words(d[j], W) for d in ds]) for j in range(2)]
    _SWK[logn] = (ins, (_key_slab(o, k0, dimB), _key_slab(o, k1, dimB)), exp0, exp1)
    return _SWK[logn]


@pytest.mark.parametrize("logn,classes", CASES)
def test_he_mul_matches_the_integers(engine_ctx, oracle_ctx, logn, classes):
    torch = _torch()
    ins, keys, exp0, exp1 = _mul_case(oracle_ctx(logn, DIMS[logn][2]), logn)
    with _context(engine_ctx, logn, classes) as (g, (dimP, dimA, dimB)):
        dev = [to_device(v) for v in ins]
        o0, o1 = torch.empty_like(dev[0]), torch.empty_like(dev[0])
        g.he_mul(o0, o1, *dev, to_device(keys[0]), to_device(keys[1]), W, LOGQ, dimA, dimB, dimP)
        _assert_words("he_mul c0", o0, exp0, g.n)
        _assert_words("he_mul c1", o1, exp1, g.n)


@pytest.mark.parametrize("logn,classes", CASES)
def test_he_swk_matches_the_integers(engine_ctx, oracle_ctx, logn, classes):
    torch = _torch()
    ins, keys, exp0, exp1 = _swk_case(oracle_ctx(logn, DIMS[logn][2]), logn)
    with _context(engine_ctx, logn, classes) as (g, (dimP, _, dimB)):
        d0, d1 = to_device(ins[0]), to_device(ins[1])
        o0, o1 = torch.empty_like(d0), torch.empty_like(d0)
        g.he_swk(o0, o1, d0, d1, to_device(keys[0]), to_device(keys[1]), W, LOGQ, dimB, dimP)
        _assert_words("he_swk c0", o0, exp0, g.n)
        _assert_words("he_swk c1", o1, exp1, g.n)


@pytest.mark.parametrize("logn,classes", RING15)
def test_he_mul_rs_matches_the_integers_and_rides_in_the_streaming_tail(engine_ctx, oracle_ctx, logn, classes):
    """he_rs (src/he-rescale.c:33-54) of the he_mul expectation: mpi_rdiv by Delta = 2^40, then mpi_smod q_l / Delta"""
    torch = _torch()
    ins, keys, exp0, exp1 = _mul_case(oracle_ctx(logn, DIMS[logn][2]), logn)
    delta, qnext = 1 << LOGDELTA_RS, 1 << (LOGQ - LOGDELTA_RS)
    rs = lambda polys: [[ref.mpi_smod(ref.mpi_rdiv(v, delta), qnext) for v in e] for e in polys]
    with _context(engine_ctx, logn, classes) as (g, (dimP, dimA, dimB)):
        dev = [to_device(v) for v in ins]
        o0, o1 = torch.empty_like(dev[0]), torch.empty_like(dev[0])
        try:
            g.profile(True)
            g.profile_collect()
            g.he_mul_rs(o0, o1, *dev, to_device(keys[0]), to_device(keys[1]), W, LOGQ, dimA, dimB, dimP, LOGDELTA_RS)
            torch.cuda.synchronize()
            prof = g.profile_collect()
        finally:
            g.profile(False)
        assert "bridge_tail_stream" in prof, sorted(prof)
        _assert_words("he_mul_rs c0", o0, rs(exp0), g.n)
        _assert_words("he_mul_rs c1", o1, rs(exp1), g.n)


@pytest.mark.parametrize("logn,classes", CASES)
def test_hoisted_rotations_equal_poly_rot_and_he_swk(engine_ctx, logn, classes):
    torch = _torch()
    from tests.test_he_rot_hoisted_gpu import _composed, _dense
    n = 1 << logn
    rng = np.random.default_rng(3500 + logn)
    c0 = to_device(np.concatenate([_dense(rng, W, n, LOGQ) for _ in range(BATCH)]))
    c1 = to_device(np.concatenate([_dense(rng, W, n, LOGQ) for _ in range(BATCH)]))
    with _context(engine_ctx, logn, classes) as (g, (dimP, _, dimB)):
        keys = [tuple(to_device(np.concatenate([rng.integers(0, g.p[d], size=n, dtype=np.uint64) for d in range(dimB)])) for _ in range(2)) for _ in ROTS]
        out0 = torch.empty(len(ROTS) * c0.numel(), dtype=torch.int64, device="cuda")
        out1 = torch.empty_like(out0)
        g.he_rot_hoisted(out0, out1, c0, c1, ROTS, [k[0] for k in keys], [k[1] for k in keys], W, LOGQ, dimB, dimP)
        e0, e1 = _composed(g, c0, c1, ROTS, keys, W, LOGQ, dimB, dimP)
        torch.cuda.synchronize()
        for name, a, b in (("c0", out0, e0), ("c1", out1, e1)):
            bad = torch.nonzero(a != b).flatten()
            assert bad.numel() == 0, "%s: %d words differ, first at %s" % (name, bad.numel(), bad[:4].tolist())
        assert len(set(to_host(out0[:n]).tolist())) > n // 2        # not degenerate


def _gemv_case(logn):
    """One giant step's inner sum of he_gemv (src/he-algo.c:70-78) in integers, once per ring: smod(sum_j rot_j * diag[giant n1 + j], q)
    for he_ecd-shaped sparse diagonals and dense rotations, built as tests/test_gemv_inner_gpu.py builds them"""
    if logn in _GEMV:
        return _GEMV[logn]
    from tests.test_gemv_inner_gpu import LOGDELTA, _diag
    n, q = 1 << logn, 1 << LOGQ
    n1, _ = gemv_steps(GEMV_SLOTS)
    rng = random.Random(4500 + logn)
    diags = [_diag(rng, n, GEMV_SLOTS, True, LOGDELTA) for _ in range(GEMV_SLOTS)]
    rots = [[(_centred(rng, n), _centred(rng, n)) for _ in range(BATCH)] for _ in range(n1)]
    terms = [[(i, v) for i, v in enumerate(d) if v] for d in diags[GEMV_GIANT * n1:(GEMV_GIANT + 1) * n1]]
    exp = []
    for c in range(2):
        prods = [[sparse_mul(rots[j][b][c], terms[j], n) for j in range(n1)] for b in range(BATCH)]
        exp.append([[ref.mpi_smod(sum(col), q) for col in zip(*prods[b])] for b in range(BATCH)])
    slabs = [np.concatenate([ints_to_words(rots[j][b][c], W) for j in range(n1) for b in range(BATCH)]) for c in range(2)]
    _GEMV[logn] = (np.concatenate([ints_to_words(d, W) for d in diags]), slabs, exp)
    return _GEMV[logn]


@pytest.mark.parametrize("logn,classes", RING15)
def test_gemv_inner_matches_the_integers(engine_ctx, logn, classes):
    torch = _torch()
    from tests.test_gemv_inner_gpu import _dimpt
    diag, slabs, exp = _gemv_case(logn)
    with _context(engine_ctx, logn, classes) as (g, _):
        with g.gemv_plan(to_device(diag), GEMV_SLOTS, W, LOGQ, _dimpt(LOGQ, logn)) as plan:
            assert plan.exact and plan.live == GEMV_SLOTS
            out0 = torch.empty(BATCH * W * g.n, dtype=torch.int64, device="cuda")
            out1 = torch.empty_like(out0)
            g.gemv_inner(out0, out1, to_device(slabs[0]), to_device(slabs[1]), plan, GEMV_GIANT, W)
            torch.cuda.synchronize()
        _assert_words("gemv_inner c0", out0, exp[0], g.n)
        _assert_words("gemv_inner c1", out1, exp[1], g.n)
