"""Whole gpq_he_mul / gpq_he_swk / gpq_he_mul_rs / gpq_he_rot_hoisted calls on coefficients that sit IN THE ROUNDING WINDOWS of the
one-product relinearisation tail on the kernels' own decision (no gpq_debug_force_redo): bridge_tail_stream flags them by its window
tests, and the exact kernels behind it (bridge_fallback_tail_pre / _post, bridge_limb_scale, the front re-run, bridge_roundfix,
bridge_addround, bridge_rescale_masked), working under a per-wave FlagScope, write them.  tests/window_cases.py builds the inputs: the key
switch of 1 with the key NTT(X) returns X, so a ciphertext with c1 = 1 (he_mul: a1 = b1 = 1) and a key made from chosen residues hands
the tail exactly the chosen integers -- x mod P on half-1 .. half+2, 0, 1, 2, P-1, P-2 and on ladders across the window edges, crossed with
the wrap corner of the quotient -- next to random coefficients and clean groups of 64, so that waves without a flag sit next to flagged ones.

Every expected value comes from the restated reference (oracle/bigint_ref: he_mul, he_swk, he_relin_tail, mpi_rdiv / mpi_smod; worker
processes of tests/he_anchors.py), every coefficient of every output is compared, and the per-kernel profile proves that the streaming
tail ran under the default settings.  The same inputs then run under every other setting of the tail.

OUT OF SCOPE: the CRT windows of d2 and of the addends (amb_d, bridge_crt_decompose) cannot be reached by operands in the centred range
(|d| <= n q^2 / 2 is far below P_A / 2, so the fraction of d / P_A is never within 2^-38 of 1/2); they stay with gpq_debug_force_redo
(tests/test_stream_bridge_gpu.py)."""
import random

import numpy as np
import pytest

from oracle import bigint_ref as ref
from oracle.expect import words_to_ints
from tests import window_cases as wc
from tests.he_anchors import assert_anchored, expect_all, he_mul_tasks, he_swk_tasks

pytestmark = pytest.mark.gpu

# (logn, log2 q_L, log2 q_l).  The key switch hands the tail limbs weighted for the one-product tail only in the two-pass transforms
# (bridge_tables.hpp: can_prescale, logn > 12), so n = 2^13 is the smallest ring in which bridge_tail_stream runs inside a whole call:
#   STREAM_SHAPES  dims 4/8/12 (<8,4,true,6>, he_swk <6,0,false,3>); 8/16/24, the reference's default limb counts; 15/30/45 with 14 words
#                  (<12,8,true,5>, <12,0,false,4>); a lower level of it (zero-padded k steps) -- here the profile must show the streaming tail;
#   SMALL_SHAPES   the same moduli in single-pass rings (dims 4/7/11, 8/16/24, 15/30/45): the same coefficients reach round 3's tail
#                  (bridge_relin_front_mfma and the CRT kernels behind it, whose windows sit at the same values of x mod P).
STREAM_SHAPES = [(13, 200, 200), (13, 438, 438), (13, 850, 850), (13, 850, 500)]
SMALL_SHAPES = [(9, 200, 200), (10, 438, 438), (9, 850, 850), (9, 850, 500)]
SHAPES = STREAM_SHAPES + SMALL_SHAPES
BATCH, CHUNK, CRAFTED = 5, 2, (1, 4)                 # three launch groups, the last one short; a crafted ciphertext second in a full group, one alone


def _torch():
    import torch
    return torch


def _dev(values, W):
    from gpqhe_amd import ints_to_big, to_device
    return to_device(np.concatenate([ints_to_big(v, W) for v in values]))


def _centred(rng, logq, n):
    h = 1 << (logq - 1)
    return [rng.randrange(-h, h) for _ in range(n)]


def _one(n):
    return [1] + [0] * (n - 1)


def _setup(engine_ctx, oracle_ctx, logn, logqL, logql):
    dimP, dimA, dimB, dimevk = ref.he_dims(logn, oracle_ctx(logn, 60).p, logqL, logql)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    assert (dimP, dimA, dimB, dimevk) == g.he_dims(logqL, logql) and g.p[:dimB] == o.p[:dimB]
    return g, o, (dimA, dimB, dimP), (logqL + 64) // 64, wc.TailModel(o.p, dimP, dimB)


def _key(o, crafted, dimB):
    from gpqhe_amd import to_device
    return to_device(o.ntt_slab(crafted.slab(o.p, dimB), dimB))


def _report(what, crafted):
    for name, c in zip(("key 0", "key 1"), crafted):
        print("%s %s: crafted per class %s; %d of %d crafted coefficients modelled inside a window (%d below 1/2, %d below 1)"
              % (what, name, sorted(c.counts().items()), len(c.win), len(c.cls), sum(1 for w in c.win.values() if w == 1),
                 sum(1 for w in c.win.values() if w == 2)))


_CASES = {}


def _case(engine_ctx, oracle_ctx, logn, logqL, logql):
    """inputs and reference outputs of one shape, computed once: BATCH ciphertext pairs (a1 = b1 = 1 in the crafted ones), a (d0, d1) batch for
    he_swk (d1 = 1 in the crafted ones), the two keys, and ref.he_mul / ref.he_swk of every ciphertext"""
    key = (logn, logqL, logql)
    if key in _CASES:
        return _CASES[key]
    g, o, dims, W, M = _setup(engine_ctx, oracle_ctx, logn, logqL, logql)
    n, dimB = g.n, dims[1]
    rng = random.Random(7000 + logn + logql)
    crafted = [wc.build(M, n, 31 + logql), wc.build(M, n, 32 + logql)]
    _report("n=2^%d q_L=2^%d q_l=2^%d" % key, crafted)
    rlk = [_key(o, c, dimB) for c in crafted]
    cts = [[_centred(rng, logql, n) for _ in range(BATCH)] for _ in range(4)]          # a0, a1, b0, b1
    swk = [[_centred(rng, logql, n) for _ in range(BATCH)] for _ in range(2)]          # d0, d1
    for k in CRAFTED:
        cts[1][k], cts[3][k], swk[1][k] = _one(n), _one(n), _one(n)
    cts, swk = [_dev(v, W) for v in cts], [_dev(v, W) for v in swk]
    idx = list(range(BATCH))
    want = expect_all(he_mul_tasks(logn, logql, W, dims, cts, rlk, idx) + he_swk_tasks(logn, logql, W, dims, swk, rlk, idx))
    _CASES[key] = (g, dims, W, cts, swk, rlk, want[:BATCH], want[BATCH:])
    return _CASES[key]


def _he_mul(g, cts, rlk, W, logql, dims):
    torch = _torch()
    o0, o1 = torch.empty_like(cts[0]), torch.empty_like(cts[0])
    g.he_mul(o0, o1, *cts, rlk[0], rlk[1], W, logql, *dims)
    torch.cuda.synchronize()
    return o0, o1


def _he_swk(g, d, swk, W, logql, dims):
    torch = _torch()
    o0, o1 = torch.empty_like(d[0]), torch.empty_like(d[0])
    g.he_swk(o0, o1, d[0], d[1], swk[0], swk[1], W, logql, dims[1], dims[2])
    torch.cuda.synchronize()
    return o0, o1


def _compare(what, got, want, per, keys=("c0", "c1")):
    for name, t, key in zip(("c0", "c1"), got, keys):
        assert_anchored("%s %s" % (what, name), t, want, key, list(range(len(want))), per)


@pytest.mark.parametrize("logn,logqL,logql", SHAPES)
def test_he_mul_and_he_swk_on_window_coefficients(engine_ctx, oracle_ctx, logn, logqL, logql):
    g, dims, W, cts, swk, rlk, want_mul, want_swk = _case(engine_ctx, oracle_ctx, logn, logqL, logql)
    per = W * g.n
    try:
        g.set_chunk(CHUNK)
        g.profile(True)
        g.profile_collect()
        mul = _he_mul(g, cts, rlk, W, logql, dims)
        prof_mul = g.profile_collect()
        sw = _he_swk(g, swk, rlk, W, logql, dims)
        prof_swk = g.profile_collect()
    finally:
        g.profile(False)
        g.set_chunk(32)
    print("he_mul kernels: %s" % sorted(prof_mul))
    print("he_swk kernels: %s" % sorted(prof_swk))
    _compare("he_mul", mul, want_mul, per)
    _compare("he_swk", sw, want_swk, per)
    # Which tail ran.  (That the exact kernels WROTE the flagged coefficients is shown by the comparison above, not by the profile: the masked
    # kernels are launched behind every streamed call, flagged or not; at half+1, half+2 and on the half+k ladder the streaming kernel's own
    # result is wrong by construction -- its estimate is below 1/2, the truth above -- so only the exact path gives the reference's word.)
    for name, prof in (("he_mul", prof_mul), ("he_swk", prof_swk)):
        if logn > 12:
            assert "bridge_tail_stream" in prof and prof["bridge_tail_stream"][1] >= 3, (name, sorted(prof))     # one per launch group
        else:
            assert "bridge_relin_front" in prof, (name, sorted(prof))


def _settings():
    """(name, apply, restore) of every other way the tail can run"""
    return [
        ("two lanes", lambda g: g.set_overlap(True), lambda g: g.set_overlap(-1)),
        ("separate kernels", lambda g: g.set_stream_bridge(False), lambda g: g.set_stream_bridge(True)),
        ("prescale 0", lambda g: g.set_prescale(0), lambda g: g.set_prescale(g.PRESCALE_DEFAULT)),
        ("prescale 1", lambda g: g.set_prescale(1), lambda g: g.set_prescale(g.PRESCALE_DEFAULT)),
        ("prescale 2", lambda g: g.set_prescale(2), lambda g: g.set_prescale(g.PRESCALE_DEFAULT)),
        ("VALU bridge", lambda g: g.set_bridge_mfma(False), lambda g: g.set_bridge_mfma(True)),
        ("exact CRT", lambda g: g.set_exact_crt(True), lambda g: g.set_exact_crt(False)),
    ]


@pytest.mark.parametrize("setting", range(len(_settings())), ids=[s[0].replace(" ", "_") for s in _settings()])
def test_every_setting_gives_the_reference_on_window_coefficients(engine_ctx, oracle_ctx, setting):
    logn, logqL, logql = STREAM_SHAPES[0]
    g, dims, W, cts, swk, rlk, want_mul, want_swk = _case(engine_ctx, oracle_ctx, logn, logqL, logql)
    name, apply, restore = _settings()[setting]
    try:
        g.set_chunk(CHUNK)
        apply(g)
        mul = _he_mul(g, cts, rlk, W, logql, dims)
        if name == "two lanes":
            assert g.last_lanes() == 2
        sw = _he_swk(g, swk, rlk, W, logql, dims)
    finally:
        restore(g)
        g.set_chunk(32)
    _compare("he_mul (%s)" % name, mul, want_mul, W * g.n)
    _compare("he_swk (%s)" % name, sw, want_swk, W * g.n)


@pytest.mark.parametrize("logDelta", [1, 40, 63, 64])
@pytest.mark.parametrize("logn,logqL,logql", [STREAM_SHAPES[0], STREAM_SHAPES[2], SMALL_SHAPES[0], SMALL_SHAPES[2]])
def test_he_mul_rs_on_window_coefficients(engine_ctx, oracle_ctx, logn, logqL, logql, logDelta):
    """he_rs rides in the tail (1 <= log2 Delta <= 63; at 64 the call runs as two): the coefficients the streaming kernel flags are written
    unrescaled by the exact kernels and finished by bridge_rescale_masked.  The keys also carry r = half+1 with a quotient chosen from the
    addends of the first crafted ciphertext (whose b0 is sparse, so that d0 = a0 b0 is known in closed form) so that the sum sits on and next
    to the SECOND rounding's tie: a wrong first rounding flips the second.  In the single-pass rings the call runs as he_mul, then he_rs."""
    torch = _torch()
    g, o, dims, W, M = _setup(engine_ctx, oracle_ctx, logn, logqL, logql)
    n, ql = g.n, 1 << logql
    rng = random.Random(8000 + logn + logql + logDelta)
    cts = [[_centred(rng, logql, n) for _ in range(BATCH)] for _ in range(4)]
    for k in CRAFTED:
        cts[1][k], cts[3][k] = _one(n), _one(n)
    k = CRAFTED[0]                                         # d0 = a0 b0, d1 = a0 b1 + a1 b0 = a0 + b0 (src/he-mult.c:121-136 with a1 = b1 = 1)
    terms = {0: rng.randrange(-(ql // 2), ql // 2), rng.randrange(1, n - 1): rng.randrange(-(ql // 2), ql // 2), n - 1: -1}
    cts[2][k] = [terms.get(i, 0) for i in range(n)]
    d0 = wc.sparse_negacyclic(cts[0][k], terms, ql)
    d1 = [ref.mpi_smod(x + y, ql) for x, y in zip(cts[0][k], cts[2][k])]
    crafted = [wc.build(M, n, 41 + logDelta, rs=(logDelta, d0)), wc.build(M, n, 42 + logDelta, rs=(logDelta, d1))]
    _report("he_mul_rs n=2^%d q_l=2^%d Delta=2^%d" % (logn, logql, logDelta), crafted)
    rlk = [_key(o, c, dims[1]) for c in crafted]
    cts = [_dev(v, W) for v in cts]
    o0, o1 = torch.empty_like(cts[0]), torch.empty_like(cts[0])
    try:
        g.set_chunk(CHUNK)
        g.profile(True)
        g.profile_collect()
        g.he_mul_rs(o0, o1, *cts, rlk[0], rlk[1], W, logql, *dims, logDelta)
        torch.cuda.synchronize()
        prof = g.profile_collect()
    finally:
        g.profile(False)
        g.set_chunk(32)
    print("he_mul_rs kernels: %s" % sorted(prof))
    want = expect_all(he_mul_tasks(logn, logql, W, dims, cts, rlk, list(range(BATCH)), rs=logDelta))
    _compare("he_mul_rs", (o0, o1), want, W * n, keys=("rs0", "rs1"))
    # the closed-form addends are the reference's: its UNRESCALED he_mul output sits on and next to the second rounding's tie at the rs members
    for c, key in zip(crafted, ("c0", "c1")):
        unrescaled = words_to_ints(want[k][key], W, n)
        ties = [i for i, (name, _) in c.cls.items() if name in wc.RS_CLASSES]
        assert len(ties) >= 6
        for i in ties:
            target = ((1 << (logDelta - 1)) + wc.RS_CLASSES.index(c.cls[i][0]) - 1) % (1 << logDelta)
            assert unrescaled[i] % (1 << logDelta) == target, (key, i, c.cls[i])
    if logn > 12:
        assert "bridge_tail_stream" in prof, sorted(prof)
        if logDelta < 64:
            assert "bridge_rescale" not in prof, sorted(prof)  # the rescale rode in the tail; flagged coefficients: the masked rescale


def test_he_rot_hoisted_on_window_coefficients(engine_ctx, oracle_ctx):
    """c1 = 1 is its own rotation, so rotation r with the key NTT(X_r) hands the tail X_r; the addend is poly_rot(c0)"""
    from gpqhe_amd import big_to_ints, to_host
    torch = _torch()
    logn, logqL, logql = STREAM_SHAPES[0]
    g, o, dims, W, M = _setup(engine_ctx, oracle_ctx, logn, logqL, logql)
    n, (_, dimB, dimP) = g.n, dims
    rng = random.Random(9000)
    rots, batch = [1, 40, 5], 3
    crafted = [(wc.build(M, n, 51 + r), wc.build(M, n, 61 + r)) for r in rots]
    for r, c in zip(rots, crafted):
        _report("he_rot_hoisted rot %d" % r, c)
    hkeys = [tuple(o.ntt_slab(c.slab(o.p, dimB), dimB) for c in pair) for pair in crafted]
    from gpqhe_amd import to_device
    dkeys = [tuple(to_device(k) for k in pair) for pair in hkeys]
    c0 = [_centred(rng, logql, n) for _ in range(batch)]
    c1 = [_one(n), _centred(rng, logql, n), _one(n)]
    out0 = torch.empty(len(rots) * batch * W * n, dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    try:
        g.set_chunk(CHUNK)
        g.profile(True)
        g.profile_collect()
        g.he_rot_hoisted(out0, out1, _dev(c0, W), _dev(c1, W), rots, [k[0] for k in dkeys], [k[1] for k in dkeys], W, logql, dimB, dimP)
        torch.cuda.synchronize()
        prof = g.profile_collect()
    finally:
        g.profile(False)
        g.set_chunk(32)
    print("he_rot_hoisted kernels: %s" % sorted(prof))
    assert "bridge_tail_stream" in prof, sorted(prof)
    got0, got1 = big_to_ints(to_host(out0), W, n), big_to_ints(to_host(out1), W, n)
    for r, rot in enumerate(rots):
        for k in range(batch):
            x0, x1 = ref.he_swk(o, ref.poly_rot(c0[k], rot), ref.poly_rot(c1[k], rot), *hkeys[r], dimP, dimB, logql)
            assert got0[r * batch + k] == x0, "rotation by %d, ciphertext %d: c0" % (rot, k)
            assert got1[r * batch + k] == x1, "rotation by %d, ciphertext %d: c1" % (rot, k)


def test_a_wave_that_walks_several_groups(engine_ctx, oracle_ctx):
    """bridge_tail_stream is persistent: 256 blocks of 8 waves, wave w takes groups w, w + 2048, .. with the next group's first steps fetched
    while the current one is summed.  n = 2^13 and 9 ciphertexts in one launch group are 2 x 9 x 128 = 2304 groups: waves 0 .. 255 walk
    two.  Every ciphertext has d2 = 1 (a1 = b1 = 1) and the same keys, so every polynomial -- those of the groups walked last, after a
    prefetch, included -- carries the crafted coefficients; b0 is sparse, so the addends are known in closed form and the expected output is
    smod(rdiv(x, P) + d, q_l) on the chosen integers (window_cases.closed_form), cross-checked against ref.he_relin_tail on two polynomials."""
    from gpqhe_amd import big_to_ints, to_host
    torch = _torch()
    logn, logq, batch = 13, 438, 9
    g, o, dims, W, M = _setup(engine_ctx, oracle_ctx, logn, logq, logq)
    n, ql, (dimA, dimB, dimP) = g.n, 1 << logq, dims
    assert 2 * batch * (n // 64) > 8 * 256                 # more groups than waves (bridge_launch.hpp: kStreamBlocks, kStreamWaves)
    rng = random.Random(9100)
    crafted = [wc.build(M, n, 71), wc.build(M, n, 72)]
    _report("n=2^13 q=2^438, 2304 groups", crafted)
    rlk = [_key(o, c, dimB) for c in crafted]
    a0 = [_centred(rng, logq, n) for _ in range(batch)]
    terms = [{0: rng.randrange(-(ql // 2), ql // 2), rng.randrange(1, n): rng.randrange(-(ql // 2), ql // 2), n - 1: -1} for _ in range(batch)]
    b0 = [[t.get(i, 0) for i in range(n)] for t in terms]
    cts = [_dev(a0, W), _dev([_one(n)] * batch, W), _dev(b0, W), _dev([_one(n)] * batch, W)]
    try:
        g.profile(True)
        g.profile_collect()
        got = _he_mul(g, cts, rlk, W, logq, dims)
        prof = g.profile_collect()
    finally:
        g.profile(False)
    print("he_mul kernels: %s" % sorted(prof))
    assert prof["bridge_tail_stream"][1] == 1, sorted(prof)                                       # ONE launch over all 2304 groups
    got = [big_to_ints(to_host(t), W, n) for t in got]
    want = []
    for k in range(batch):
        d0 = wc.sparse_negacyclic(a0[k], terms[k], ql)
        d1 = [ref.mpi_smod(x + y, ql) for x, y in zip(a0[k], b0[k])]
        want.append((wc.closed_form(M, crafted[0].xs, d0, ql), wc.closed_form(M, crafted[1].xs, d1, ql), d0, d1))
    k = batch - 1                                          # the closed form against the restated tail, on c0 and c1 of the last ciphertext
    e0, e1 = ref.he_relin_tail(o, crafted[0].slab(o.p, dimB), crafted[1].slab(o.p, dimB), want[k][2], want[k][3], dimP, dimB, ql)
    assert e0 == want[k][0] and e1 == want[k][1]
    for k in range(batch):
        assert got[0][k] == want[k][0], "c0 of ciphertext %d" % k
        assert got[1][k] == want[k][1], "c1 of ciphertext %d" % k


@pytest.mark.parametrize("dim,logq", [(15, 438), (45, 850), (58, 1000)])
def test_plain_crt_fast_paths_across_their_window(engine_ctx, oracle_ctx, dim, logq):
    """gpq_rns_reconstruct: the fast paths cannot decide the centring of x within 2^-38 (matrix cores, 104 fraction bits) / 2^-61
    (bridge_reconstruct_low, 128 bits) below 1/2; x on the models' ladders across the window's lower edge and on half +- k"""
    from gpqhe_amd import big_to_ints, to_device, to_host
    torch = _torch()
    logn = 8
    g, o = engine_ctx(logn, 60), oracle_ctx(logn, 60)
    n, basis = g.n, ref.RnsBasis(o.p[:dim])
    rng = random.Random(dim)
    lad = wc.crt_ladder(wc.CrtModel(o.p, dim, 104, 38)) + wc.crt_ladder(wc.CrtModel(o.p, dim, 128, 61))
    assert len(lad) <= n // 4
    print("dim %d: %d ladder values, %d modelled inside a window" % (dim, len(lad), sum(1 for _, w in lad if w)))
    xs = [rng.randrange(basis.P) for _ in range(n)]
    for i, (x, _) in zip(wc.layout(n, len(lad), dim, dirty_groups=[0, n // 64 - 1]), lad):
        xs[i] = x
    slab = np.array([x % o.p[d] for d in range(dim) for x in xs], dtype=np.uint64)
    want = ref.poly_rns2mpi([slab[d * n:(d + 1) * n] for d in range(dim)], basis, 1 << logq)
    W = (logq + 63) // 64
    try:
        for mfma in (True, False):
            g.set_bridge_mfma(mfma)
            big = torch.empty(W * n, dtype=torch.int64, device="cuda")
            g.rns_reconstruct(big, W, to_device(slab), dim, logq)
            assert big_to_ints(to_host(big), W, n)[0] == want, "matrix cores" if mfma else "VALU"
    finally:
        g.set_bridge_mfma(True)
