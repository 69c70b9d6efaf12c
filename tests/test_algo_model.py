"""tests/algo_model.py -- the five evaluators of src/he-algo.c:131-458 call for call -- pinned without a device:
  * on the restated reference (oracle/bigint_ref.py) at logn 7, q_L = 2^200, Delta = 2^30: levels, and the collapse of every additive chain
    (he_copy_ct, he_neg, he_add, he_addpt, he_subpt, he_moddown) into one sum and ONE mpi_smod -- LazyOps against BigintOps, word for word and
    bit for bit in nu and B;
  * where oracle/_ref is built, against the EXECUTED reference through its per-call he_* slots, with ct_get's l, nu and B.  The reference caps q
    by ring (src/precomp.c:53-64): q = 2^200 needs logn 13."""
import random

import pytest

from oracle import ref
from tests import algo_model as am
from tests import ref_jobs

LOGN, LOGQ, LOGDELTA = 7, 200, 30
NU0, B0 = 3.0 * 2 ** 30, 1234.5
CASES = [("inv", 1), ("inv", 2), ("sqrt", 1), ("sqrt", 2), ("sigmoid", 0), ("log", 0), ("exp", 1), ("exp", 2)]


def centred(rng, n, logq):
    h = 1 << (logq - 1)
    v = [rng.randrange(-h, h) for _ in range(n)]
    v[:6] = [0, -1, h - 1, -h, 1, -(h - 1)]
    return v


def inputs(o, logn, logq, logdelta, seed, down=0):
    """a ciphertext centred mod q_l, l = L - down, a key for q_L and he_exp's plaintext"""
    from oracle import bigint_ref as br
    n = 1 << logn
    rng = random.Random(seed)
    dimevk = br.he_dims(logn, o.p, logq, logq)[3]
    logql = logq - down * logdelta
    return dict(ct=(centred(rng, n, logql), centred(rng, n, logql)), rlk=(o.gen(seed * 100 + 1, dimevk), o.gen(seed * 100 + 2, dimevk)),
                m=[rng.randrange(-(1 << logdelta), 1 << logdelta) for _ in range(n)])


def result(ops, out):
    c = ops.value(out)
    return (list(c[0]), list(c[1])), out.l, ref.bits(out.nu), ref.bits(out.B)


@pytest.fixture(scope="module")
def small(oracle_ctx):
    from oracle import bigint_ref as br
    probe = oracle_ctx(LOGN, 12)
    o = oracle_ctx(LOGN, br.he_dims(LOGN, probe.p, LOGQ, LOGQ)[3])
    return o, inputs(o, LOGN, LOGQ, LOGDELTA, 7)


@pytest.mark.parametrize("kind,iter", CASES)
def test_additive_chains_collapse_into_one_smod(small, kind, iter):
    o, ins = small
    L = LOGQ // LOGDELTA
    Bmult = [1000.0 + 3 * l for l in range(L + 1)]                    # any table: both sides read the same one
    got = []
    for cls in (am.BigintOps, am.LazyOps):
        ops = cls(o, LOGN, LOGQ, LOGDELTA, ins["rlk"], Bmult)
        out = am.run(kind, ops, am.Ct(ins["ct"], L, NU0, B0), iter, ins["m"])
        got.append(result(ops, out))
        assert out.l == L - am.depth(kind, iter)
        h = 1 << (ops.logql(out.l) - 1)
        assert all(-h <= v < h for c in got[-1][0] for v in c)           # in mpi_smod's range at the output's level
    assert got[0] == got[1]
    assert ops.most_terms >= (3 if kind in ("sigmoid", "exp") else 1)   # the closing sums really were deferred


_SHAPE_INPUTS = {}
SHAPE_CASES = [(cell, kind, iter) for cell, shape in am.SLAB_SHAPES.items() for kind, iter in shape[6]]


@pytest.mark.parametrize("cell,kind,iter", SHAPE_CASES, ids=["%s-%s-%d" % c for c in SHAPE_CASES])
def test_additive_chains_collapse_at_every_slab_shape(oracle_ctx, cell, kind, iter):
    """the same, below the top level, at other scales and bases: the shapes tests/test_he_algo_shapes_gpu.py runs the library at"""
    from oracle import bigint_ref as br
    logn, logq, logdelta, down = am.SLAB_SHAPES[cell][:4]
    if cell not in _SHAPE_INPUTS:
        probe = oracle_ctx(logn, am.primes_for(logn, logq))
        o = oracle_ctx(logn, br.he_dims(logn, probe.p, logq, logq)[3])
        _SHAPE_INPUTS[cell] = o, inputs(o, logn, logq, logdelta, 7, down)
    o, ins = _SHAPE_INPUTS[cell]
    L = logq // logdelta
    Bmult = [1000.0 + 3 * l for l in range(L + 1)]
    got = []
    for cls in (am.BigintOps, am.LazyOps):
        ops = cls(o, logn, logq, logdelta, ins["rlk"], Bmult)
        assert ops.logql(L - down) == logq - down * logdelta
        out = am.run(kind, ops, am.Ct(ins["ct"], L - down, NU0, B0), iter, ins["m"])
        got.append(result(ops, out))
        assert out.l == L - down - am.depth(kind, iter)
        h = 1 << (ops.logql(out.l) - 1)
        assert all(-h <= v < h for c in got[-1][0] for v in c)
    assert got[0] == got[1]
    assert ops.most_terms >= (3 if kind in ("sigmoid", "exp") else 1) and ops.sums >= 1
    if cell == "D" and kind == "sigmoid":
        # Delta = 2^4: he_const_pt of -1/48, -17/80640 and 31/1451520 is 0, every product by them is 0, and what is left is he_const_pt(1/2)
        assert [am.const_int(re, logdelta) for re in (-1. / 48, -17. / 80640, 31. / 1451520)] == [0, 0, 0]
        n = 1 << logn
        assert got[0][0] == ([am.const_int(0.5, logdelta)] + [0] * (n - 1), [0] * n)


def test_constants_are_he_const_pts():
    """round half away from zero of re * Delta, exactly (src/he-encode.c:119-125)"""
    assert am.const_int(0.5, 1) == 1 and am.const_int(-0.5, 1) == -1 and am.const_int(0.25, 1) == 1 and am.const_int(-0.25, 1) == -1
    assert am.const_int(0.125, 2) == 1 and am.const_int(0.124, 2) == 0
    assert am.const_int((1. / 4) / (-1. / 48), 30) == -12 << 30
    assert am.const_int(1. / 9., 50) == round(1. / 9. * 2 ** 50)
    assert [am.depth(k, 3) for k in am.KINDS] == [4, 6, 4, 4, 7]


# ---------------------------------------------------------------------------
# the executed reference
# ---------------------------------------------------------------------------
REF_SHAPE = dict(logn=13, logq=200, logdelta=30, slots=2)
REF_CASES = [("inv", 2), ("sqrt", 1), ("sigmoid", 0), ("log", 0), ("exp", 1)]


# ... and below the top level, at other scales: (kind, iter, logDelta, levels below the top)
REF_CASES_AT = [("inv", 1, 20, 2), ("log", 0, 20, 3), ("sqrt", 1, 59, 0), ("exp", 0, 30, 2), ("inv", 1, 59, 0)]


def reference_job(arg):
    """one evaluator on the executed reference's per-call functions and on the restatement, same inputs: (reference, restatement, Lazy)"""
    kind, iter = arg[:2]
    from oracle.oracle import OracleCtx
    logn, logq, logdelta, slots = (REF_SHAPE[k] for k in ("logn", "logq", "logdelta", "slots"))
    down = 0
    if len(arg) == 4:
        logdelta, down = arg[2:]
    R = ref.Ref().init(logn, 1 << logq, slots, 1 << logdelta)
    o = OracleCtx(logn, R.dimub)
    ins = inputs(o, logn, logq, logdelta, 11, down)
    R.evk_set("rlk", *ins["rlk"])
    assert R.Lmax == logq // logdelta
    L = R.Lmax - down
    Brs, Bmult = R.he_bounds()
    m = None
    if kind == "exp":
        a = complex(0.75, 0) / (1 << iter)                            # src/he-algo.c:444
        R.he_ecd(1, [a] * slots)
        m = R.pt_get(1)[0]
    out = []
    for ops in (am.RefOps(R, logdelta), am.BigintOps(o, logn, logq, logdelta, ins["rlk"], Bmult, Brs), am.LazyOps(o, logn, logq, logdelta, ins["rlk"], Bmult, Brs)):
        out.append(result(ops, am.run(kind, ops, am.Ct(ins["ct"], L, NU0, B0), iter, m)))
    return out


@pytest.fixture(scope="module")
def reference_results():
    ref_jobs.require_reference()
    return ref.run(reference_job, REF_CASES, workers=8)


@pytest.mark.parametrize("k", range(len(REF_CASES)), ids=["%s-%d" % c for c in REF_CASES])
def test_model_equals_the_executed_reference(reference_results, k):
    kind, iter = REF_CASES[k]
    got, want, lazy = reference_results[k]
    assert got[1] == want[1] == REF_SHAPE["logq"] // REF_SHAPE["logdelta"] - am.depth(kind, iter)
    for c in (0, 1):
        bad = [i for i, (x, y) in enumerate(zip(got[0][c], want[0][c])) if x != y]
        assert not bad, "c%d: %d coefficients differ, first at %s" % (c, len(bad), bad[:3])
    assert got[2] == want[2], "nu bits %016x vs %016x" % (got[2], want[2])
    assert got[3] == want[3], "B bits %016x vs %016x" % (got[3], want[3])
    assert lazy == want


@pytest.fixture(scope="module")
def reference_results_at():
    ref_jobs.require_reference()
    return ref.run(reference_job, REF_CASES_AT, workers=8)


@pytest.mark.parametrize("k", range(len(REF_CASES_AT)), ids=["%s-%d-delta%d-%ddown" % c for c in REF_CASES_AT])
def test_model_equals_the_executed_reference_below_the_top_and_at_other_scales(reference_results_at, k):
    kind, iter, logdelta, down = REF_CASES_AT[k]
    got, want, lazy = reference_results_at[k]
    assert got[1] == want[1] == REF_SHAPE["logq"] // logdelta - down - am.depth(kind, iter)
    for c in (0, 1):
        bad = [i for i, (x, y) in enumerate(zip(got[0][c], want[0][c])) if x != y]
        assert not bad, "c%d: %d coefficients differ, first at %s" % (c, len(bad), bad[:3])
    assert got[2] == want[2], "nu bits %016x vs %016x" % (got[2], want[2])
    assert got[3] == want[3], "B bits %016x vs %016x" % (got[3], want[3])
    assert lazy == want
