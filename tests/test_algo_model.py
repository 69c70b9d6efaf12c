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


def inputs(o, logn, logq, logdelta, seed):
    from oracle import bigint_ref as br
    n = 1 << logn
    rng = random.Random(seed)
    dimevk = br.he_dims(logn, o.p, logq, logq)[3]
    return dict(ct=(centred(rng, n, logq), centred(rng, n, logq)), rlk=(o.gen(seed * 100 + 1, dimevk), o.gen(seed * 100 + 2, dimevk)),
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


def reference_job(arg):
    """one evaluator on the executed reference's per-call functions and on the restatement, same inputs: (reference, restatement, Lazy)"""
    kind, iter = arg
    from oracle.oracle import OracleCtx
    logn, logq, logdelta, slots = (REF_SHAPE[k] for k in ("logn", "logq", "logdelta", "slots"))
    R = ref.Ref().init(logn, 1 << logq, slots, 1 << logdelta)
    o = OracleCtx(logn, R.dimub)
    ins = inputs(o, logn, logq, logdelta, 11)
    R.evk_set("rlk", *ins["rlk"])
    L = R.Lmax
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
