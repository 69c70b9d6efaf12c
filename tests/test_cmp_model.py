"""tests/cmp_model.py -- he_cmp / he_cmppt of src/he-algo.c:460-548 call for call -- pinned without a device:
  * the collapse of every additive chain, the he_add in front of a nested he_inv and he_cmppt's dense he_addpt included, into one sum and ONE
    mpi_smod: LazyOps against BigintOps at logn 7, q_L = 2^200, Delta = 2^20, word for word and bit for bit in nu and B, at the top level and
    two levels below it;
  * he_cmp_core's last bn = 1 - an is dead: dropping it changes no word;
  * gpq_he_cmp_rounds against the reference's double expression for alpha 1..52, -1 outside; gpq_he_cmp_depth and its overflow;
  * where oracle/_ref is built, the EXECUTED reference through its per-call he_* slots against both, at logn 13 / q = 2^200."""
import random

import pytest

from oracle import ref
from tests import algo_model as am
from tests import cmp_model as cm
from tests import ref_jobs
from tests.test_algo_model import centred, inputs, result

LOGN, LOGQ, LOGDELTA = 7, 200, 20
NU0, B0, NU1, B1 = 3.0 * 2 ** 20, 1234.5, 5.0 * 2 ** 20, 77.25
TOP = [(0, 0), (1, 0), (2, 0), (1, 1), (0, 2)]              # (1, 1): depth 8; (0, 2): depth 9, the deepest that fits 9 * 20 + 1 <= 200
DOWN2 = [(0, 0), (1, 0), (2, 0), (0, 1)]
CASES = [(0,) + c for c in TOP] + [(2,) + c for c in DOWN2]
IDS = ["%ddown-iter%d-t%d" % c for c in CASES]


@pytest.fixture(scope="module")
def small(oracle_ctx):
    from oracle import bigint_ref as br
    probe = oracle_ctx(LOGN, 12)
    o = oracle_ctx(LOGN, br.he_dims(LOGN, probe.p, LOGQ, LOGQ)[3])
    out = {}
    for down in (0, 2):
        ins = inputs(o, LOGN, LOGQ, LOGDELTA, 7, down)
        rng = random.Random(99 + down)
        n, logql = 1 << LOGN, LOGQ - down * LOGDELTA
        ins["ct2"] = (centred(rng, n, logql), centred(rng, n, logql))
        ins["dense"] = [rng.randrange(-(1 << (logql - 1)), 1 << (logql - 1)) for _ in range(n)]     # about logql bits
        ins["dense"][:3] = [(1 << (logql - 1)) - 1, -(1 << (logql - 1)), 0]
        ins["one"] = am.const_plaintext(n, am.const_int(1, LOGDELTA))
        out[down] = ins
    return o, out


def _both(o, ins, down, f):
    """f(ops, first input, second input) on BigintOps and LazyOps -> the two results and the LazyOps"""
    L = LOGQ // LOGDELTA
    Bmult = [1000.0 + 3 * l for l in range(L + 1)]
    got = []
    for cls in (cm.BigintOps, cm.LazyOps):
        ops = cls(o, LOGN, LOGQ, LOGDELTA, ins["rlk"], Bmult)
        out = f(ops, am.Ct(ins["ct"], L - down, NU0, B0), am.Ct(ins["ct2"], L - down, NU1, B1))
        got.append(result(ops, out) + (ops.logql(out.l),))
    return got[0], got[1], ops


@pytest.mark.parametrize("down,iter,t", CASES, ids=IDS)
def test_he_cmp_chains_collapse_into_one_smod(small, down, iter, t):
    o, ins = small
    want, lazy, ops = _both(o, ins[down], down, lambda ops, a, b: cm.he_cmp(ops, a, b, iter, t))
    assert want[1] == LOGQ // LOGDELTA - down - cm.depth(iter, t)
    h = 1 << (want[4] - 1)
    assert all(-h <= v < h for c in want[0] for v in c)
    assert lazy == want
    assert ops.most_terms >= 2                              # he_add's two terms went into one sum with he_inv's constant


@pytest.mark.parametrize("which", ["dense", "one"])
@pytest.mark.parametrize("down,iter,t", CASES, ids=IDS)
def test_he_cmppt_chains_collapse_into_one_smod(small, down, iter, t, which):
    o, ins = small
    pt_nu = float(1 << LOGDELTA) if which == "one" else 7.0 * 2 ** 20         # above NU0: pt->nu decides the maximum
    want, lazy, ops = _both(o, ins[down], down, lambda ops, a, b: cm.he_cmppt(ops, a, ins[down][which], pt_nu, iter, t))
    assert want[1] == LOGQ // LOGDELTA - down - cm.depth(iter, t)
    assert lazy == want
    if which == "one":                                      # he_const_pt(1) as a dense plaintext is he_addpt by the constant
        again, _, _ = _both(o, ins[down], down, lambda ops, a, b: _cmppt_const(ops, a, iter, t))
        assert again == want


def _cmppt_const(ops, ct, iter, t):
    an, out = ops.alloc(), ops.alloc()
    ops.addpt(an, ct, 1)
    cm.he_cmp_core(ops, an, ct, iter, t)
    ops.copy(out, an)
    return out


@pytest.mark.parametrize("iter,t", [(0, 0), (1, 1), (0, 2)])
def test_the_last_bn_is_dead(small, iter, t):
    o, ins = small
    full, lazy_full, _ = _both(o, ins[0], 0, lambda ops, a, b: cm.he_cmp(ops, a, b, iter, t))
    cut, lazy_cut, _ = _both(o, ins[0], 0, lambda ops, a, b: cm.he_cmp(ops, a, b, iter, t, dead_bn=False))
    assert full == cut == lazy_full == lazy_cut


def test_rounds_and_depth():
    from gpqhe_amd import _native
    lib = _native.load()
    table = [cm.rounds(a) for a in range(1, 53)]
    assert table[:8] == [0, 2, 4, 5, 6, 8, 9, 10] and table[-1] == 57
    assert [lib.gpq_he_cmp_rounds(a) for a in range(1, 53)] == table
    assert lib.gpq_he_cmp_rounds(0) == -1 and lib.gpq_he_cmp_rounds(53) == -1 and lib.gpq_he_cmp_rounds(0xFFFFFFFF) == -1
    for iter, t in TOP + [(7, 57), (4093, 0), (0, 1364), (1, 1023)]:           # 4096 levels at the most
        assert lib.gpq_he_cmp_depth(iter, t) == cm.depth(iter, t)
    for iter, t in [(4094, 0), (0, 1365), (1, 1024), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (0xFFFFFFFD, 0xFFFFFFFF), (65533, 65535)]:
        assert lib.gpq_he_cmp_depth(iter, t) == -1, (iter, t)
    # the five evaluators' two host functions do not know the comparison
    assert lib.gpq_he_algo_depth(5, 1) == -1


# ---------------------------------------------------------------------------
# the executed reference
# ---------------------------------------------------------------------------
REF_SHAPE = dict(logn=13, logq=200, slots=2)
REF_CASES = [("cmp", 1, 0, 30, 0), ("cmp", 0, 1, 20, 2), ("cmppt", 0, 0, 30, 0)]       # (function, iter, t, logDelta, levels below the top)


def reference_job(arg):
    """one comparison on the executed reference's per-call functions and on the restatement, same inputs: (reference, restatement, Lazy)"""
    fn, iter, t, logdelta, down = arg
    from oracle.oracle import OracleCtx
    logn, logq, slots = (REF_SHAPE[k] for k in ("logn", "logq", "slots"))
    R = ref.Ref().init(logn, 1 << logq, slots, 1 << logdelta)
    o = OracleCtx(logn, R.dimub)
    ins = inputs(o, logn, logq, logdelta, 13, down)
    rng = random.Random(17)
    n, logql = 1 << logn, logq - down * logdelta
    ct2 = (centred(rng, n, logql), centred(rng, n, logql))
    dense = [rng.randrange(-(1 << (logql - 1)), 1 << (logql - 1)) for _ in range(n)]
    R.evk_set("rlk", *ins["rlk"])
    L = R.Lmax - down
    Brs, Bmult = R.he_bounds()
    pt_nu = 7.0 * 2 ** logdelta
    out = []
    for ops in (cm.RefOps(R, logdelta), cm.BigintOps(o, logn, logq, logdelta, ins["rlk"], Bmult, Brs), cm.LazyOps(o, logn, logq, logdelta, ins["rlk"], Bmult, Brs)):
        a, b = am.Ct(ins["ct"], L, NU0, B0), am.Ct(ct2, L, NU1, B1)
        got = cm.he_cmp(ops, a, b, iter, t) if fn == "cmp" else cm.he_cmppt(ops, a, dense, pt_nu, iter, t)
        out.append(result(ops, got))
    return out


@pytest.fixture(scope="module")
def reference_results():
    ref_jobs.require_reference()
    return ref.run(reference_job, REF_CASES, workers=3)


@pytest.mark.parametrize("k", range(len(REF_CASES)), ids=["%s-iter%d-t%d-delta%d-%ddown" % c for c in REF_CASES])
def test_model_equals_the_executed_reference(reference_results, k):
    fn, iter, t, logdelta, down = REF_CASES[k]
    got, want, lazy = reference_results[k]
    assert got[1] == want[1] == REF_SHAPE["logq"] // logdelta - down - cm.depth(iter, t)
    for c in (0, 1):
        bad = [i for i, (x, y) in enumerate(zip(got[0][c], want[0][c])) if x != y]
        assert not bad, "c%d: %d coefficients differ, first at %s" % (c, len(bad), bad[:3])
    assert got[2] == want[2], "nu bits %016x vs %016x" % (got[2], want[2])
    assert got[3] == want[3], "B bits %016x vs %016x" % (got[3], want[3])
    assert lazy == want
