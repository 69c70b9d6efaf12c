"""Tables: polyctx_init / hectx_init of the EXECUTED reference against the restatement, word for word.

For every logn 1..17 and two moduli each: dimub, the whole prime chain, pinv_mont / pinv_barr / ninv of every prime, every word of
zetas / zetas_inv, phat_invmp and P of every prefix -- against oracle.OracleCtx, the dimub formula (orc_dimub, the twin of gpq_dimub)
and bigint_ref.RnsBasis.  hectx_init: dim, dimevk, L and q[l] against bigint_ref.he_dims for every (logn, log q_L, log Delta) the
tests and bench.py use that the reference accepts (on logn 10..15 it caps q: src/precomp.c:53-64, :338-350)."""
import pytest

from oracle import bigint_ref as br
from oracle import ref
from oracle.oracle import lib
from tests import ref_jobs

CAP = {10: 27, 11: 54, 12: 109, 13: 218, 14: 438, 15: 881}          # the reference's own bound on log q (128-bit classical)
# two moduli per ring; inside 10..15 at or below the cap
POLY = [(logn, logq) for logn in range(1, 10) for logq in (61, 120)] + \
       [(10, 27), (10, 20), (11, 54), (11, 30), (12, 109), (12, 60), (13, 218), (13, 100), (14, 438), (14, 200), (15, 881), (15, 590),
        (16, 850), (16, 100), (17, 835), (17, 61)]
# (logn, log q_L, log Delta, slots): headline and default shapes of bench.py / README, the shapes of the GPU tests the reference accepts,
# and the shapes tests/test_ref_functions.py runs
HE = [(16, 850, 50, 8), (14, 438, 50, 16), (15, 881, 50, 8), (17, 835, 50, 8), (8, 120, 30, 8), (9, 120, 30, 16), (7, 61, 20, 2), (9, 240, 30, 1),
      (10, 27, 17, 2), (11, 54, 18, 4), (12, 100, 25, 2), (12, 109, 20, 1), (13, 200, 40, 2), (13, 218, 21, 4), (16, 120, 30, 64), (16, 850, 30, 64),
      (8, 59, 30, 1), (8, 58, 29, 2), (8, 177, 59, 4)]


@pytest.fixture(scope="module")
def poly_tables():
    ref_jobs.require_reference()
    return dict(zip(POLY, ref.run(ref_jobs.tables, POLY, workers=8)))


@pytest.fixture(scope="module")
def he_tables():
    ref_jobs.require_reference()
    return dict(zip(HE, ref.run(ref_jobs.hectx, HE, workers=8)))


@pytest.mark.parametrize("logn,logq", POLY)
def test_polyctx_tables(poly_tables, oracle_ctx, logn, logq):
    t = poly_tables[(logn, logq)]
    logqub = CAP.get(logn, logq)
    assert t["logqub"] == logqub
    assert t["dimub"] == (1 + logn + 4 * logqub) // 59 + 1 == lib().orc_dimub(logn, logqub)
    o = oracle_ctx(logn, t["dimub"])
    n = 1 << logn
    assert [nd["p"] for nd in t["nodes"]] == o.p
    for d, nd in enumerate(t["nodes"]):
        p = nd["p"]
        for name in ("pinv_mont", "pinv_barr", "ninv"):
            assert nd[name] == o.const(name, d), (d, name)
        assert nd["pinv_mont"] * p % (1 << 64) == 1 and nd["pinv_barr"] == (1 << 120) // p and nd["ninv"] == pow(n, -1, p) * (1 << 64) % p
        assert t["zeta_diffs"][d] == (0, 0), "prime %d: words of zetas / zetas_inv that differ" % d
        psi = o.const("psi", d)
        assert t["psi_R"][d] == (psi * (1 << 64) % p, pow(psi, -1, p) * (1 << 64) % p)
        assert pow(psi, n, p) == p - 1                                # a primitive 2n-th root
    for d in range(t["dimub"]):
        basis = br.RnsBasis(o.p[:d + 1])
        assert t["prefix"][d] == (basis.phat_invmp, basis.P), "prefix of %d primes" % (d + 1)


@pytest.mark.parametrize("logn,logq,logdelta,slots", HE)
def test_hectx_tables(he_tables, oracle_ctx, logn, logq, logdelta, slots):
    t = he_tables[(logn, logq, logdelta, slots)]
    o = oracle_ctx(logn, t["dimub"])
    assert t["primes"] == o.p
    L = logq // logdelta                                              # ceil() of an integer quotient, src/precomp.c:391
    assert t["L"] == L
    assert t["q"] == [1 << (logq - (L - l) * logdelta) for l in range(L + 1)]
    dimP, dimA, dimB, dimevk = br.he_dims(logn, o.p, logq, logq)
    assert (t["dim"], t["dimevk"]) == (dimP, dimevk)
    P = br.RnsBasis(o.p[:dimP]).P
    assert (t["P"], t["PqL"]) == (P, P << logq)
    assert dimB == dimevk
    # on a standard ring at its cap the reference's own chain can be SHORTER than its dimevk (logn 11, q = 2^54: 4 primes, dimevk 5):
    # there its he_relin walks off the chain; the driver refuses such calls and tests/test_ref_functions.py picks shapes with room
    assert (dimevk <= t["dimub"]) == ((logn, logq) not in ((11, 54),))


def test_headline_shape_is_the_readmes(he_tables, golden):
    t = he_tables[(16, 850, 50, 8)]
    assert (len(t["primes"]), t["dim"], t["dimevk"], t["L"]) == (58, 15, 45, 17)
    rec = golden["context_dims"]["16_850_50"]
    assert (t["L"], t["dim"], t["dimevk"], t["dimub"], t["P"].bit_length(), t["PqL"].bit_length()) == \
           (rec["L"], rec["dim"], rec["dimevk"], rec["dimub"], rec["nbits_P"], rec["nbits_PqL"])
    rec = golden["context_dims"]["14_438_50"]
    t = he_tables[(14, 438, 50, 16)]
    assert (t["L"], t["dim"], t["dimevk"], t["dimub"]) == (rec["L"], rec["dim"], rec["dimevk"], rec["dimub"])


def test_the_cap_comes_back_as_an_error_not_an_abort():
    ref_jobs.require_reference()
    assert ref.run(ref_jobs.over_the_cap, [(10, 28), (12, 120), (15, 882)]) == [-2, -2, -2]

