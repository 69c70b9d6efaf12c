"""Whole functions: the restatement (oracle/bigint_ref.py around the C oracle) against the EXECUTED reference, coefficient for coefficient.

`ref.which()` is the build compared with: the reference as it is where the loaded libgcrypt floor-divides negative dividends
correctly, the build that routes mpi_fdiv through oracle_fdiv otherwise.  On a library with the defect the as-is build is compared
as well, with bigint_ref.mpi_rdiv monkeypatched to the defect's rule -- so the one difference between the reference as such a machine
runs it and the restatement is that one sign, measured.

Shapes stay inside what the reference accepts: on logn 10..15 it caps q (src/precomp.c:53-64, :338-350) and its chain holds
dimub = (1 + logn + 4 logqub) / 59 + 1 primes and no more.  Inputs: seeded centred coefficients that include 0, -1, q/2 - 1, -q/2;
all-max same-sign ciphertexts (the worst carry into mpi_rdiv's tie); one ciphertext squared (ct1 == ct2, the same object).
l and the bits of nu and B are compared everywhere; where B holds Bmult[l] (a long double product of the reference's bounds table) the
formula is evaluated with the reference's own table, read through the driver.  One he_mul has its destination aliasing both operands."""
import random

import pytest

from oracle import bigint_ref as br
from oracle import ref
from tests import ref_jobs
from tests.test_libgcrypt_pin import _moduli

ALL = ["he_add", "he_mulpt", "he_mul", "he_moddown", "he_rot", "he_gemv"]
SHAPES = [
    dict(logn=8, logq=120, logdelta=30, slots=1, seed=1),
    dict(logn=8, logq=120, logdelta=30, slots=8, seed=2),
    dict(logn=9, logq=120, logdelta=30, slots=16, seed=3),
    dict(logn=9, logq=90, logdelta=30, slots=2, seed=4, kind="max"),
    dict(logn=8, logq=177, logdelta=59, slots=2, seed=5, kind="min"),
    dict(logn=10, logq=27, logdelta=17, slots=2, seed=6),
    dict(logn=10, logq=27, logdelta=17, slots=16, seed=7, only=["he_add", "he_mulpt", "he_rot", "he_gemv"]),
    dict(logn=12, logq=100, logdelta=25, slots=2, seed=8),
    dict(logn=12, logq=100, logdelta=25, slots=8, seed=9, kind="max", only=["he_mul", "he_rot", "he_moddown"]),
    dict(logn=13, logq=200, logdelta=40, slots=2, seed=10, only=["he_add", "he_mulpt", "he_mul", "he_moddown", "he_rot"]),
    dict(logn=13, logq=200, logdelta=40, slots=1, seed=11, only=["he_gemv"]),
    # the reference's default shape, single calls
    dict(logn=14, logq=438, logdelta=50, slots=16, seed=12, only=["he_mul"]),
    dict(logn=14, logq=438, logdelta=50, slots=16, seed=13, only=["he_rot"]),
]
_id = lambda a: "logn%d-q%d-D%d-s%d-%s%s" % (a["logn"], a["logq"], a["logdelta"], a["slots"], a.get("kind", "random"), "-" + "+".join(a["only"]) if a.get("only") else "")


@pytest.fixture(scope="module")
def results():
    ref_jobs.require_reference()
    return ref.run(ref_jobs.check_functions, SHAPES, workers=8)


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[_id(a) for a in SHAPES])
def test_functions_equal_the_executed_reference(results, k):
    a, r = SHAPES[k], results[k]
    assert r["diffs"] == []
    ran = set(r["names"])
    for name in a.get("only", ALL):
        assert any(x == name or x.startswith(name) for x in ran), "%s did not run" % name
    if "he_mul" in a.get("only", ALL):
        assert {"he_mul", "he_rs", "he_rs_ties", "he_square", "he_square_in_place"} <= ran
    if "he_rot" in a.get("only", ALL):
        assert {"he_rot %d" % a["slots"], "he_rot %d" % (a["slots"] + 3), "he_conj"} <= ran      # rot >= slots: he_rot indexes rk[rot] and does not bound it
    if "he_gemv" in a.get("only", ALL):
        assert {"he_gemv", "he_sum", "he_idx"} <= ran


def test_gemv_steps_and_diagonal_order():
    """n1, n2 of src/he-algo.c:51-54, and which diagonal meets which rotation: diagonal k = i n1 + j is rotated back by the giant step i n1"""
    assert [br.gemv_steps(s) for s in (1, 2, 4, 8, 16, 32, 64)] == [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]
    from gpqhe_amd import gemv_steps
    assert all(gemv_steps(s) == br.gemv_steps(s) for s in (1, 2, 4, 8, 16, 32, 64, 128))
    slots = 8
    A = list(range(slots * slots))
    assert ref_jobs.zrotdiag(A, slots, 0, 0) == [A[i * slots + i] for i in range(slots)]
    assert ref_jobs.zrotdiag(A, slots, 5, -4) == [A[((i - 4) % slots) * slots + (i + 1) % slots] for i in range(slots)]


@pytest.mark.parametrize("logn,logq,slots", [(3, 61, 2), (7, 61, 8), (9, 120, 16), (10, 27, 4), (12, 100, 8), (13, 200, 16), (16, 120, 64)])
def test_polynomial_level_equals_the_executed_reference(logn, logq, slots):
    ref_jobs.require_reference()
    diffs, = ref.run(ref_jobs.check_poly, [(logn, logq, slots, 50 + logn)], workers=1)
    assert diffs == []


# ---------------------------------------------------------------------------
# the floor-division defect: measured, not argued
# ---------------------------------------------------------------------------
def _dividends(golden, count_per_modulus):
    rng = random.Random(11)
    cases = []
    for m in _moduli(golden):
        h = m // 2
        vals = [0, 1, -1, h, -h, h + 1, -h - 1, m, -m, m + h, -(m + h), -(m + h) - 1, -(m + h) + 1, 7 * m + h + 1, -(7 * m + h + 1), -1000503, 1000503]
        for _ in range(count_per_modulus):
            v = rng.randrange(0, m << rng.choice([1, 10, 80]))
            vals += [v, -v]
        cases.append((vals, m))
    return cases


def test_oracle_fdiv_and_the_defects_rule(golden):
    """oracle_fdiv == Python's divmod on dividends of both signs (also with the quotient aliasing the dividend and a NULL remainder, the two
    call shapes of the reference), == gcry_mpi_div(.., -1) on the non-negative half; the as-is build's mpi_rdiv == the defect's rule on a
    library with the defect and == the restatement on one without; the _floor build's mpi_rdiv == the restatement everywhere."""
    ref_jobs.require_reference()
    cases = _dividends(golden, 350)
    assert sum(len(v) for v, _ in cases) >= 10000
    out, = ref.run(ref_jobs.division, [cases], workers=1)
    floor = ref.run(ref_jobs.floor_build_rdiv, cases, workers=8)
    native = ref.floor_is_native()
    lost = 0
    for (vals, m), r, fl in zip(cases, out, floor):
        want = [divmod(v, m) for v in vals]
        assert r["ofdiv"] == want
        assert [q for q, _ in r["ofdiv_alias"]] == [q for q, _ in want]
        assert [g for g, v in zip(r["gcry"], vals) if v >= 0] == [w for w, v in zip(want, vals) if v >= 0]
        if native:
            assert r["rdiv_noalias"] == [br.mpi_rdiv(v, m) for v in vals]
            # with the quotient aliasing the dividend the library takes the sign for its adjustment from the overwritten operand: for
            # -m < a < 0 what a correct library returns there is not known here, so that window is left out on such a library
            assert [g for g, v in zip(r["rdiv"], vals) if not -m < v < 0] == [br.mpi_rdiv(v, m) for v in vals if not -m < v < 0]
        else:
            assert r["rdiv_noalias"] == [ref_jobs.defect_rdiv_noalias(v, m) for v in vals]
            assert r["rdiv"] == [ref_jobs.defect_rdiv(v, m) for v in vals]
        assert fl == [br.mpi_rdiv(v, m) for v in vals]
        lost += sum(1 for v, g in zip(vals, r["rdiv"]) if g != br.mpi_rdiv(v, m))
    assert (lost == 0) if native else (lost > 3000)


DEFECT_SHAPES = [dict(logn=8, logq=120, logdelta=30, slots=2, seed=21, only=["he_mul", "he_rot"], build=ref.AS_IS),
                 dict(logn=9, logq=90, logdelta=30, slots=4, seed=22, only=["he_mul", "he_rot"], build=ref.AS_IS)]


@pytest.mark.parametrize("k", range(len(DEFECT_SHAPES)))
def test_as_is_build_equals_the_restatement_with_the_defects_rule(monkeypatch, k):
    """he_mul, he_rs, he_rot of the reference AS THIS MACHINE RUNS IT.  With a correct libgcrypt that is the restatement itself; with the
    defect it is the restatement with mpi_rdiv swapped for the defect's rule -- and differs from the unpatched restatement."""
    ref_jobs.require_reference()
    a = DEFECT_SHAPES[k]
    got, = ref.run(ref_jobs.functions_run, [a], workers=1)
    plain = ref_jobs.compare_functions(got, ref_jobs.functions_expected(a, got["_ctx"], got))
    if ref.floor_is_native():
        assert plain == []
        return
    assert any(d.startswith("he_mul c") for d in plain) and any(d.startswith("he_rs c") for d in plain) and any(d.startswith("he_rot") for d in plain)
    monkeypatch.setattr(br, "mpi_rdiv", ref_jobs.defect_rdiv)
    assert ref_jobs.compare_functions(got, ref_jobs.functions_expected(a, got["_ctx"], got)) == []
