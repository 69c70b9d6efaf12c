"""The numpy model of the encoder (tests/ecd_model.py) against the EXECUTED reference's he_ecd above 8192 slots, and against its record.

Where oracle/_ref/ exists the model, on the table `roots_via_sincos` makes, must equal the reference word for word at 16384, 32768 and
65536 slots (and at 16384 slots with gap = 2), and tests/golden/ref_ecd_big.json must be what the reference computes here.  On a bare
checkout the model must reproduce the record wherever this machine's table has the recorded digest; the record holds no table.  The
inputs are large enough to see a contracted butterfly: the uniform vectors' largest coefficients have 58-62 bits.
tests/test_he_ecd_big_gpu.py then holds the device against the model.  No GPU."""
import numpy as np
import pytest

from tests import big_record, ecd_model
from tests.ref_jobs import require_reference


@pytest.fixture(scope="module")
def live():
    require_reference()
    return big_record.live_ecd()


@pytest.mark.parametrize("k", range(len(big_record.ECD_CASES)), ids=[big_record.ecd_name(c) for c in big_record.ECD_CASES])
def test_model_equals_the_executed_reference(live, k):
    case = big_record.ECD_CASES[k]
    exp, offending = big_record.ecd_model_coeffs(case)
    assert offending == 0
    bad = np.argwhere(exp != live[k])
    assert not len(bad), "case %s: %d coefficients differ from the reference, first (vector, coefficient) %s" % (big_record.ecd_name(case), len(bad), bad[:3].tolist())


def test_stored_record_is_what_the_reference_computes(live):
    rec = {big_record.ecd_name(c): big_record.ecd_case_record(c, g, big_record.roots(c[1])) for c, g in zip(big_record.ECD_CASES, live)}
    assert rec == big_record.golden(big_record.ECD_JSON)["cases"], "tests/golden/ref_ecd_big.json is not what the executed reference computes: python -m tests.big_record rewrites it"


def test_inputs_reach_58_to_62_bits_and_the_tie():
    """a condition on the inputs, asserted on the model's coefficients as the record asserts it on the reference's"""
    for case in big_record.ECD_CASES:
        logn, slots, logDelta, W = case
        coeffs, offending = big_record.ecd_model_coeffs(case)
        assert offending == 0
        for k in range(2):
            assert big_record.MIN_BITS <= ecd_model.max_bits(coeffs[k]) <= big_record.MAX_BITS, big_record.ecd_name(case)
        # the constant vector: coefficient 0 is round(2.5) = 3 and coefficient n/2 round(-1.5) = -2, half away from zero
        assert int(coeffs[2, 0]) == 3 and int(coeffs[2, (1 << logn) // 2]) == -2


def test_model_reproduces_the_stored_record_where_the_table_is_the_recorded_one():
    """what a checkout without the reference has: the record, and this machine's table if its digest is the recorded one"""
    stored = big_record.golden(big_record.ECD_JSON)["cases"]
    assert sorted(stored) == sorted(big_record.ecd_name(c) for c in big_record.ECD_CASES)
    compared = 0
    for case in big_record.ECD_CASES:
        rec = stored[big_record.ecd_name(case)]
        assert (rec["logn"], rec["slots"], rec["logDelta"], rec["W"], rec["seed"]) == case + (big_record.ecd_seed(case),)
        assert all(big_record.MIN_BITS <= b <= big_record.MAX_BITS for b in rec["max_bits"])
        if big_record.roots_sha(big_record.roots(case[1])) != rec["roots_sha256"]:
            continue                                                      # another libm: the record says nothing about this table
        coeffs, offending = big_record.ecd_model_coeffs(case)
        assert offending == 0 and big_record.sha_words(ecd_model.words(coeffs, case[3])) == rec["sha256"], \
            "case %s: the model on the recorded table does not give the recorded slab" % big_record.ecd_name(case)
        compared += 1
    print("cases compared with the record:", compared)
