"""The numpy model of the decoder (tests/dcd_model.py) against the EXECUTED reference's he_dcd above 8192 slots, and against its record.

Where oracle/_ref/ exists the model, on the table `roots_via_sincos` makes, must equal the reference bit for bit at 16384, 32768 and
65536 slots -- coefficients of 54-62 bits, the 54-bit patterns of mpi_to_double's rounding, one nu that is no power of two -- and
tests/golden/ref_dcd_big.json must be what the reference computes here.  On a bare checkout the model must reproduce the record wherever
this machine's table has the recorded digest.  tests/test_he_dcd_big_gpu.py then holds the device against the model.  No GPU."""
import numpy as np
import pytest

from tests import big_record, dcd_model
from tests.ref_jobs import require_reference


@pytest.fixture(scope="module")
def live():
    require_reference()
    return big_record.live_dcd()


@pytest.mark.parametrize("k", range(len(big_record.DCD_CASES)), ids=[big_record.dcd_name(c) for c in big_record.DCD_CASES])
def test_model_equals_the_executed_reference(live, k):
    case = big_record.DCD_CASES[k]
    got, exp = live[k], big_record.dcd_model_doubles(case)
    bad = np.argwhere(dcd_model.bits(got) != dcd_model.bits(exp))
    assert not len(bad), "case %s: %d doubles differ from the reference, first (plaintext, slot, part) %s" % (big_record.dcd_name(case), len(bad), bad[:3].tolist())


def test_stored_record_is_what_the_reference_computes(live):
    rec = {big_record.dcd_name(c): big_record.dcd_case_record(c, g, big_record.roots(c[1])) for c, g in zip(big_record.DCD_CASES, live)}
    assert rec == big_record.golden(big_record.DCD_JSON)["cases"], "tests/golden/ref_dcd_big.json is not what the executed reference computes: python -m tests.big_record rewrites it"


def test_inputs_hold_54_to_62_bits_every_pattern_and_a_general_nu():
    assert sum(1 for c in big_record.DCD_CASES if np.frexp(c[2])[0] != 0.5) == 1
    for case in big_record.DCD_CASES:
        logn, slots, nu = case
        p = big_record.dcd_plaintexts(case)
        gap, nh = (1 << logn) // 2 // slots, (1 << logn) // 2
        assert len(p) == big_record.COUNT and all(len(v) == 1 << logn for v in p)
        for k in (0, 2):
            assert all(54 <= abs(v).bit_length() <= 62 for v in p[k])
        read = [p[1][i * gap + h] for i in range(8) for h in (0, nh)]
        assert len(set(read)) == 8                                        # (M odd or even) x (b = 0 or 1) x both signs reach the decoder


def test_model_reproduces_the_stored_record_where_the_table_is_the_recorded_one():
    stored = big_record.golden(big_record.DCD_JSON)["cases"]
    assert sorted(stored) == sorted(big_record.dcd_name(c) for c in big_record.DCD_CASES)
    compared = 0
    for case in big_record.DCD_CASES:
        rec = stored[big_record.dcd_name(case)]
        assert (rec["logn"], rec["slots"], float.fromhex(rec["nu"]), rec["seed"]) == case + (big_record.dcd_seed(case),)
        if big_record.roots_sha(big_record.roots(case[1])) != rec["roots_sha256"]:
            continue                                                      # another libm: the record says nothing about this table
        assert big_record.sha_doubles(big_record.dcd_model_doubles(case)) == rec["sha256"], \
            "case %s: the model on the recorded table does not give the recorded doubles" % big_record.dcd_name(case)
        compared += 1
    print("cases compared with the record:", compared)
