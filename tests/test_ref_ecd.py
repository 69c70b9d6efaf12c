"""The numpy model of the encoder (tests/ecd_model.py) against the EXECUTED reference's he_ecd, and against its stored record.

Where oracle/_ref/ exists the model, on the table `roots_via_sincos` makes, must equal the reference word for word on every recorded case
and at 2048, 4096 and 8192 slots, and the stored record (tests/golden/ref_ecd.json, ref_ecd_roots512.npy) must be what the reference
computes here.  On a bare checkout the model on the STORED table must reproduce the stored record.  tests/test_he_ecd_gpu.py then holds the
device against the model on the stored table.  No GPU."""
import numpy as np
import pytest

from oracle import ref
from tests import ecd_model, ecd_record
from tests.ref_jobs import require_reference


@pytest.fixture(scope="module")
def live():
    require_reference()
    cases = [(c[0], c[1], c[2], ecd_record.case_vectors(c)) for c in ecd_record.CASES]
    cases += [(c[0], c[1], c[2], ecd_record.large_vectors(c)) for c in ecd_record.LARGE]
    return ref.run(ecd_record.ref_encode, cases, workers=6)


def test_model_equals_the_executed_reference(live):
    for case, got in zip(ecd_record.CASES, live):
        logn, slots, logDelta, W = case
        exp, offending = ecd_model.encode(ecd_record.case_vectors(case), ecd_model.roots_via_sincos(slots), 1 << logn, logDelta)
        assert offending == 0
        bad = np.argwhere(exp != got)
        assert not len(bad), "case %s: %d coefficients differ from the reference, first (vector, coefficient) %s" % (ecd_record.case_name(case), len(bad), bad[:3].tolist())


@pytest.mark.parametrize("k", range(len(ecd_record.LARGE)), ids=["slots%d" % c[1] for c in ecd_record.LARGE])
def test_model_equals_the_executed_reference_at_large_slot_counts(live, k):
    case = ecd_record.LARGE[k]
    logn, slots, logDelta = case
    got = live[len(ecd_record.CASES) + k]
    exp, offending = ecd_model.encode(ecd_record.large_vectors(case), ecd_model.roots_via_sincos(slots), 1 << logn, logDelta)
    assert offending == 0
    bad = np.argwhere(exp != got)
    assert not len(bad), "%d slots: %d coefficients differ from the reference, first %s" % (slots, len(bad), bad[:3].tolist())


def test_stored_record_is_what_the_reference_computes(live):
    rec = {ecd_record.case_name(c): ecd_record.case_record(c, g) for c, g in zip(ecd_record.CASES, live)}
    assert rec == ecd_record.ecd_golden()["cases"], "tests/golden/ref_ecd.json is not what the executed reference computes: python -m tests.ecd_record rewrites it"
    assert np.array_equal(ecd_record.stored_roots(), ecd_model.roots_via_sincos(ecd_record.ROOTS_SLOTS)), \
        "tests/golden/ref_ecd_roots512.npy is not this C library's sincos table"


def test_model_on_the_stored_table_reproduces_the_stored_record():
    """what a checkout without the reference has: the record and the table it was made with"""
    stored, T = ecd_record.ecd_golden()["cases"], ecd_record.stored_roots()
    assert sorted(stored) == sorted(ecd_record.case_name(c) for c in ecd_record.CASES)
    for case in ecd_record.CASES:
        w, offending = ecd_record.model_words(case, T)
        rec = stored[ecd_record.case_name(case)]
        assert offending == 0 and ecd_record.sha(w) == rec["sha256"], "case %s: the model on the stored table does not give the stored slab" % ecd_record.case_name(case)
        assert (rec["logn"], rec["slots"], rec["logDelta"], rec["W"], rec["seed"]) == case + (ecd_record.case_seed(case),)
        assert 56 <= rec["max_bits"] <= ecd_record.MAX_BITS


def test_a_fused_complex_product_changes_the_record():
    """the recorded inputs are large enough to see a contracted butterfly: with the real part of (dr + i di)(c + i s) evaluated as
    fma(dr, c, -(di s)) -- one exact product, one rounding -- coefficients of the 64-slot case change (small messages could not tell)"""
    from fractions import Fraction
    logn, slots, logDelta, W = case = (9, 64, 30, 7)
    z, T = ecd_record.case_vectors(case)[0], ecd_record.stored_roots()
    plain, _ = ecd_model.encode(z, T, 1 << logn, logDelta)
    fma_sub = lambda a, b, r: float(Fraction(a) * Fraction(b) - Fraction(r))          # round(a b - r), exactly
    re, im = [float(v) for v in z.real], [float(v) for v in z.imag]
    stride, pow5 = ecd_record.ROOTS_SLOTS // slots, [pow(5, j, 4 * slots) for j in range(slots // 2)]
    length = slots
    while length >= 2:                                                                   # src/canemb.c:64-77
        mid, idx_mod = length // 2, 4 * length
        for i in range(0, slots, length):
            for j in range(mid):
                c, s = T[(idx_mod - pow5[j] % idx_mod) * (4 * slots // idx_mod) * stride]
                dr, di = re[i + j] - re[i + j + mid], im[i + j] - im[i + j + mid]
                re[i + j], im[i + j] = re[i + j] + re[i + j + mid], im[i + j] + im[i + j + mid]
                re[i + j + mid], im[i + j + mid] = fma_sub(dr, float(c), di * float(s)), dr * float(s) + di * float(c)
        length //= 2
    perm = ecd_model.bit_reverse(slots)
    fused = ecd_model.c_round(np.array(re)[perm] / slots * 2.0 ** logDelta).astype(np.int64)
    gap = (1 << logn) // 2 // slots
    assert int((fused != plain[0, :(1 << logn) // 2:gap]).sum()) > slots // 8
