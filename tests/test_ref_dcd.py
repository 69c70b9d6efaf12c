"""The numpy model of the decoder (tests/dcd_model.py) against the EXECUTED reference's he_dcd, and against its stored record.

Where oracle/_ref/ exists the model, on the table `roots_via_sincos` makes, must equal the reference bit for bit on every recorded case
and at 2048, 4096 and 8192 slots, its closed form of mpi_to_double must be the reference's function, and the stored record
(tests/golden/ref_dcd.json with ref_ecd_roots512.npy) must be what the reference computes here.  On a bare checkout the model on the
STORED table must reproduce the stored record.  tests/test_he_dcd_gpu.py then holds the device against the model on the stored table.
The last four tests show that the recorded inputs would have caught a decoder that rounds differently.  No GPU."""
import random
from fractions import Fraction

import numpy as np
import pytest

from oracle import ref
from tests import dcd_model, dcd_record
from tests.ecd_model import roots_via_sincos
from tests.ref_jobs import require_reference


@pytest.fixture(scope="module")
def live():
    require_reference()
    cases = [(c[0], c[1], c[3], dcd_record.case_plaintexts(c)) for c in dcd_record.CASES]
    cases += [(c[0], c[1], c[3], dcd_record.large_plaintexts(c)) for c in dcd_record.LARGE]
    return ref.run(dcd_record.ref_decode, cases, workers=6)


def _same(got, exp, what):
    bad = np.argwhere(dcd_model.bits(got) != dcd_model.bits(exp))
    assert not len(bad), "%s: %d doubles differ from the reference, first (plaintext, slot, part) %s: %r vs %r" % (
        what, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(exp[tuple(bad[0])]))


def test_model_equals_the_executed_reference(live):
    for case, got in zip(dcd_record.CASES, live):
        _same(dcd_record.model_doubles(case, roots_via_sincos(case[1])), got, "case %s" % dcd_record.case_name(case))


@pytest.mark.parametrize("k", range(len(dcd_record.LARGE)), ids=["slots%d" % c[1] for c in dcd_record.LARGE])
def test_model_equals_the_executed_reference_at_large_slot_counts(live, k):
    case = dcd_record.LARGE[k]
    logn, slots, W, nu = case
    exp = dcd_model.decode(dcd_record.large_plaintexts(case), roots_via_sincos(slots), slots, nu)
    _same(exp, live[len(dcd_record.CASES) + k], "%d slots" % slots)


def test_closed_form_of_mpi_to_double_is_the_reference_function():
    require_reference()
    rng = random.Random(53)
    values = [rng.getrandbits(b) | (1 << (b - 1)) for b in [rng.randint(1, 1100) for _ in range(1500)]]
    values += [(1 << 53) + d for d in (-1, 0, 1, 2, 3)] + [(1 << 1024) - 1, (1 << 1024) - (1 << 970), ((1 << 54) - 1) << 970, ((1 << 53) - 1) << 971, 0]
    values = values + [-v for v in values]
    got, = ref.run(dcd_record.ref_to_double, [values], workers=1)
    exp = np.array([dcd_model.mpi_to_double(v) for v in values])
    assert np.array_equal(dcd_model.bits(got), dcd_model.bits(exp))
    nearest = np.array([float(v) if abs(v).bit_length() <= 1024 and abs(v) < (1 << 1024) - (1 << 970) else np.nan for v in values])
    assert int((np.isfinite(nearest) & (nearest != exp)).sum()) > 100          # (it is NOT round-to-nearest)
    assert np.isinf(exp).any() and np.isinf(dcd_model.mpi_to_double(((1 << 54) - 1) << 970))


def test_stored_record_is_what_the_reference_computes(live):
    rec = {dcd_record.case_name(c): dcd_record.case_record(c, g) for c, g in zip(dcd_record.CASES, live)}
    assert rec == dcd_record.dcd_golden()["cases"], "tests/golden/ref_dcd.json is not what the executed reference computes: python -m tests.dcd_record rewrites it"
    assert np.array_equal(dcd_record.stored_roots(), roots_via_sincos(dcd_record.ROOTS_SLOTS)), \
        "tests/golden/ref_ecd_roots512.npy is not this C library's sincos table"


@pytest.fixture(scope="module")
def recorded():
    """the model on the stored table, once per case: what the variants below are compared with"""
    T = dcd_record.stored_roots()
    return T, {c: dcd_record.model_doubles(c, T) for c in dcd_record.CASES}


def test_model_on_the_stored_table_reproduces_the_stored_record(recorded):
    """what a checkout without the reference has: the record and the table it was made with"""
    T, model = recorded
    stored = dcd_record.dcd_golden()["cases"]
    assert sorted(stored) == sorted(dcd_record.case_name(c) for c in dcd_record.CASES)
    for case in dcd_record.CASES:
        rec = stored[dcd_record.case_name(case)]
        assert np.isfinite(model[case]).all()
        assert dcd_record.sha(model[case]) == rec["sha256"], "case %s: the model on the stored table does not give the stored doubles" % dcd_record.case_name(case)
        assert (rec["logn"], rec["slots"], rec["W"], float.fromhex(rec["nu"]), rec["seed"]) == case + (dcd_record.case_seed(case),)


def _changed(recorded, cases, **variant):
    T, model = recorded
    return sum(int((dcd_model.bits(dcd_record.model_doubles(c, T, **variant)) != dcd_model.bits(model[c])).sum()) for c in cases)


def test_a_round_to_nearest_conversion_changes_the_record(recorded):
    """b = 1 with M even and lower bits set: nearest rounds up, the reference's bit loop does not"""
    assert _changed(recorded, dcd_record.CASES, to_double=dcd_model.to_double_nearest) > 0


def test_a_truncating_conversion_changes_the_record(recorded):
    """b = 1 with M odd: the reference's bit loop rounds up, truncation does not"""
    assert _changed(recorded, dcd_record.CASES, to_double=dcd_model.to_double_truncating) > 0


def test_a_fused_complex_product_changes_the_record(recorded):
    """the real part of (br + i bi)(c + i s) as fma(br, c, -(bi s)): one exact product, one rounding"""
    def fused(br, bi, c, s):
        q = np.multiply(bi, s)
        cc = np.broadcast_to(c, br.shape)
        out = np.empty_like(br)
        for idx in np.ndindex(br.shape):
            out[idx] = float(Fraction(float(br[idx])) * Fraction(float(cc[idx])) - Fraction(float(q[idx])))      # round(a b - r), exactly
        return out
    assert _changed(recorded, [(9, 16, 2, 3.0 * 2 ** 29 + 1), (9, 64, 7, 2.0 ** 30)], real_part=fused) > 0


def test_a_product_with_the_reciprocal_changes_the_record(recorded):
    """x * (1 / nu) in place of x / nu, where nu is no power of two"""
    assert len(dcd_record.NOT_POW2) == 2
    for case in dcd_record.NOT_POW2:
        assert _changed(recorded, [case], quotient=lambda x, nu: np.multiply(x, np.divide(1.0, nu))) > 0
