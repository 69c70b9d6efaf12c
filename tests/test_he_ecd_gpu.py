"""gpq_he_ecd / gpq_he_ecd_diagonals: he_ecd (src/he-encode.c:53-64, :107-111; src/canemb.c:62-81) on the device.

* word for word against the record of the EXECUTED reference (tests/golden/ref_ecd.json): the device and the numpy model
  (tests/ecd_model.py) both read the stored root table, so this machine's libm plays no part; the model's slab must have the recorded
  sha256 and the device's slab must be the model's.  The output is poisoned first: a word the call should have zeroed shows up.
* a batch of 67 vectors against the same vectors one by one; the capacity edge (8192 slots); the range rules (2^63, infinity, the bad
  counter, a Delta that is no power of two); the diagonals of a matrix gathered by the kernel against the model's zrotdiag vectors."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpqhe_amd import GpqError, to_host
from tests import ecd_model, ecd_record

pytestmark = pytest.mark.gpu
POISON = int(np.array([0xA5A5DEADBEEF5A5A], dtype=np.uint64).view(np.int64)[0])


def _dev(z):
    return torch.from_numpy(np.ascontiguousarray(z, dtype=np.complex128)).to("cuda")


def _encode(g, plan, z, logDelta, W, bad=None):
    """[count][W][n] uint64 of one gpq_he_ecd call on a poisoned output"""
    z = np.array(z, dtype=np.complex128, ndmin=2)
    out = torch.full((z.shape[0] * W * g.n,), POISON, dtype=torch.int64, device="cuda")
    g.he_ecd(plan, out, _dev(z), logDelta, W, bad)
    torch.cuda.synchronize()
    return to_host(out).reshape(z.shape[0], W, g.n)


def _same(got, exp, what):
    bad = np.argwhere(got != exp)
    assert not len(bad), "%s: %d words differ, first (vector, word, coefficient) %s: %#x vs %#x" % (
        what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(exp[tuple(bad[0])]))


@pytest.fixture(scope="module")
def stored():
    return ecd_record.ecd_golden()["cases"], ecd_record.stored_roots()


@pytest.mark.parametrize("case", ecd_record.CASES, ids=ecd_record.case_name)
def test_words_equal_the_record_of_the_executed_reference(engine_ctx, stored, case):
    record, T = stored
    logn, slots, logDelta, W = case
    exp, offending = ecd_record.model_words(case, T)
    assert offending == 0 and ecd_record.sha(exp) == record[ecd_record.case_name(case)]["sha256"], "the model on the stored table is not the record"
    g = engine_ctx(logn, 2)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with g.ecd_plan(slots, T) as plan:
        got = _encode(g, plan, ecd_record.case_vectors(case), logDelta, W, bad)
    _same(got, exp, ecd_record.case_name(case))
    assert int(bad.item()) == 0
    assert int((got[:, 0] != 0).sum()) >= 2 * slots                      # (not degenerate: the uniform vector alone fills 2 slots coefficients)


def test_a_batch_equals_its_vectors_one_by_one(engine_ctx, stored):
    _, T = stored
    logn, slots, logDelta, W, count = 9, 16, 20, 2, 67
    g = engine_ctx(logn, 2)
    rng = np.random.default_rng(67)
    scale = 2.0 ** rng.integers(-20, 41, size=(count, 1))
    z = scale * (rng.uniform(-1, 1, (count, slots)) + 1j * rng.uniform(-1, 1, (count, slots)))
    with g.ecd_plan(slots, T) as plan:
        got = _encode(g, plan, z, logDelta, W)
        single = np.concatenate([_encode(g, plan, z[k], logDelta, W) for k in range(count)])
    _same(got, single, "batch of %d" % count)
    coeffs, offending = ecd_model.encode(z, T, g.n, logDelta)
    assert offending == 0
    _same(got, ecd_model.words(coeffs, W), "batch against the model")


def test_capacity_edge_8192_slots(engine_ctx):
    logn, slots, logDelta = ecd_record.LARGE[-1]
    assert slots == 8192 and slots == (1 << logn) // 2
    g = engine_ctx(logn, 2)
    T = ecd_model.roots_via_sincos(slots)                                 # the same table on both sides
    z = ecd_record.large_vectors(ecd_record.LARGE[-1])[:1]
    coeffs, offending = ecd_model.encode(z, T, g.n, logDelta)
    assert offending == 0
    with g.ecd_plan(slots, T) as plan:
        _same(_encode(g, plan, z, logDelta, 1), ecd_model.words(coeffs, 1), "8192 slots")
    with pytest.raises(GpqError):                                         # one workgroup's LDS holds no more
        engine_ctx(15, 2).ecd_plan(2 * slots)


def test_range_2_63_and_infinity_are_zero_and_counted(engine_ctx, stored):
    record, T = stored
    case = (9, 16, 20, 2)
    logn, slots, logDelta, W = case
    g = engine_ctx(logn, 2)
    ordinary = ecd_record.case_vectors(case)
    z = np.zeros((4, slots), dtype=np.complex128)
    z[0] = 2.0 ** (63 - logDelta)                                         # a constant vector: coefficient 0 is exactly 2^63, the others 0
    z[1], z[2] = ordinary[0], ordinary[2]
    z[3] = ordinary[0]
    z[3, 5] = complex(np.inf, 1.0)
    coeffs, offending = ecd_model.encode(z, T, g.n, logDelta)
    alone = [ecd_model.encode(z[k], T, g.n, logDelta)[1] for k in range(4)]
    assert alone[0] == 1 and alone[1] == alone[2] == 0 and alone[3] >= slots and offending == sum(alone)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with g.ecd_plan(slots, T) as plan:
        got = _encode(g, plan, z, logDelta, W, bad)
        below = _encode(g, plan, np.full(slots, 2.0 ** (63 - logDelta) - 2.0 ** (10 - logDelta)), logDelta, W)   # the largest double below 2^63
    assert int(bad.item()) == offending
    _same(got, ecd_model.words(coeffs, W), "range")
    assert not got[0].any(), "the coefficient of 2^63 is stored as 0"
    assert int(below[0, 0, 0]) == 2 ** 63 - 1024 and int(below[0, 1, 0]) == 0
    # the neighbours are their record
    whole, _ = ecd_record.model_words(case, T)
    assert ecd_record.sha(whole) == record[ecd_record.case_name(case)]["sha256"]
    _same(got[1:3], whole[[0, 2]], "neighbours of the offending vectors")


def test_a_delta_that_is_no_power_of_two_is_refused(engine_ctx, stored):
    _, T = stored
    g = engine_ctx(9, 6)
    slots = 4
    z = _dev(np.ones((1, slots)))
    A = _dev(np.ones((slots, slots)))
    out = torch.full((2 * g.n,), POISON, dtype=torch.int64, device="cuda")
    with g.ecd_plan(slots, T) as plan:
        g.profile(True)
        try:
            for delta in (3.0 * 2 ** 29, 1e9, 2.0 ** 30 + 1):
                with pytest.raises(GpqError):
                    g.gemv_plan_from_matrix(plan, A, Delta=delta, logql=120, dimpt=3)
                with pytest.raises(GpqError):
                    g.he_ecd(plan, out, z, Delta=delta, W=2)
            assert g.lib.gpq_he_ecd(g.h, plan.h, C.c_void_p(out.data_ptr()), C.c_void_p(z.data_ptr()), 64, 2, 1, None, g._stream()) == -1   # no 64-bit Delta
            assert g.profile_collect() == {}                              # nothing was launched
        finally:
            g.profile(False)
        torch.cuda.synchronize()
        assert bool((out == POISON).all())
        g.gemv_plan_from_matrix(plan, A, Delta=2.0 ** 30, logql=120, dimpt=3).close()


@pytest.mark.parametrize("slots", [4, 8, 16])
def test_diagonals_of_a_matrix_equal_the_encoded_zrotdiag_vectors(engine_ctx, stored, slots):
    _, T = stored
    logn, logDelta, W = 9, 30, 2
    g = engine_ctx(logn, 2)
    n1, n2 = ecd_model.gemv_steps(slots)
    assert (n1, n2) == {4: (2, 2), 8: (4, 2), 16: (4, 4)}[slots]          # 8: the non-square split
    rng = np.random.default_rng(slots)
    A = 2.0 ** 30 * (rng.uniform(-1, 1, (slots, slots)) + 1j * rng.uniform(-1, 1, (slots, slots)))   # coefficients of 60 bits
    zero = slots // 2 + 1
    A[np.arange(slots), (np.arange(slots) + zero) % slots] = 0           # diagonal `zero` is all zero
    vectors = ecd_model.diagonal_vectors(A)
    assert not vectors[zero].any() and all(vectors[k].any() for k in range(slots) if k != zero)
    out = torch.full((slots * W * g.n,), POISON, dtype=torch.int64, device="cuda")
    with g.ecd_plan(slots, T) as plan:
        g.he_ecd_diagonals(plan, out, _dev(A), logDelta, W)
        torch.cuda.synchronize()
        got = to_host(out).reshape(slots, W, g.n)
        _same(got, _encode(g, plan, vectors, logDelta, W), "%d slots" % slots)
    assert not got[zero].any() and all(got[k].any() for k in range(slots) if k != zero)
    coeffs, offending = ecd_model.encode(vectors, T, g.n, logDelta)
    assert offending == 0
    _same(got, ecd_model.words(coeffs, W), "%d slots against the model" % slots)
