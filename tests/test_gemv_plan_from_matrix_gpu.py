"""gpq_gemv_plan_create_from_matrix: the plan made from the slots x slots matrix on the device (diagonals encoded there into a one-word
slab) against gpq_gemv_plan_create on the diagonals the numpy model (tests/ecd_model.py) encodes on the host -- the same plan (dim, live,
exact, rotations) and, through gpq_he_gemv_planned, the same words.  Keys and ciphertexts are those of tests/test_he_gemv_planned_gpu.py.
A matrix with a coefficient out of range leaves no plan."""
import numpy as np
import pytest
import torch

from gpqhe_amd import GpqError, to_device
from tests import ecd_model, ecd_record
from tests.test_he_gemv_planned_gpu import LOGDELTA, Shape, _same

pytestmark = pytest.mark.gpu
SLOTS, BATCH, LOGQ = 16, 3, 120


def _matrix(seed):
    """entries of magnitude <= 1 (30-bit coefficients, like Shape's diagonals); diagonal 6 is all zero"""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (SLOTS, SLOTS)) + 1j * rng.uniform(-1, 1, (SLOTS, SLOTS))
    A[np.arange(SLOTS), (np.arange(SLOTS) + 6) % SLOTS] = 0
    return A


@pytest.mark.parametrize("logn", [9, 13], ids=["logn9", "logn13-two-pass"])
def test_plan_from_matrix_equals_plan_from_model_encoded_diagonals(engine_ctx, logn):
    sh = Shape(engine_ctx, logn, LOGQ, SLOTS, BATCH)
    g, T, A = sh.g, ecd_record.stored_roots(), _matrix(logn)
    coeffs, offending = ecd_model.encode(ecd_model.diagonal_vectors(A), T, sh.n, LOGDELTA)
    assert offending == 0 and 28 <= ecd_model.max_bits(coeffs) <= 31
    diag = to_device(ecd_model.words(coeffs, sh.W).reshape(-1))
    A_dev = torch.from_numpy(A).to("cuda")
    c0, c1 = sh.ciphertexts()
    with g.ecd_plan(SLOTS, T) as ecd, g.gemv_plan(diag, SLOTS, sh.W, LOGQ, sh.dimpt) as host_plan, \
            g.gemv_plan_from_matrix(ecd, A_dev, LOGDELTA, LOGQ, sh.dimpt) as dev_plan:
        for name in ("dim", "live", "exact", "bytes", "diag_bits"):
            assert getattr(dev_plan, name) == getattr(host_plan, name), name
        assert dev_plan.exact and dev_plan.live == SLOTS - 1
        assert dev_plan.rotations() == host_plan.rotations() and sum(dev_plan.rotations()) >= sh.n1
        got = sh.planned(dev_plan, c0, c1)
        _same(got, sh.planned(host_plan, c0, c1), "logn %d" % logn)
    assert bool(got[0].any()) and bool(got[1].any())


def test_a_coefficient_out_of_range_leaves_no_plan(engine_ctx):
    sh = Shape(engine_ctx, 9, LOGQ, SLOTS, 1)
    A = _matrix(1)
    A[3, 4] = 2.0 ** 40                                                   # times Delta = 2^30: beyond 2^63
    with sh.g.ecd_plan(SLOTS, ecd_record.stored_roots()) as ecd:
        with pytest.raises(GpqError, match="2\\^63"):
            sh.g.gemv_plan_from_matrix(ecd, torch.from_numpy(A).to("cuda"), LOGDELTA, LOGQ, sh.dimpt)
