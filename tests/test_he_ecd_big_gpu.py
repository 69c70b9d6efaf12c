"""gpq_he_ecd on plans of more than one block: above 8192 slots, or forced by gpq_ecd_plan_set_block (kernels he_ecd_cols, he_ecd_block,
he_ecd_slab).  Every comparison is an equality of words.

* the recorded cases of tests/ecd_record.py with a forced split (k = 1, 2, 3; a gap of 64), on the stored table: the stored sha256 and
  the model, all six vectors in one call, and again after set_block(0);
* 16384, 32768 and 65536 slots on this machine's sincos table against the model, and against tests/golden/ref_ecd_big.json where that
  table has the recorded digest;
* coefficients without an image in different blocks, 32 words, batches of 1 and 5, the refusals, and one capture and replay."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpqhe_amd import GpqError, to_host
from tests import big_record, dcd_model, ecd_model, ecd_record

pytestmark = pytest.mark.gpu
POISON = int(np.array([0xA5A5DEADBEEF5A5A], dtype=np.uint64).view(np.int64)[0])
# (logn, slots) of ecd_record.CASES -> slots per workgroup
FORCED = {(9, 16): 8, (10, 512): 128, (9, 64): 8, (8, 128): 64, (13, 64): 16}


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


def test_set_block_exists_and_checks_its_argument(engine_ctx):
    g = engine_ctx(9, 2)
    T = ecd_record.stored_roots()
    with g.ecd_plan(64, T) as plan:
        for block in (2, 4, 3, 6, 128, 1):                                # 64 / block > 8, no power of two, above the slots, below 2
            with pytest.raises(GpqError):
                plan.set_block(block)
        for block in (8, 16, 32, 64, 0):
            plan.set_block(block)
    with g.ecd_plan(1, T) as plan:
        plan.set_block(0)
        with pytest.raises(GpqError):
            plan.set_block(1)


@pytest.mark.parametrize("case", [c for c in ecd_record.CASES if (c[0], c[1]) in FORCED], ids=ecd_record.case_name)
def test_a_forced_split_gives_the_recorded_words(engine_ctx, case):
    record, T = ecd_record.ecd_golden()["cases"], ecd_record.stored_roots()
    logn, slots, logDelta, W = case
    exp, offending = ecd_record.model_words(case, T)
    assert offending == 0 and ecd_record.sha(exp) == record[ecd_record.case_name(case)]["sha256"], "the model on the stored table is not the record"
    g = engine_ctx(logn, 2)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with g.ecd_plan(slots, T) as plan:
        if case == (9, 64, 30, 7):
            with pytest.raises(GpqError):                                 # 32 blocks
                plan.set_block(2)
        plan.set_block(FORCED[(logn, slots)])
        got = _encode(g, plan, ecd_record.case_vectors(case), logDelta, W, bad)
        _same(got, exp, "%s in blocks of %d" % (ecd_record.case_name(case), FORCED[(logn, slots)]))
        assert ecd_record.sha(got) == record[ecd_record.case_name(case)]["sha256"] and int(bad.item()) == 0
        plan.set_block(0)
        _same(_encode(g, plan, ecd_record.case_vectors(case), logDelta, W, bad), exp, "%s after set_block(0)" % ecd_record.case_name(case))
    assert int(bad.item()) == 0


def test_a_forced_split_gathers_the_diagonals_of_a_matrix(engine_ctx):
    logn, slots, logDelta, W = 9, 16, 30, 2
    g, T = engine_ctx(logn, 2), ecd_record.stored_roots()
    rng = np.random.default_rng(16)
    A = 2.0 ** 30 * (rng.uniform(-1, 1, (slots, slots)) + 1j * rng.uniform(-1, 1, (slots, slots)))
    coeffs, offending = ecd_model.encode(ecd_model.diagonal_vectors(A), T, g.n, logDelta)
    out = torch.full((slots * W * g.n,), POISON, dtype=torch.int64, device="cuda")
    with g.ecd_plan(slots, T) as plan:
        g.he_ecd_diagonals(plan.set_block(4), out, _dev(A), logDelta, W)
        torch.cuda.synchronize()
    assert offending == 0
    _same(to_host(out).reshape(slots, W, g.n), ecd_model.words(coeffs, W), "diagonals in blocks of 4")


@pytest.mark.parametrize("case", big_record.ECD_CASES, ids=big_record.ecd_name)
def test_real_sizes_equal_the_model_and_the_record(engine_ctx, case):
    logn, slots, logDelta, W = case
    coeffs, offending = big_record.ecd_model_coeffs(case)
    exp = ecd_model.words(coeffs, W)
    g = engine_ctx(logn, 2)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with g.ecd_plan(slots, big_record.roots(slots), block=0) as plan:
        got = _encode(g, plan, big_record.ecd_vectors(case), logDelta, W, bad)
    _same(got, exp, big_record.ecd_name(case))
    assert offending == 0 and int(bad.item()) == 0
    rec = big_record.golden(big_record.ECD_JSON)["cases"][big_record.ecd_name(case)]
    if big_record.roots_sha(big_record.roots(slots)) == rec["roots_sha256"]:
        assert big_record.sha_words(got) == rec["sha256"], "the device's slab is not the executed reference's"


@pytest.mark.parametrize("logn,slots,block", [(15, 16384, 0), (16, 32768, 4096)])
def test_encode_then_decode_on_the_device_is_model_encode_then_model_decode(engine_ctx, logn, slots, block):
    case = [c for c in big_record.ECD_CASES if c[:2] == (logn, slots)][0]
    logDelta, W = case[2], 2
    coeffs, _ = big_record.ecd_model_coeffs(case)
    exp = dcd_model.decode([[int(v) for v in p] for p in coeffs], big_record.roots(slots), slots, 2.0 ** logDelta)
    g = engine_ctx(logn, 2)
    count = coeffs.shape[0]
    slab = torch.full((count * W * g.n,), POISON, dtype=torch.int64, device="cuda")
    out = torch.from_numpy(np.full(count * slots * 2, 0xFFF8DEADBEEF5A5A, dtype=np.uint64).view(np.int64)).to("cuda")
    with g.ecd_plan(slots, big_record.roots(slots), block=0) as plan:
        plan.set_block(block)
        g.he_ecd(plan, slab, _dev(big_record.ecd_vectors(case)), logDelta, W)
        g.he_dcd(plan, out.view(torch.float64), slab, 2.0 ** logDelta, W)
        torch.cuda.synchronize()
    got = to_host(out).view(np.float64).reshape(count, slots, 2)
    differ = np.argwhere(dcd_model.bits(got) != dcd_model.bits(exp))
    assert not len(differ), "%d doubles differ, first (vector, slot, part) %s" % (len(differ), differ[0].tolist())


def test_coefficients_without_an_image_in_different_blocks(engine_ctx):
    """Vector 0 is canemb of a coefficient vector with 1.5 * 2^63 at slot 5 (real part) and -2^64 at slot 8 (imaginary part): the slots
    i with the same i mod 2 share a block, so the two lie in different blocks, and they are the only coefficients of the vector without
    an image.  (No input gives exactly one NaN coefficient: every coefficient is a sum over all slots.)  Vector 1 holds one NaN slot, so
    none of its 2 slots coefficients has an image.  Vector 2 is an ordinary neighbour."""
    case = big_record.ECD_CASES[0]
    logn, slots, logDelta, W = case
    T, g = big_record.roots(slots), engine_ctx(logn, 2)
    rng = np.random.default_rng(63)
    x = 2.0 ** (40 - logDelta) * (rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots))
    x[5] = 1.5 * 2.0 ** (63 - logDelta) + x[5].imag * 1j
    x[8] = x[8].real - 2.0 ** (64 - logDelta) * 1j
    re, im = dcd_model.canemb(x.real, x.imag, T)
    z = np.zeros((3, slots), dtype=np.complex128)
    z[0] = re[0] + 1j * im[0]
    z[1] = big_record.ecd_vectors(case)[1]
    z[1, 12345] = complex(np.nan, np.nan)
    z[2] = big_record.ecd_vectors(case)[0]
    coeffs, offending = ecd_model.encode(z, T, g.n, logDelta)
    alone = [ecd_model.encode(z[k], T, g.n, logDelta)[1] for k in range(3)]
    assert alone == [2, 2 * slots, 0] and offending == 2 + 2 * slots
    assert coeffs[0, 5] == 0 and coeffs[0, 8 + g.n // 2] == 0 and int((coeffs[0] != 0).sum()) == 2 * slots - 2
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with g.ecd_plan(slots, T, block=0) as plan:
        got = _encode(g, plan, z, logDelta, W, bad)
    assert int(bad.item()) == offending
    _same(got, ecd_model.words(coeffs, W), "range")
    assert not got[0, :, 5].any() and not got[0, :, 8 + g.n // 2].any() and not got[1].any()
    _same(got[2:], ecd_model.words(big_record.ecd_model_coeffs(case)[0][:1], W), "the neighbour")


def test_32_words_and_batches_of_one_and_five(engine_ctx):
    case = big_record.ECD_CASES[0]
    logn, slots, logDelta, _ = case
    g = engine_ctx(logn, 2)
    coeffs, _ = big_record.ecd_model_coeffs(case)
    z = big_record.ecd_vectors(case)
    with g.ecd_plan(slots, big_record.roots(slots), block=0) as plan:
        _same(_encode(g, plan, z[1], logDelta, 32), ecd_model.words(coeffs[1:2], 32), "one vector of 32 words")
        order = [2, 0, 1, 1, 0]
        _same(_encode(g, plan, z[order], logDelta, 1), ecd_model.words(coeffs[order], 1), "five vectors")


def test_refusals_launch_nothing(engine_ctx):
    g, other = engine_ctx(15, 2), engine_ctx(15, 6)
    slots, W = 16384, 1
    z = _dev(np.ones((1, slots)))
    out = torch.full((W * g.n + 2,), POISON, dtype=torch.int64, device="cuda")
    o, zz, s = C.c_void_p(out.data_ptr()), C.c_void_p(z.data_ptr()), g._stream()
    g.profile(True)
    try:
        for refused in (g.n, 3 << 12, 2 * g.n, 0):                        # slots = n, no power of two
            with pytest.raises(GpqError):
                g.ecd_plan(refused, block=0)
        with pytest.raises(GpqError):                                     # 16 blocks
            g.ecd_plan(slots, block=1024)
        with pytest.raises(GpqError):                                     # gpq_ecd_plan_create itself keeps one workgroup's limit
            g.ecd_plan(slots)
        with other.ecd_plan(slots, block=0) as foreign, g.ecd_plan(slots, block=0) as plan:
            assert g.lib.gpq_he_ecd(g.h, foreign.h, o, zz, 30, W, 1, None, s) == -1       # a plan of another context
            assert g.lib.gpq_he_ecd(g.h, plan.h, C.c_void_p(out.data_ptr() + 8), zz, 30, W, 1, None, s) == -1   # out not 16-byte aligned
            assert g.lib.gpq_he_ecd(g.h, plan.h, o, zz, 30, 33, 1, None, s) == -1
            assert g.lib.gpq_he_ecd(g.h, plan.h, o, zz, 30, W, 0, None, s) == -1
            A = _dev(np.ones(4))
            assert g.lib.gpq_he_ecd_diagonals(g.h, plan.h, o, C.c_void_p(A.data_ptr()), 30, W, None, s) == -1   # a 16384 x 16384 matrix
            with pytest.raises(GpqError):
                g.gemv_plan_from_matrix(plan, A, Delta=2.0 ** 30, logql=120, dimpt=3)
        assert g.profile_collect() == {}
    finally:
        g.profile(False)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_one_capture_and_replay_after_a_warm_call(engine_ctx):
    case = big_record.ECD_CASES[0]
    logn, slots, logDelta, W = case
    g = engine_ctx(logn, 2)
    exp = ecd_model.words(big_record.ecd_model_coeffs(case)[0], W)
    z = _dev(big_record.ecd_vectors(case))
    out = torch.full((exp.size,), POISON, dtype=torch.int64, device="cuda")
    with g.ecd_plan(slots, big_record.roots(slots), block=0) as plan:
        g.he_ecd(plan, out, z, logDelta, W)                                # the warm call: the hand-off memory of this shape
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g.he_ecd(plan, out, z, logDelta, W)
        out.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        _same(to_host(out).reshape(exp.shape), exp, "replay")
        del graph
