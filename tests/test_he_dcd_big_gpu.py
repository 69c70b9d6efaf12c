"""gpq_he_dcd on plans of more than one block: above 8192 slots, or forced by gpq_ecd_plan_set_block (kernels he_dcd_block, he_dcd_cols).
Every comparison is an equality of the 64-bit patterns of the doubles.

* the recorded cases of tests/dcd_record.py with a forced split (k = 1, 2, 3) on the stored table: the stored sha256 and the model, all
  eight plaintexts in one call, and again after set_block(0);
* 16384, 32768 and 65536 slots (and 16384 slots with gap = 2) with one and two words on this machine's sincos table against the model,
  and against tests/golden/ref_dcd_big.json where that table has the recorded digest;
* a batch of five, a plan of another context."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpqhe_amd import GpqError, to_host
from tests import big_record, dcd_model, dcd_record

pytestmark = pytest.mark.gpu
POISON_BITS = 0xFFF8DEADBEEF5A5A                                          # a NaN with a payload: compared as bits only
FORCED = {(9, 16): 8, (10, 512): 128, (9, 64): 8, (8, 128): 64}          # (logn, slots) of dcd_record.CASES -> slots per workgroup
REAL = big_record.DCD_CASES + [(16, 16384, 1e9)]                          # the last: gap = 2, model only


def _poisoned(count, slots):
    return torch.from_numpy(np.full(count * slots * 2, POISON_BITS, dtype=np.uint64).view(np.int64)).to("cuda")


def _decode(g, plan, words, nu, W):
    """[count][slots][2] float64 of one gpq_he_dcd call on a poisoned output"""
    count = words.shape[0]
    out = _poisoned(count, plan.slots)
    g.he_dcd(plan, out.view(torch.float64), torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1)).to("cuda"), nu, W)
    torch.cuda.synchronize()
    return to_host(out).view(np.float64).reshape(count, plan.slots, 2)


def _same(got, exp, what):
    bad = np.argwhere(dcd_model.bits(got) != dcd_model.bits(exp))
    assert not len(bad), "%s: %d doubles differ, first (plaintext, slot, part) %s: %r vs %r" % (
        what, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(exp[tuple(bad[0])]))


@pytest.mark.parametrize("case", [c for c in dcd_record.CASES if (c[0], c[1]) in FORCED], ids=dcd_record.case_name)
def test_a_forced_split_gives_the_recorded_doubles(engine_ctx, case):
    record, T = dcd_record.dcd_golden()["cases"], dcd_record.stored_roots()
    logn, slots, W, nu = case
    exp = dcd_record.model_doubles(case, T)
    assert dcd_record.sha(exp) == record[dcd_record.case_name(case)]["sha256"], "the model on the stored table is not the record"
    g = engine_ctx(logn, 2)
    words = dcd_model.words(dcd_record.case_plaintexts(case), W)
    with g.ecd_plan(slots, T) as plan:
        if (logn, slots) == (9, 64):
            with pytest.raises(GpqError):                                 # 32 blocks
                plan.set_block(2)
        plan.set_block(FORCED[(logn, slots)])
        got = _decode(g, plan, words, nu, W)
        _same(got, exp, "%s in blocks of %d" % (dcd_record.case_name(case), FORCED[(logn, slots)]))
        assert dcd_record.sha(got) == record[dcd_record.case_name(case)]["sha256"]
        plan.set_block(0)
        _same(_decode(g, plan, words, nu, W), exp, "%s after set_block(0)" % dcd_record.case_name(case))


@pytest.mark.parametrize("case", REAL, ids=big_record.dcd_name)
def test_real_sizes_equal_the_model_and_the_record(engine_ctx, case):
    logn, slots, nu = case
    exp = big_record.dcd_model_doubles(case)
    coeffs = big_record.dcd_plaintexts(case)
    g = engine_ctx(logn, 2)
    rec = big_record.golden(big_record.DCD_JSON)["cases"].get(big_record.dcd_name(case))
    with g.ecd_plan(slots, big_record.roots(slots), block=0) as plan:
        for W in (1, 2):
            got = _decode(g, plan, big_record.int64_words(coeffs, W), nu, W)
            _same(got, exp, "%s, W = %d" % (big_record.dcd_name(case), W))
            if rec and big_record.roots_sha(big_record.roots(slots)) == rec["roots_sha256"]:
                assert big_record.sha_doubles(got) == rec["sha256"], "the device's doubles are not the executed reference's"
    assert np.isfinite(got).all() and int((got != 0).sum()) >= 2 * slots


def test_a_batch_of_five_and_a_plan_of_another_context(engine_ctx):
    case = big_record.DCD_CASES[0]
    logn, slots, nu = case
    g, other = engine_ctx(logn, 2), engine_ctx(logn, 6)
    words, exp = big_record.int64_words(big_record.dcd_plaintexts(case), 1), big_record.dcd_model_doubles(case)
    order = [2, 0, 1, 1, 0]
    with g.ecd_plan(slots, big_record.roots(slots), block=0) as plan, other.ecd_plan(slots, block=0) as foreign:
        _same(_decode(g, plan, words[order], nu, 1), exp[order], "five plaintexts")
        _same(_decode(g, plan, words[1:2], nu, 1), exp[1:2], "one plaintext")
        out, big = _poisoned(1, slots), torch.zeros(g.n, dtype=torch.int64, device="cuda")
        g.profile(True)
        try:
            assert g.lib.gpq_he_dcd(g.h, foreign.h, C.c_void_p(out.data_ptr()), C.c_void_p(big.data_ptr()), 1.0, 1, 1, g._stream()) == -1
            assert g.lib.gpq_he_dcd(g.h, plan.h, C.c_void_p(out.data_ptr() + 8), C.c_void_p(big.data_ptr()), 1.0, 1, 1, g._stream()) == -1
            assert g.profile_collect() == {}
        finally:
            g.profile(False)
        torch.cuda.synchronize()
        assert bool((out == out[0]).all())
