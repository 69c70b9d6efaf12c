"""gpq_he_dcd: he_dcd (src/he-encode.c:66-74, :114-117; src/canemb.c:43-60; src/types.c:77-106) on the device.

* bit for bit (uint64 views of the doubles) against the record of the EXECUTED reference (tests/golden/ref_dcd.json): the device and the
  numpy model (tests/dcd_model.py) both read the stored root table, so this machine's libm plays no part; the model's doubles must have
  the recorded sha256 and the device's doubles must be the model's.  The output is poisoned first.
* a batch of 67 plaintexts against the same plaintexts one by one; the capacity edge (8192 slots); a coefficient of 1100 bits (infinity);
  encode -> decode on the device against the two models; every refusal."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import to_host
from tests import dcd_model, dcd_record, ecd_model

pytestmark = pytest.mark.gpu
POISON_BITS = 0xFFF8DEADBEEF5A5A                                          # a NaN with a payload: compared as bits only


def _slab(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1)).to("cuda")


def _poisoned(count, slots):
    return torch.from_numpy(np.full(count * slots * 2, POISON_BITS, dtype=np.uint64).view(np.int64)).to("cuda")


def _decode(g, plan, words, nu, W):
    """[count][slots][2] float64 of one gpq_he_dcd call on a poisoned output"""
    count = words.shape[0]
    out = _poisoned(count, plan.slots)
    g.he_dcd(plan, out.view(torch.float64), _slab(words), nu, W)
    torch.cuda.synchronize()
    return to_host(out).view(np.float64).reshape(count, plan.slots, 2)


def _same(got, exp, what):
    bad = np.argwhere(dcd_model.bits(got) != dcd_model.bits(exp))
    assert not len(bad), "%s: %d doubles differ, first (plaintext, slot, part) %s: %r (%#x) vs %r (%#x)" % (
        what, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), int(dcd_model.bits(got)[tuple(bad[0])]),
        float(exp[tuple(bad[0])]), int(dcd_model.bits(exp)[tuple(bad[0])]))


@pytest.fixture(scope="module")
def stored():
    return dcd_record.dcd_golden()["cases"], dcd_record.stored_roots()


@pytest.mark.parametrize("case", dcd_record.CASES, ids=dcd_record.case_name)
def test_doubles_equal_the_record_of_the_executed_reference(engine_ctx, stored, case):
    record, T = stored
    logn, slots, W, nu = case
    exp = dcd_record.model_doubles(case, T)
    assert dcd_record.sha(exp) == record[dcd_record.case_name(case)]["sha256"], "the model on the stored table is not the record"
    g = engine_ctx(logn, 2)
    with g.ecd_plan(slots, T) as plan:
        got = _decode(g, plan, dcd_model.words(dcd_record.case_plaintexts(case), W), nu, W)
    _same(got, exp, dcd_record.case_name(case))
    assert np.isfinite(got).all() and int((got != 0).sum()) >= 2 * slots


def test_a_batch_equals_its_plaintexts_one_by_one(engine_ctx, stored):
    _, T = stored
    logn, slots, W, count, nu = 9, 16, 2, 67, 3.0 * 2 ** 29 + 1
    g = engine_ctx(logn, 2)
    rng = random.Random(67)
    coeffs = [[dcd_record._signed(rng, 2, 126) for _ in range(g.n)] for _ in range(count)]
    words = dcd_model.words(coeffs, W)
    with g.ecd_plan(slots, T) as plan:
        got = _decode(g, plan, words, nu, W)
        single = np.concatenate([_decode(g, plan, words[k:k + 1], nu, W) for k in range(count)])
    _same(got, single, "batch of %d" % count)
    _same(got, dcd_model.decode(coeffs, T, slots, nu), "batch against the model")


def test_capacity_edge_8192_slots(engine_ctx):
    logn, slots, W, nu = dcd_record.LARGE[-1]
    assert slots == 8192 and slots == (1 << logn) // 2
    g = engine_ctx(logn, 2)
    T = ecd_model.roots_via_sincos(slots)                                 # the same table on both sides
    coeffs = dcd_record.large_plaintexts(dcd_record.LARGE[-1])
    with g.ecd_plan(slots, T) as plan:
        _same(_decode(g, plan, dcd_model.words(coeffs, W), nu, W), dcd_model.decode(coeffs, T, slots, nu), "8192 slots")


@pytest.mark.parametrize("sign", [1, -1])
def test_one_slot_and_a_coefficient_of_1100_bits(engine_ctx, stored, sign):
    _, T = stored
    logn, slots, W, nu = 7, 1, 18, 3.0 * 2 ** 29 + 1
    g = engine_ctx(logn, 2)
    rng = random.Random(1100)
    coeffs = [[dcd_record._signed(rng, 30, 900) for _ in range(g.n)]]
    coeffs[0][0] = sign * (rng.getrandbits(1100) | (1 << 1099))          # the real part: beyond every double
    exp = dcd_model.decode(coeffs, T, slots, nu)
    assert np.isinf(exp[0, 0, 0]) and np.sign(exp[0, 0, 0]) == sign and np.isfinite(exp[0, 0, 1]) and exp[0, 0, 1] != 0
    with g.ecd_plan(slots, T) as plan:
        got = _decode(g, plan, dcd_model.words(coeffs, W), nu, W)
    assert np.isinf(got[0, 0, 0]) and np.sign(got[0, 0, 0]) == sign
    assert dcd_model.bits(got)[0, 0, 1] == dcd_model.bits(exp)[0, 0, 1]


def test_encode_then_decode_on_the_device_is_model_encode_then_model_decode(engine_ctx, stored):
    _, T = stored
    logn, slots, logDelta, W = 9, 64, 30, 2
    g = engine_ctx(logn, 2)
    rng = np.random.default_rng(964)
    z = 2.0 ** 25 * (rng.uniform(-1, 1, (5, slots)) + 1j * rng.uniform(-1, 1, (5, slots)))
    coeffs, offending = ecd_model.encode(z, T, g.n, logDelta)
    assert offending == 0 and ecd_model.max_bits(coeffs) > 53
    exp = dcd_model.decode([[int(v) for v in p] for p in coeffs], T, slots, 2.0 ** logDelta)
    slab = torch.empty(5 * W * g.n, dtype=torch.int64, device="cuda")
    out = _poisoned(5, slots)
    with g.ecd_plan(slots, T) as plan:
        g.he_ecd(plan, slab, torch.from_numpy(z).to("cuda"), logDelta, W)
        g.he_dcd(plan, out.view(torch.float64), slab, 2.0 ** logDelta, W)
        torch.cuda.synchronize()
    got = to_host(out).view(np.float64).reshape(5, slots, 2)
    _same(got, exp, "encode -> decode")
    assert np.abs(got[..., 0] + 1j * got[..., 1] - z).max() < 1e-3       # (and it is the message again, to the encoder's rounding)


def test_refusals_launch_nothing(engine_ctx, stored):
    _, T = stored
    g, other = engine_ctx(9, 2), engine_ctx(9, 6)
    slots, W = 4, 2
    big = torch.zeros(W * g.n, dtype=torch.int64, device="cuda")
    out = _poisoned(1, slots)
    o, b, s = C.c_void_p(out.data_ptr()), C.c_void_p(big.data_ptr()), g._stream()
    with g.ecd_plan(slots, T) as plan, other.ecd_plan(slots, T) as foreign:
        call = g.lib.gpq_he_dcd
        g.profile(True)
        try:
            assert call(None, plan.h, o, b, 1.0, W, 1, s) == -1
            assert call(g.h, None, o, b, 1.0, W, 1, s) == -1
            assert call(g.h, plan.h, None, b, 1.0, W, 1, s) == -1
            assert call(g.h, plan.h, o, None, 1.0, W, 1, s) == -1
            assert call(g.h, foreign.h, o, b, 1.0, W, 1, s) == -1          # a plan of another context
            assert call(g.h, plan.h, o, b, 1.0, 0, 1, s) == -1
            assert call(g.h, plan.h, o, b, 1.0, 33, 1, s) == -1
            assert call(g.h, plan.h, o, b, 1.0, W, 0, s) == -1
            for nu in (0.0, -1.0, float("inf"), float("nan")):
                assert call(g.h, plan.h, o, b, nu, W, 1, s) == -1
            if torch.cuda.device_count() > 1:                               # the wrong current device
                with torch.cuda.device(1):
                    assert call(g.h, plan.h, o, b, 1.0, W, 1, s) == -1
            assert g.profile_collect() == {}                                # nothing was launched
        finally:
            g.profile(False)
        torch.cuda.synchronize()
        assert bool((out == out[0]).all()) and int(out[0].item()) == int(np.array([POISON_BITS], dtype=np.uint64).view(np.int64)[0])
        assert call(g.h, plan.h, o, b, 5e-324, W, 1, s) == 0               # the smallest double above 0 is a nu
        torch.cuda.synchronize()
