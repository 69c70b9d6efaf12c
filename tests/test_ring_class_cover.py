"""The matrix ring x butterfly class x cache policy of the transform kernels, as the case tables of tests/test_inject_gpu.py and
tests/test_ring15_calls_gpu.py spell it.  No device: the GPU files parametrise over the tables, so an entry that left them would only shrink
their matrix; it fails here instead.  A ring or a class added to engine.hip's launch_strided / for_limb_ranges fails here until the tables grow."""
import os
import re

from tests import test_inject_gpu as inject
from tests import test_ring15_calls_gpu as calls

ENGINE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpqhe_amd", "csrc", "engine.hip")
TWO_PASS_RINGS = [13, 14, 15, 16, 17]
CLASSES = 3                                      # wide-split, split, 7-mad


def _source():
    with open(ENGINE) as f:
        return f.read()


def test_the_rings_and_classes_are_still_the_ones_this_test_knows():
    text = _source()
    strided = text[text.index("int launch_strided("):text.index("int launch_contig(")]
    assert sorted(int(r) for r in re.findall(r"case (\d+):", strided)) == TWO_PASS_RINGS
    ranges = text[text.index("int for_limb_ranges("):text.index("static inline void with_nt(")]
    assert re.findall(r"f\((\w+)\{\}", ranges) == ["TwW", "TwS", "uint64_t"]         # one launch per class present, in this order


def test_class_ranges_follow_for_limb_ranges():
    assert inject.class_ranges(3, (1, 2)) == (1, 1, 1) and inject.launches(3, (1, 2)) == 3
    assert inject.class_ranges(9, (3, 6)) == (3, 3, 3) and inject.class_ranges(12, (1, 2)) == (1, 1, 10)
    assert inject.class_ranges(3, (0, 0)) == (0, 0, 3) and inject.class_ranges(3, (0, 3)) == (0, 3, 0) and inject.class_ranges(3, (3, 3)) == (3, 0, 0)
    assert inject.class_ranges(2, (0, 64)) == (0, 2, 0) and inject.class_ranges(2, (64, 64)) == (2, 0, 0) and inject.class_ranges(2, (5, 1)) == (1, 0, 1)
    assert [inject.launches(3, c) for c in ((0, 0), (0, 3), (3, 3), (1, 1), (0, 1), (1, 3))] == [1, 1, 1, 2, 2, 2]


def _all_classes(dim, classes):
    return inject.launches(dim, classes) == CLASSES


def test_every_ring_has_all_three_classes_in_one_transform_against_the_oracle():
    for logn in TWO_PASS_RINGS:
        assert any(ring == logn and _all_classes(dim, classes) for ring, dim, classes in inject.CASES), "ring %d" % logn
    assert {ring for ring, _, _ in inject.CASES} <= set(TWO_PASS_RINGS)


def test_ring_15_has_each_uniform_arrangement():
    for uniform in ((0, 3, 0), (3, 0, 0), (0, 0, 3)):                            # limbs per class: all split, all wide-split, all 7-mad
        assert any(ring == 15 and inject.class_ranges(dim, classes) == uniform for ring, dim, classes in inject.CASES), uniform


def test_both_cache_policies_are_parametrized():
    assert sorted(inject.NT_POLICIES) == [0, 1]
    marks = [m for m in inject.test_injected_butterflies_match_the_oracle.pytestmark if m.name == "parametrize"]
    assert any(m.args[0] == "nt" and m.args[1] is inject.NT_POLICIES for m in marks)
    assert any(m.args[0] == "logn,dim,classes" and m.args[1] is inject.CASES for m in marks)


def test_the_odd_batch_runs_the_pair_and_the_single_form():
    assert inject.BATCH == 3 and calls.BATCH == 3


def test_whole_calls_run_ring_15_by_default_and_rings_14_to_16_under_all_classes():
    assert (15, None) in calls.CASES and (15, None) in calls.RING15
    for logn in (14, 15, 16):
        assert any(ring == logn and classes is not None and _all_classes(calls.DIMS[ring][2], classes) for ring, classes in calls.CASES), "ring %d" % logn
    assert any(ring == 15 and classes is not None and _all_classes(calls.DIMS[ring][2], classes) for ring, classes in calls.RING15)
    assert set(calls.RING15) <= set(calls.CASES) and {ring for ring, _ in calls.CASES} <= set(calls.DIMS)
    for test, table in ((calls.test_he_mul_matches_the_integers, calls.CASES), (calls.test_he_swk_matches_the_integers, calls.CASES),
                        (calls.test_hoisted_rotations_equal_poly_rot_and_he_swk, calls.CASES),
                        (calls.test_he_mul_rs_matches_the_integers_and_rides_in_the_streaming_tail, calls.RING15),
                        (calls.test_gemv_inner_matches_the_integers, calls.RING15)):
        marks = [m for m in test.pytestmark if m.name == "parametrize"]
        assert any(m.args[1] is table for m in marks), test.__name__
    assert len(calls.ROTS) == 2 and calls.GEMV_SLOTS == 4 and calls.LOGDELTA_RS == 40 and (calls.LOGQ, calls.W) == (200, 4)
