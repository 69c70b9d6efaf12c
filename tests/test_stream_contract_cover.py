"""Every function of include/gpqhe_hip.h that takes a `void *stream` is in exactly one class of tests/stream_contract.py, the names of every
class are pinned here, and every function that launches has a closure.  No device.  An export added to the header fails here until someone
reads its launch code and decides its class; an entry that leaves the table, or moves from CAPTURABLE to ORDERED, needs a deliberate edit
of this file (and, by include/gpqhe_hip.h's own sentences, of the header)."""
import os
import re

from tests import stream_contract as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpqhe_hip.h")


def stream_functions(text):
    """the names of the prototypes with a `void *stream` parameter, in the header's order"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|long|size_t|unsigned|void)\s+(gpq_\w+)\s*\(([^;{]*?)\)\s*;", text)
    return [name for name, args in protos if re.search(r"void\s*\*\s*stream\b", args)]


def _header():
    with open(HEADER) as f:
        return f.read()


PINNED = {
    sc.CAPTURABLE: [
        "gpq_ntt", "gpq_invntt", "gpq_ntt_reference", "gpq_rns_mul", "gpq_rns_add", "gpq_poly_mul_rns", "gpq_mulpt_rns", "gpq_he_mul_tensor", "gpq_keyswitch",
        "gpq_rns_decompose", "gpq_rns_decompose_limbs", "gpq_rns_reconstruct", "gpq_poly_mul", "gpq_he_rs", "gpq_he_rescale", "gpq_he_mul", "gpq_he_mul_rs",
        "gpq_relin_tail", "gpq_big_transpose", "gpq_big_addsub", "gpq_relin_tail_overwriting", "gpq_he_swk", "gpq_he_mulpt", "gpq_poly_rot", "gpq_poly_conj",
        "gpq_he_mulpt_const", "gpq_he_addpt_const", "gpq_he_rot_hoisted", "gpq_he_gemv", "gpq_gemv_inner", "gpq_he_gemv_planned", "gpq_he_gemv_multi",
        "gpq_he_ecd", "gpq_he_ecd_diagonals", "gpq_he_dcd", "gpq_he_dec", "gpq_sample_zo", "gpq_sample_error", "gpq_sample_uniform", "gpq_small_to_big",
        "gpq_he_enc_pk", "gpq_he_enc_sk", "gpq_surf_bytes", "gpq_rng_device_bytes", "gpq_big_add", "gpq_big_sub", "gpq_big_neg", "gpq_evk_pack",
        "gpq_he_genswk_batch"],
    sc.ORDERED: [
        "gpq_rns_reconstruct_general", "gpq_poly_mul_general", "gpq_gemv_plan_create", "gpq_gemv_plan_create_from_matrix", "gpq_he_rs_general",
        "gpq_relin_tail_general", "gpq_he_mul_general", "gpq_he_mulpt_general", "gpq_he_swk_general", "gpq_he_genswk"],
    sc.REFUSES_IN_CAPTURE: ["gpq_gemv_multi_create"],
    sc.NOT_A_LAUNCH: ["gpq_upload", "gpq_download", "gpq_copy", "gpq_stream_sync", "gpq_stream_wait", "gpq_probe_stream", "gpq_stream_destroy",
                      "gpq_timer_start", "gpq_timer_stop"],
}


def test_the_parser_finds_the_prototypes_it_is_meant_to():
    names = stream_functions(_header())
    assert len(names) == len(set(names)) == 68, len(names)
    assert {"gpq_ntt", "gpq_he_mul", "gpq_gemv_multi_create", "gpq_timer_stop", "gpq_upload", "gpq_he_genswk_batch"} <= set(names)
    assert stream_functions("int gpq_x(void *stream);\nint gpq_y(int a,\n   void  * stream);\n/* int gpq_z(void *stream); */ int gpq_w(void *s);") == ["gpq_x", "gpq_y"]


def test_every_function_with_a_stream_is_in_exactly_one_class():
    names = stream_functions(_header())
    classes = (sc.CAPTURABLE, sc.ORDERED, sc.REFUSES_IN_CAPTURE, sc.NOT_A_LAUNCH)
    for name in names:
        assert name in sc.TABLE, "%s takes a `void *stream` and tests/stream_contract.py gives it no class: read its launch code and add it" % name
        assert sc.TABLE[name] in classes, name
    # (a dict gives every name one class; the lists below are what the GPU file iterates over)
    listed = [n for cls in classes for n in sc.names_of(cls)]
    assert sorted(listed) == sorted(sc.TABLE) and len(listed) == len(set(listed))
    extra = set(sc.TABLE) - set(names)
    assert extra == set(sc.NAMED_OTHERWISE), "in the table but not a prototype with a `void *stream`: %s" % sorted(extra)
    for name in sc.NAMED_OTHERWISE:
        assert re.search(r"\b%s\s*\(" % name, _header()), name


def test_the_classes_are_the_pinned_ones_name_for_name():
    for cls, names in PINNED.items():
        have = sc.names_of(cls)
        assert sorted(have) == sorted(names), "%s: left the table: %s; not pinned here: %s" % (cls, sorted(set(names) - set(have)), sorted(set(have) - set(names)))
    assert sum(len(v) for v in PINNED.values()) == len(sc.TABLE) == 69
    assert [len(PINNED[c]) for c in (sc.CAPTURABLE, sc.ORDERED, sc.REFUSES_IN_CAPTURE, sc.NOT_A_LAUNCH)] == [49, 10, 1, 9]


def test_every_launching_function_has_a_closure_and_the_others_a_reason():
    launching = sc.names_of(sc.CAPTURABLE) + sc.names_of(sc.ORDERED)
    assert sorted(sc.CALLS) == sorted(launching), "without a closure: %s; a closure without a class: %s" % (
        sorted(set(launching) - set(sc.CALLS)), sorted(set(sc.CALLS) - set(launching)))
    for name, call in sc.CALLS.items():
        assert callable(call)
        specs = [s for s in sc.SPECS if s.name == name]
        assert specs and all(s.call is call for s in specs), name                     # ONE closure per entry point, whatever inputs it runs on
        assert all(s.shapes and set(s.shapes) <= set(sc.SHAPES) | {sc.ECD_SHAPE[0]} for s in specs), name
    keys = [s.key for s in sc.SPECS]
    assert len(keys) == len(set(keys))
    assert sorted(sc.NOT_A_LAUNCH_REASON) == sorted(sc.names_of(sc.NOT_A_LAUNCH))
    for name, reason in sc.NOT_A_LAUNCH_REASON.items():
        assert reason and "\n" not in reason, name
    assert set(sc.REPEATS_ON_REPLAY) <= set(sc.names_of(sc.CAPTURABLE))
    # the runs the issue names beyond one per entry point: gpq_ntt / gpq_invntt on a slab with an all-zero limb
    assert {"gpq_ntt (all-zero limb)", "gpq_invntt (all-zero limb)"} <= set(keys)


def test_the_header_states_the_class_of_every_function_in_the_table():
    """include/gpqhe_hip.h carries the contract itself: a section that defines the classes and lists every function of the table under its
    class, so that a reader of the header alone knows which calls may be captured"""
    text = _header()
    m = re.search(r"/\* ---- stream classes.*?\*/", text, flags=re.S)
    assert m, "include/gpqhe_hip.h has no `stream classes` section"
    section = m.group(0)
    for cls in (sc.CAPTURABLE, sc.ORDERED, sc.REFUSES_IN_CAPTURE, sc.NOT_A_LAUNCH):
        block = re.search(r"^ \* %s\b(.*?)(?=^ \* [A-Z_]{7,}\b|\Z)" % cls, section, flags=re.S | re.M)
        assert block, cls
        stated = set(re.findall(r"\bgpq_\w+", block.group(1)))
        for name in sc.names_of(cls):
            assert name in stated, "the header's stream classes section does not list %s under %s" % (name, cls)
        others = stated & set(sc.TABLE) - set(sc.names_of(cls))
        assert not others, "%s: listed under %s in the header, in another class in the table" % (sorted(others), cls)
