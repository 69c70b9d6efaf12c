"""Every switch of include/gpqhe_hip.h is run by the settings tests or is listed as not being one (tests/bridge_settings.py).  No device: the
entries of SETTINGS are applied to a recorder.  A switch added to the header fails here until someone decides where it belongs."""
import os
import re

from tests import bridge_settings as bs

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpqhe_hip.h")


def _switches():
    with open(HEADER) as f:
        text = f.read()
    names = set(re.findall(r"^int\s+(gpq_set_\w+)\s*\(", text, flags=re.M))
    names |= set(re.findall(r"^int\s+(gpq_debug_force_redo)\s*\(\s*gpq_ctx\s*\*", text, flags=re.M))
    return names


def test_the_header_still_declares_the_switches_this_test_looks_for():
    names = _switches()
    assert {"gpq_set_prescale", "gpq_set_stream_bridge", "gpq_set_bridge_mfma", "gpq_set_exact_crt", "gpq_set_lazy_decompose", "gpq_debug_force_redo",
            "gpq_set_overlap", "gpq_set_nt_policy", "gpq_set_limb_classes", "gpq_set_limb_block", "gpq_set_chunk", "gpq_set_device"} <= names, names


def test_every_switch_is_run_by_a_setting_or_listed_as_not_one():
    names, used = _switches(), bs.switches_used()
    for name in sorted(names):
        assert (name in used) != (name in bs.NOT_A_WORD_SETTING), \
            "%s: %s" % (name, "both used by SETTINGS and listed in NOT_A_WORD_SETTING" if name in used else
                        "no entry of tests/bridge_settings.SETTINGS calls it and NOT_A_WORD_SETTING does not list it")
    for name, reason in bs.NOT_A_WORD_SETTING.items():
        assert name in names, "%s is listed in NOT_A_WORD_SETTING but the header does not declare it" % name
        assert reason and "\n" not in reason
    assert set(used) <= names, "SETTINGS calls what the header does not declare: %s" % sorted(set(used) - names)


# The whole table: every entry's name, the switches it flips with their arguments, and whether the bridge-only calls run under it.  The GPU
# files parametrise over the table, so an entry that left it, or changed what it sets, would only shrink their matrix; it fails here instead.
_BRIDGE, _TAIL = ("bridge", "tail"), ("tail",)
TABLE = {
    "default": ([], _BRIDGE),
    "stream bridge off": ([("set_stream_bridge", False)], _BRIDGE),
    "prescale 2": ([("set_prescale", 2)], _TAIL),
    "prescale 1": ([("set_prescale", 1)], _TAIL),
    "prescale 0": ([("set_prescale", 0)], _TAIL),
    "integer-VALU decompose": ([("set_bridge_mfma", False)], _BRIDGE),
    "exact CRT": ([("set_exact_crt", True)], _BRIDGE),
    "canonical decompose": ([("set_lazy_decompose", False)], _TAIL),
    "force redo 1": ([("debug_force_redo", 1)], _BRIDGE),
    "force redo 7": ([("debug_force_redo", 7)], _BRIDGE),
    "nt always": ([("set_nt_policy", 1)], _TAIL),
    "general butterflies": ([("set_limb_classes", 0, 0)], _BRIDGE),
    "limb block 2": ([("set_limb_block", 2)], _BRIDGE),
    "two lanes": ([("set_overlap", 1)], _TAIL),
    "stream bridge off + prescale 0 + exact CRT": ([("set_stream_bridge", False), ("set_prescale", 0), ("set_exact_crt", True)], _TAIL),
    "integer-VALU decompose + force redo 3": ([("set_bridge_mfma", False), ("debug_force_redo", 3)], _BRIDGE),
    "prescale 2 + canonical decompose + limb block 2": ([("set_prescale", 2), ("set_lazy_decompose", False), ("set_limb_block", 2)], _TAIL),
}


def test_the_table_is_the_pinned_one_entry_for_entry():
    assert list(bs.SETTINGS) == list(TABLE), "entries missing: %s, entries not pinned here: %s" % (
        sorted(set(TABLE) - set(bs.SETTINGS)), sorted(set(bs.SETTINGS) - set(TABLE)))
    for setting, (apply, tags) in bs.SETTINGS.items():
        r = bs.Recorder()
        apply(r)
        calls, want_tags = TABLE[setting]
        assert r.calls == calls, "`%s` sets %s, pinned as %s" % (setting, r.calls, calls)
        assert tuple(tags) == want_tags, setting
    # the settings the bridge-only calls run under (tests/test_settings_bridge_calls_gpu.py), and the key-switching calls under all of them
    assert bs.tagged("bridge") == [s for s, (_, tags) in TABLE.items() if "bridge" in tags] and len(bs.tagged("bridge")) == 9
    assert bs.tagged("tail") == list(TABLE) and len(TABLE) == 17
    assert bs.CHUNK == 2 and list(bs.ALWAYS) == ["gpq_set_chunk"]
