"""gpq_shim_he_inv / _sqrt / _sigmoid / _log / _exp with real libgcrypt MPIs (tests/c/algo_host.c): each result equals the reference's loop
(src/he-algo.c:131-458) run over this library's own per-call symbols in the same program -- every integer, l, and the bits of nu and B; the
0 returns (an odd modulus, a depth that does not fit, a source that is not centred) leave dst untouched; and where polynomials are kept
resident (n >= 4096) a call finds its source on the device, uploads nothing again and leaves its result there."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["he_inv", "he_sqrt", "he_sigmoid", "he_log", "he_exp"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("algo") / "algo_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "algo_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def _run(args):
    res = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert not [x for x in lines if x.startswith(("FAIL", "MISMATCH"))], lines
    return lines


def _stats(lines, name, when):
    m = [re.match(r"poly stats %s %s: resident (\d+) confirmed (\d+) changed (\d+)$" % (name, when), x) for x in lines]
    (hit,) = [x for x in m if x]
    return tuple(int(v) for v in hit.groups())


# (13, 200): the resident-operand path (n >= 4096); the reference's context caps q by ring (src/precomp.c:53-64), so q = 2^200 needs logn 13
@pytest.mark.parametrize("logn,logq,all_five", [(8, 120, 0), (13, 200, 1)])
def test_one_call_equals_the_loop_over_the_per_call_symbols(host, logn, logq, all_five):
    lines = _run([host, "check", str(logn), str(logq), str(all_five)])
    for name in NAMES[:5 if all_five else 2]:
        assert "ok " + name in lines and "ok %s leaves its source" % name in lines, name
        assert "%s returned 1, he_ecd calls %d" % (name, 1 if name == "he_exp" else 0) in lines
        before, after = _stats(lines, name, "before"), _stats(lines, name, "after")
        if logn >= 12:
            # both polynomials of the source served from their resident copies and confirmed, none uploaded again; the result is remembered
            assert after[1] - before[1] == 2 and after[2] == before[2], (name, before, after)
            assert after[0] >= before[0] >= 2, (name, before, after)
        else:
            assert before[0] == after[0] == 0
    assert "ok he_inv in place, two iterations" in lines


# below the top level and at another scale: q_l, the limb counts, W and Bmult[l] (a different value per level) are no longer the top's.
# (8, 120, Delta 2^20, l = 5 of 6: q_0 = 1, so he_exp runs without an iteration and ends at q_1 = 2^20; 13, 200, Delta 2^30, l = 4 of 6: he_exp
# without an iteration ends at q_0 = 2^20)
@pytest.mark.parametrize("logn,logq,logdelta,down", [(8, 120, 20, 1), (13, 200, 30, 2)])
def test_one_call_equals_the_loop_below_the_top_level(host, logn, logq, logdelta, down):
    lines = _run([host, "check_at", str(logn), str(logq), str(logdelta), str(down), "1"])
    L = logq // logdelta
    assert "source at l %d of L %d" % (L - down, L) in lines
    for name in NAMES:
        assert "ok " + name in lines and "ok %s leaves its source" % name in lines, name
        assert "%s returned 1, he_ecd calls %d" % (name, 1 if name == "he_exp" else 0) in lines
        before, after = _stats(lines, name, "before"), _stats(lines, name, "after")
        if logn >= 12:
            assert after[1] - before[1] == 2 and after[2] == before[2], (name, before, after)
            assert after[0] >= before[0] >= 2, (name, before, after)
        else:
            assert before[0] == after[0] == 0
    assert "ok he_inv in place, two iterations" in lines and "ok he_sigmoid in place" in lines


def test_the_zero_returns_leave_dst_untouched(host):
    lines = _run([host, "refuse", "8", "120"])
    for name in ("he_inv", "he_sqrt", "he_exp"):
        assert "%s with a depth that does not fit returned 0" % name in lines and "ok %s beyond the chain leaves dst" % name in lines
    for name in NAMES:
        assert "%s of a source that is not centred returned 0" % name in lines and "ok %s of a source that is not centred leaves dst" % name in lines
    lines = _run([host, "odd", "8", "120"])
    for name in NAMES:
        assert "%s at an odd modulus returned 0" % name in lines and "ok %s at an odd modulus leaves dst" % name in lines
