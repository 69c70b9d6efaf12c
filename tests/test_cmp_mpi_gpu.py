"""gpq_shim_he_cmp / gpq_shim_he_cmppt with real libgcrypt MPIs (tests/c/cmp_host.c): each result equals the reference's loop
(src/he-algo.c:460-548) run over this library's own per-call symbols in the same program -- every integer, l, and the bits of nu and B; with
dst == ct1, dst == ct2 and one ciphertext on both sides; the 0 returns (unequal levels, alpha 0 and 53, a depth beyond l, a source that is not
centred) leave dst untouched; and where polynomials are kept resident (n >= 4096) a call finds both sources on the device and uploads
nothing again."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cmp") / "cmp_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "cmp_host.c"),
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


# (logn, logq, logDelta, he_cmp's iter and alpha, he_cmppt's iter and t).  (8, 120, 2^20): L = 6 and q_0 = 1, so at most 5 levels: alpha 1 is t 0.
# (13, 200, 2^30): the resident-operand path; he_cmppt with a round, 6 levels down to q_0 = 2^20.  (13, 200, 2^20): alpha 2 is t 2, 9 of 10 levels.
@pytest.mark.parametrize("logn,logq,logdelta,iter,alpha,iterpt,tpt", [(8, 120, 20, 1, 1, 2, 0), (13, 200, 30, 1, 1, 0, 1), (13, 200, 20, 0, 2, 1, 1)])
def test_one_call_equals_the_loop_over_the_per_call_symbols(host, logn, logq, logdelta, iter, alpha, iterpt, tpt):
    lines = _run([host, "check", str(logn), str(logq), str(logdelta), str(iter), str(alpha), str(iterpt), str(tpt)])
    for what in ("he_cmp", "he_cmp leaves its first source", "he_cmp leaves its second source", "he_cmp with dst == ct1", "he_cmp with dst == ct2",
                 "he_cmp of one ciphertext with itself", "he_cmppt", "he_cmppt leaves its source", "he_cmppt by he_const_pt(1)"):
        assert "ok " + what in lines, what
    assert "he_cmp returned 1" in lines and "he_cmppt returned 1" in lines
    for name, polys in (("he_cmp", 4), ("he_cmppt", 2)):
        before, after = _stats(lines, name, "before"), _stats(lines, name, "after")
        if logn >= 12:
            # every polynomial of the sources served from its resident copy and confirmed, none uploaded again; the result is remembered
            assert after[1] - before[1] == polys and after[2] == before[2], (name, before, after)
            assert after[0] >= before[0] >= 4, (name, before, after)
        else:
            assert before[0] == after[0] == 0


def test_the_zero_returns_leave_dst_untouched(host):
    lines = _run([host, "refuse", "8", "120", "20"])
    for what in ("he_cmp of unequal levels", "he_cmp with alpha 0", "he_cmp with alpha 53", "he_cmp with a depth beyond l", "he_cmp with rounds beyond l",
                 "he_cmppt with a depth beyond l", "he_cmppt with a depth that overflows", "he_cmp of a second source that is not centred",
                 "he_cmp of a first source that is not centred", "he_cmppt of a source that is not centred"):
        assert what + " returned 0" in lines and "ok %s leaves dst" % what in lines, what
