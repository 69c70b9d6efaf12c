"""The plan cache of he_gemv / he_sum / he_idx through the reference's signatures with real libgcrypt MPIs (tests/c/gemv_plan_host.c): a
repeat call with the same matrix makes no he_ecd call, whatever the encoded diagonals depend on misses, five matrices evict the first of
four entries, gpq_shim_gemv_plan_cache(0) restores the per-call path, an odd q takes the loop -- and every result equals the reference's
loop over the library's per-call symbols in every coefficient, l, and the bits of nu and B."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gemv_plan") / "gemv_plan_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "gemv_plan_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


EXPECTED = ["first call", "first call encodes every diagonal", "second call, another ciphertext", "second call makes no he_ecd call",
            "matrix changed in place", "a changed entry misses", "the changed matrix hits next time", "another level", "another ct->l misses",
            "another Delta", "another Delta misses", "the plan made before is still there", "the fifth matrix is kept", "the first matrix was evicted",
            "he_sum", "he_sum again", "he_sum again makes no he_ecd call", "he_idx 0", "he_idx 0 again", "he_idx again makes no he_ecd call",
            "he_gemv in place", "he_nrm2 sequence", "cache off: first call encodes", "cache off: second call encodes"]


@pytest.mark.parametrize("logn,logq,slots", [(8, 120, 8), (9, 150, 16), (8, 120, 1)])
def test_repeat_calls_reuse_the_plan(plan_host, logn, logq, slots):
    res = subprocess.run([plan_host, "check", str(logn), str(logq), str(slots), "0"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    assert not [x for x in lines if x.startswith(("FAIL", "MISMATCH"))], res.stdout
    for name in EXPECTED + (["he_idx %d" % (5 % slots), "he_idx %d again" % (5 % slots)] if slots > 1 else []):
        assert "ok " + name in lines, res.stdout


def test_an_odd_modulus_takes_the_loop_every_time(plan_host):
    res = subprocess.run([plan_host, "check", "8", "120", "4", "1"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    for name in ("odd q first", "odd q first call encodes", "odd q second", "odd q second call encodes"):
        assert "ok " + name in lines, res.stdout
