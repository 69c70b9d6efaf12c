"""gpq_mpi_shim_set_device_ecd through the reference's signatures with real libgcrypt MPIs (tests/c/ecd_host.c): he_gemv / he_sum / he_idx
with the diagonals encoded on the device from the matrix give the coefficients, l and bits of nu and B of the same calls with the host
program's he_ecd -- a plain-C statement of the reference's encoder that reads polyctx.ring -- while he_ecd is called zero times instead
of once per diagonal; a matrix with a coefficient beyond 2^63 falls back to he_ecd and gives the host encoder's words."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ecd_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ecd") / "ecd_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "ecd_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


EXPECTED = ["%s, switch off: one he_ecd call per diagonal", "%s, switch on: no he_ecd call", "%s, device encoder against host encoder"]


@pytest.mark.parametrize("logn,logq,slots", [(9, 120, 16), (13, 120, 4)])
def test_device_encoder_gives_the_host_encoders_results(ecd_host, logn, logq, slots):
    res = subprocess.run([ecd_host, "check", str(logn), str(logq), str(slots)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    assert not [x for x in lines if x.startswith(("FAIL", "MISMATCH"))], res.stdout
    want = [e % name for name in ("he_gemv", "he_sum", "he_idx") for e in EXPECTED]
    want += ["he_gemv again, switch on: no he_ecd call", "he_gemv again, the plan made on the device", "out of range, switch on: falls back to he_ecd",
             "out of range, switch off: he_ecd", "out of range: the fallback gives the host encoder's words"]
    for name in want:
        assert "ok " + name in lines, res.stdout
