"""gpq_shim_he_dec_dcd above 8192 slots through the reference's signatures with real libgcrypt MPIs (tests/c/dcd_host.c, whose arguments
take the shape as it is): at n = 2^15 with 16384 slots, he_dec followed by he_dcd with the plaintext staying on the device gives, bit for
bit, the doubles of the shim's he_dec followed by the host program's own decoder, twice.  The host fills its 16 * 16384 = 262 144-byte
result with a pattern before each call and accepts only non-zero finite doubles in every slot: all of those bytes came down."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dcd_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dcd_big") / "dcd_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "dcd_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_16384_slots_decode_on_the_device(dcd_host):
    logn, logq, slots = 15, 120, 16384
    assert 16 * slots == 262144
    res = subprocess.run([dcd_host, "check", str(logn), str(logq), str(slots)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    assert not [x for x in lines if x.startswith(("FAIL", "MISMATCH"))], res.stdout
    for name in ["gpq_shim_he_dec_dcd returns 1", "device decode against he_dec + host decode", "again: gpq_shim_he_dec_dcd returns 1",
                 "again, everything resident: device decode against he_dec + host decode", "he_dec alone afterwards: the same integers"]:
        assert "ok " + name in lines, res.stdout
