"""gpq_shim_he_dec_dcd through the reference's signatures with real libgcrypt MPIs (tests/c/dcd_host.c): he_dec followed by he_dcd with the
plaintext staying on the device gives, bit for bit, the doubles of the shim's he_dec followed by the host program's own decoder -- a
plain-C statement of the reference's decode that reads polyctx.ring.zetas and runs mpi_to_double's bit loop with gcry_mpi_test_bit --
twice (the second time everything is resident) and once more after a host-side edit of c1; he_dec alone still gives the same integers afterwards; and with a q_l that is no power
of two the call returns 0 and leaves m untouched."""
import os
import subprocess

import pytest

from tests.poly_stats import edited_call_movement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dcd_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dcd") / "dcd_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "dcd_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def _run(host, *args):
    res = subprocess.run([host] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    assert not [x for x in lines if x.startswith(("FAIL", "MISMATCH"))], res.stdout
    return lines, res.stdout


@pytest.mark.parametrize("logn,logq,slots", [(9, 120, 16), (13, 120, 4)])
def test_device_decode_gives_the_doubles_of_he_dec_and_the_host_decoder(dcd_host, logn, logq, slots):
    lines, out = _run(dcd_host, "check", logn, logq, slots)
    for name in ["gpq_shim_he_dec_dcd returns 1", "device decode against he_dec + host decode", "again: gpq_shim_he_dec_dcd returns 1",
                 "again, everything resident: device decode against he_dec + host decode", "he_dec copies nu", "he_dec alone afterwards: the same integers",
                 "after a host edit: gpq_shim_he_dec_dcd returns 1", "after a host edit: device decode against he_dec + host decode"]:
        assert "ok " + name in lines, out
    resident, confirmed, changed = edited_call_movement(lines)
    assert (resident > 0) == (logn >= 12), out
    if resident:
        # as printed by the build before the staged-call driver: c1 (edited) found changed, sk and c0 confirmed
        assert (confirmed, changed) == (2, 1), out


def test_a_modulus_that_is_no_power_of_two_falls_back(dcd_host):
    lines, out = _run(dcd_host, "fallback", 9, 120, 16)
    for name in ["q_l no power of two: returns 0", "q_l no power of two: m untouched", "q_l no power of two: he_dec + host decode"]:
        assert "ok " + name in lines, out
