"""The lane body of the device generator (surf_chunk, gpqhe_amd/csrc/rng_kernels.hpp) on the CPU under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/c/rng_sanitized.cpp runs every lane of the launcher's grid over positions at every phase and at the
edges of the 128-bit range, every destination offset and lengths around a lane, a wave and a workgroup, compares each byte with the block
function and lets the sanitizer watch exact-size buffers.  The bounds logic is one host- and device-callable function, checked here on the
CPU.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("san")
    flags = ["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all"]
    # whether the sanitizers' runtimes are there is decided on a program that holds none of the code under test
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(flags + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("hipcc cannot build an empty program with the host sanitizers: " + (r.stderr.splitlines() or ["?"])[-1])
    out = str(tmp / "rng_sanitized")
    r = subprocess.run(flags + ["-I", os.path.join(ROOT, "gpqhe_amd", "csrc"), os.path.join(ROOT, "tests", "c", "rng_sanitized.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_lane_body_under_asan_and_ubsan(binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    word = r.stdout.split()
    assert word[0] == "ok" and int(word[1]) > 20000
