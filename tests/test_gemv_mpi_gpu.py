"""he_gemv / he_sum / he_idx through the reference's signatures (src/he-algo.c:47-113) with real libgcrypt MPIs (tests/c/gemv_host.c): every
coefficient, l, and the bits of nu and B against the reference's loop over the library's per-call he_copy_ct / he_rot / he_mulpt / he_add / he_rs,
with keys from the library's he_genrk and a deterministic host he_ecd.  Also ct_dest == ct, he_nrm2's sequence, an odd q (the fallback), and
he_gemv on a ciphertext edited on the host since the call before (at logn 12 from its resident copy: found changed, run again)."""
import os
import subprocess

import pytest

from tests.poly_stats import edited_call_movement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gemv_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gemv") / "gemv_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "gemv_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


# logn 8 / 9: outside 10..15 the modulus bound is q itself (src/precomp.c:339-340), so small rings can carry a few levels
# (12, 109, 4, 0): the smallest ring with resident polynomials (n >= 4096), at the widest modulus it admits
@pytest.mark.parametrize("logn,logq,slots,odd", [(8, 120, 1, 0), (8, 120, 8, 0), (9, 150, 16, 0), (8, 120, 4, 1), (12, 109, 4, 0)])
def test_mpi_gemv_sum_idx_match_the_reference_loop(gemv_host, logn, logq, slots, odd):
    res = subprocess.run([gemv_host, "check", str(logn), str(logq), str(slots), str(odd)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    for name in ("he_gemv", "he_sum", "he_idx 0", "he_idx %d" % (5 % slots), "he_idx %d" % (slots - 1), "he_gemv in place", "he_gemv after a host edit"):
        assert "ok " + name in lines, res.stdout
    resident, confirmed, changed = edited_call_movement(lines)
    assert (resident > 0) == (logn >= 12), res.stdout
    if resident:
        # as printed by the build before the staged-call driver: c0 (edited) found changed, c1 confirmed
        assert (confirmed, changed) == (1, 1), res.stdout
