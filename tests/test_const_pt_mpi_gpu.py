"""Constant plaintexts behind the reference's he_mulpt / he_addpt / he_subpt symbols, with real libgcrypt MPIs (tests/c/constpt_host.c):
every step gives the same integers, l, nu and B with gpq_mpi_shim_set_const_pt(1) and (0); sparse plaintexts take the constant path, dense,
nearly sparse, wide and odd-q ones do not, and a ciphertext that is not centred falls back once.  One product is checked against the
restated reference (oracle/bigint_ref.py)."""
import os
import re
import subprocess

import pytest

from oracle import bigint_ref as ref
from tests import const_pt_cases as cp
from tests.poly_stats import edited_call_movement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("constpt") / "constpt_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "constpt_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


# step -> (calls that took the constant path, he_mulpt calls among them that fell back)
STEPS = [("he_mulpt real", 1, 0), ("he_rs real", 0, 0), ("he_mulpt negative", 1, 0), ("he_rs negative", 0, 0), ("he_mulpt complex", 1, 0),
         ("he_rs complex", 0, 0), ("he_addpt real", 1, 0), ("he_mulpt const after a host edit", 1, 0), ("he_subpt complex", 1, 0), ("he_addpt complex", 1, 0), ("he_mulpt dense", 0, 0),
         ("he_addpt dense", 0, 0), ("he_mulpt nearly sparse", 0, 0), ("he_subpt nearly sparse", 0, 0), ("he_mulpt nearly sparse at the end", 0, 0),
         ("he_addpt wide constant", 0, 0), ("he_mulpt non-centred", 1, 1), ("he_mulpt centred again", 1, 0)]


def _run(args):
    res = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert not [x for x in lines if x.startswith(("FAIL", "MISMATCH"))], [x for x in lines if not x.startswith("coeff")]
    return lines


def _counters(lines):
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in (re.match(r"counters (.*): taken (\d+) fell_back (\d+)$", x) for x in lines) if m}


# (13, 200): the resident-operand path (n >= 4096).  The reference's context caps q at 2^109 for logn 12 (src/precomp.c:53-64, 128-bit
# security), so q = 2^200 needs logn 13.
@pytest.mark.parametrize("logn,logq", [(8, 120), (13, 200)])
def test_switch_on_and_off_agree_and_the_counters_tell(host, oracle_ctx, logn, logq):
    lines = _run([host, "check", str(logn), str(logq), "1" if logn == 8 else "0"])
    got = _counters(lines)
    for name, taken, fell in STEPS:
        assert "ok " + name in lines, name
        assert got[name] == (taken, fell), (name, got[name])
    assert "ok he_mulpt complex leaves its source" in lines
    resident, confirmed, changed = edited_call_movement(lines)
    assert (resident > 0) == (logn >= 12), [x for x in lines if x.startswith("poly stats")]
    if resident:
        # as printed by the build before the staged-call driver: c0 (edited) found changed, c1 confirmed
        assert (confirmed, changed) == (1, 1), [x for x in lines if x.startswith("poly stats")]
    if logn != 8:
        return
    # the first product, integer by integer, against the restated reference with the plaintext as a dense polynomial
    n = 1 << logn
    polys = {k: [None] * n for k in ("in0", "in1", "out0", "out1")}
    for x in lines:
        if x.startswith("coeff "):
            _, name, i, v = x.split()
            polys[name][int(i)] = int(v, 16)
    a, b, level = (int(v) for v in re.match(r"constant (-?\d+) (-?\d+) level (\d+)$", [x for x in lines if x.startswith("constant ")][0]).groups())
    assert level == logq // 30 and all(v is not None for p in polys.values() for v in p)
    dim = cp.mulpt_dim(logq, 30, logn)
    o = oracle_ctx(logn, dim)
    assert cp.fits(o.p, a, b, logq, dim)
    want = ref.he_mulpt(o, (polys["in0"], polys["in1"]), cp.const_plaintext(n, a, b), dim, logq)
    assert [polys["out0"], polys["out1"]] == want == cp.closed_mulpt((polys["in0"], polys["in1"]), a, b, logq)


def test_an_odd_modulus_never_takes_the_constant_path(host):
    lines = _run([host, "odd", "8", "120"])
    got = _counters(lines)
    for name in ("odd q he_mulpt", "odd q he_addpt", "odd q he_subpt"):
        assert "ok " + name in lines and got[name] == (0, 0), (name, got.get(name))
