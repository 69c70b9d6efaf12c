"""he_genrlk / he_genck / he_genrk through the reference's signatures with real libgcrypt MPIs (tests/c/keygen_host.c), against the model
(tests/genswk_model.py, which tests/test_genswk_model.py holds against the executed reference).

The host program's samplers are fillers that hand out polynomials this test wrote; its randombytes is a counter-driven stream of its own.
Default mode: per key sample_error, then sample_uniform, in the reference's order (logged).  With gpq_mpi_shim_set_device_samplers(1):
randombytes is called per key with n, then n (nbits / 8 + 1) bytes, and no sampler is.  Every key -- rlk, ck, rk[0..8) -- holds the model's
words, and he_rot and he_mul with those keys equal the restated reference (oracle/bigint_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bigint_ref as ref
from tests import enc_model
from tests import genswk_model as gm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, ROT = 8, 3


@pytest.fixture(scope="module")
def keygen_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("keygen") / "keygen_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "keygen_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def host_stream(count):
    """the first `count` bytes of keygen_host.c's randombytes"""
    M = (1 << 64) - 1
    k = np.arange(1, (count + 7) // 8 + 1, dtype=np.uint64)
    z = k * np.uint64(0x9e3779b97f4a7c15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    z ^= z >> np.uint64(31)
    assert int(z[0]) <= M
    return z.view(np.uint8)[:count].copy()


def _write(path, polys):
    with open(path, "w") as f:
        for p in polys:
            for v in p:
                f.write("%s%X\n" % ("-" if v < 0 else "", abs(int(v))))


def _parse(stdout):
    calls, polys, name = [], {}, None
    for line in stdout.split("\n"):
        for noise in ("Generating rlk ... ", "Generating ck ... ", "Generating rk ... "):
            line = line.replace(noise, "")
        line = line.strip()
        if line.startswith("call "):
            calls.append(line[5:]); name = None
        elif line.startswith("info "):
            name = None
        elif line.startswith("poly "):
            name = line[5:]; polys[name] = []
        elif name is not None and line and line not in ("done", "done."):
            polys[name].append(int(line, 16))
    return calls, polys


@pytest.mark.parametrize("mode,logn,logq", [("host", 7, 100), ("device", 7, 100), ("host", 13, 100), ("device", 13, 100)],
                         ids=["host_samplers", "device_samplers", "host_samplers_two_pass", "device_samplers_two_pass"])
def test_keys_equal_the_model_and_switch_keys(keygen_host, tmp_path, mode, logn, logq):
    from oracle.oracle import OracleCtx
    n, q = 1 << logn, 1 << logq
    probe = OracleCtx(logn, 12)
    dimP, dimA, dimB, dimevk = ref.he_dims(logn, probe.p, logq, logq)
    o = OracleCtx(logn, dimevk)
    primes = [int(p) for p in o.p]
    P = gm.product_of(primes[:dimP])
    PqL, nbits, dimmul = P << logq, gm.nbits_of(P, logq), gm.dimmul_of(P, logq, logn)
    nb, nkeys = nbits // 8 + 1, 2 + SLOTS
    rng = np.random.default_rng(11 + logn)
    sk = enc_model.sample_hwt(enc_model.Stream(rng.integers(0, 256, 8192, dtype=np.uint8)), n)
    ct = [[int.from_bytes(rng.bytes(16), "little") % q - q // 2 for _ in range(n)] for _ in range(2)]
    if mode == "host":                                                    # what the fillers hand out: the test's own polynomials
        es = [enc_model.error_from_bytes(rng.integers(0, 256, n, dtype=np.uint8), n).tolist() for _ in range(nkeys)]
        us = [enc_model.uniform_from_bytes(rng.integers(0, 256, n * nb, dtype=np.uint8), n, nbits) for _ in range(nkeys)]
        per_key = ["sample_error", "sample_uniform"]
    else:                                                                 # the bytes the library asks randombytes for, expanded by the model
        s = enc_model.Stream(host_stream(nkeys * (n + n * nb)))
        es, us = [], []
        for _ in range(nkeys):
            es.append(enc_model.sample_error(s, n).tolist())
            us.append(enc_model.sample_uniform(s, n, PqL))
        per_key = ["randombytes %d" % n, "randombytes %d" % (n * nb)]
    _write(tmp_path / "sk.txt", [sk]); _write(tmp_path / "ct.txt", ct + ct)
    _write(tmp_path / "error.txt", es if mode == "host" else []); _write(tmp_path / "uniform.txt", us if mode == "host" else [])
    res = subprocess.run([keygen_host, mode, str(logn), str(logq), str(SLOTS), str(ROT), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    calls, polys = _parse(res.stdout)
    assert calls == ["he_genrlk"] + per_key + ["he_genck"] + per_key + ["he_genrk"] + per_key * SLOTS, \
        "the samplers / randombytes were not called in the reference's order with its byte counts"
    # the keys: rlk hides s^2 centred mod q_L (src/he-kem.c:130), ck the conjugate, rk[r] the rotation by r
    hidden = [gm.poly_mul(primes, sk, sk, (logq + 1) // 59 + 1, q), gm.galois_image(sk, 2 * n - 1)] + [gm.galois_image(sk, pow(5, r, 1 << 64)) for r in range(SLOTS)]
    assert hidden[1] == ref.poly_conj(sk) and hidden[2 + ROT] == ref.poly_rot(sk, ROT)
    got = np.fromfile(tmp_path / "keys.bin", dtype=np.uint64).reshape(nkeys, 2, dimevk * n)
    slab = lambda poly: o.ntt_slab(np.array([v % p for p in primes[:dimevk] for v in poly], dtype=np.uint64), dimevk)
    want = {}
    for j in range(nkeys):
        w0, w1 = gm.genswk(P, logq, primes, us[j], es[j], hidden[j], sk, dimmul, dimevk)
        want[j] = (slab(w0), slab(w1))
        assert np.array_equal(got[j, 1], want[j][1]), "key %d: swk.p1 differs from the model" % j
        assert np.array_equal(got[j, 0], want[j][0]), "key %d: swk.p0 differs from the model" % j
    # he_rot and he_mul with those keys: the restated reference (src/he-automorphism.c:101-115, src/he-mult.c:88-156)
    r0, r1 = ref.he_swk(o, ref.poly_rot(ct[0], ROT), ref.poly_rot(ct[1], ROT), *want[2 + ROT], dimP, dimB, logq)
    assert polys["rot_c0"] == r0 and polys["rot_c1"] == r1
    m0, m1 = ref.he_mul(o, ct, ct, *want[0], dimP, dimA, dimB, logq)
    assert polys["mul_c0"] == m0 and polys["mul_c1"] == m1
