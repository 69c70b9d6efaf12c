"""gpq_mpi_shim_set_device_rng through the reference's signatures with real libgcrypt MPIs (tests/c/rng_host.c): a host program whose
randombytes forwards to gpq_randombytes, so that host and device draw from ONE stream -- the reference's, from byte 0.

he_keypair, he_enc_sk, he_enc_pk, he_genrlk, he_genck and he_genrk for 8 rotations at n = 2^7 (one-pass transforms) and n = 2^13
(two-pass), with the device samplers fed by the host's randombytes (the path before the device generator) and with
gpq_mpi_shim_set_device_rng(1).  Both runs give the same coefficients, the same keys and the same stream position after every call; both
equal the models (tests/enc_model.py, tests/genswk_model.py) on the stream of tests/surf_model.py; and with the device generator the log
holds no randombytes call of a sampler's size -- only sample_sk's 8-byte draws."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bigint_ref as ref
from tests import enc_model, surf_model
from tests import genswk_model as gm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, LOGQ = 8, 100
POLYS = ("sk", "p0", "p1", "sk_c0", "sk_c1", "pk_c0", "pk_c1")
CALLS = ("he_keypair", "he_enc_sk", "he_enc_pk", "he_genrlk", "he_genck", "he_genrk")


@pytest.fixture(scope="module")
def rng_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rng") / "rng_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "rng_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def _parse(stdout):
    calls, pos, polys, name = [], {}, {}, None
    for line in stdout.split("\n"):
        for noise in ("Generating sk and pk ... ", "Generating rlk ... ", "Generating ck ... ", "Generating rk ... "):
            line = line.replace(noise, "")
        line = line.strip()
        if line.startswith("call "):
            calls.append(line[5:]); name = None
        elif line.startswith("pos "):
            w = line.split()
            pos[w[1]] = int(w[2]) | (int(w[3]) << 64); name = None
        elif line.startswith("poly "):
            name = line[5:]; polys[name] = []
        elif name is not None and line and line not in ("done", "done."):
            polys[name].append(int(line, 16))
    return calls, pos, polys


def _model(logn, m):
    """what the reference computes on its own stream from byte 0: polynomials, key words and the position after every call"""
    from oracle.oracle import OracleCtx
    n, q = 1 << logn, 1 << LOGQ
    dimP, dimA, dimB, dimevk = ref.he_dims(logn, OracleCtx(logn, 12).p, LOGQ, LOGQ)
    o = OracleCtx(logn, dimevk)
    primes = [int(p) for p in o.p]
    P = gm.product_of(primes[:dimP])
    PqL, nbits, dimmul = P << LOGQ, gm.nbits_of(P, LOGQ), gm.dimmul_of(P, LOGQ, logn)
    nb, nbP, nkeys = (LOGQ + 1) // 8 + 1, nbits // 8 + 1, 2 + SLOTS
    s = surf_model.Surf()
    want, pos = {}, {}
    (want["p0"], want["p1"]), sk = enc_model.he_keypair(o, s, q)
    want["sk"], pos["he_keypair"] = sk, s.pos
    want["sk_c0"], want["sk_c1"] = enc_model.he_enc_sk(o, s, m, sk, q)
    pos["he_enc_sk"] = s.pos
    want["pk_c0"], want["pk_c1"] = enc_model.he_enc_pk(o, s, m, (want["p0"], want["p1"]), q)
    pos["he_enc_pk"] = s.pos
    hidden = [gm.poly_mul(primes, sk, sk, (LOGQ + 1) // 59 + 1, q), gm.galois_image(sk, 2 * n - 1)] + [gm.galois_image(sk, pow(5, r, 1 << 64)) for r in range(SLOTS)]
    slab = lambda poly: o.ntt_slab(np.array([v % p for p in primes[:dimevk] for v in poly], dtype=np.uint64), dimevk)
    keys = []
    for j in range(nkeys):
        e = enc_model.sample_error(s, n).tolist()
        u = enc_model.sample_uniform(s, n, PqL)
        w0, w1 = gm.genswk(P, LOGQ, primes, u, e, hidden[j], sk, dimmul, dimevk)
        keys.append((slab(w0), slab(w1)))
        if j < 2:
            pos[CALLS[3 + j]] = s.pos
    pos["he_genrk"] = s.pos
    sizes = {n // 4, n, n * nb, n * nbP}
    return want, pos, keys, sizes, dimevk


@pytest.mark.parametrize("logn", [7, 13], ids=["one_pass", "two_pass"])
def test_device_rng_equals_the_forwarded_host_stream_and_the_models(rng_host, tmp_path, logn):
    n = 1 << logn
    m = [int(v) for v in np.random.default_rng(31 + logn).integers(-(1 << 40), 1 << 40, n)]
    runs = {}
    for mode in ("host", "device"):
        d = tmp_path / mode
        d.mkdir()
        with open(d / "m.txt", "w") as f:
            for v in m:
                f.write("%s%X\n" % ("-" if v < 0 else "", abs(v)))
        res = subprocess.run([rng_host, mode, str(logn), str(LOGQ), str(SLOTS), str(d)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        runs[mode] = _parse(res.stdout) + (np.fromfile(d / "keys.bin", dtype=np.uint64),)
    want, pos, keys, sizes, dimevk = _model(logn, m)
    assert 8 not in sizes
    for mode in ("host", "device"):
        calls, got_pos, polys, words = runs[mode]
        assert got_pos == pos, "%s: the stream position after a call differs from the reference's byte counts" % mode
        assert sorted(polys) == sorted(POLYS)
        for name in POLYS:
            bad = [i for i, (x, y) in enumerate(zip(polys[name], want[name])) if x != y]
            assert not bad and len(polys[name]) == n, "%s %s: %d coefficients differ from the model, first at %s" % (mode, name, len(bad), bad[:3])
        words = words.reshape(2 + SLOTS, 2, dimevk * n)
        for j, (w0, w1) in enumerate(keys):
            assert np.array_equal(words[j, 1], w1), "%s key %d: swk.p1 differs from the model" % (mode, j)
            assert np.array_equal(words[j, 0], w0), "%s key %d: swk.p0 differs from the model" % (mode, j)
        assert [c for c in calls if not c.startswith("randombytes")] == ["he_keypair", "sample_sk"] + list(CALLS[1:])
        drawn = [int(c.split()[1]) for c in calls if c.startswith("randombytes")]
        if mode == "device":
            assert drawn and set(drawn) == {8}, "with the device generator only sample_sk draws from the host's randombytes"
        else:
            assert sizes <= set(drawn) and sum(drawn) == pos["he_genrk"]
    assert runs["host"][2] == runs["device"][2] and np.array_equal(runs["host"][3], runs["device"][3])
