"""he_keypair / he_enc_sk / he_enc_pk through the reference's signatures with real libgcrypt MPIs (tests/c/enc_host.c), against the model
(tests/enc_model.py, which tests/test_ref_enc.py holds against the executed reference).

The host program's four samplers are fillers that hand out polynomials this test wrote; its randombytes is a counter-driven stream of its
own.  Default mode: the drop-ins call the samplers in the reference's order (logged), the outputs are the model's on those polynomials and
l / nu / B are set as src/he-encrypt.c:40-42.  With gpq_mpi_shim_set_device_samplers(1): randombytes is called with the reference's byte
counts in order, sample_zo / sample_error / sample_uniform are not called, sample_sk still is, and the ciphertexts are the model's on that
stream.  he_dec of the results gives the model's plaintext plus noise; a second he_enc_pk runs with keys and plaintext resident (n = 2^13);
a q_L that is no power of two runs the fallback; and the workload's q_L = 2^438 runs with seven words and eight limbs."""
import os
import subprocess

import numpy as np
import pytest

from tests import enc_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, LOGDELTA = 4, 30


@pytest.fixture(scope="module")
def enc_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("enc") / "enc_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "enc_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def host_stream(count):
    """the first `count` bytes of enc_host.c's randombytes"""
    M = (1 << 64) - 1
    out = bytearray()
    for k in range((count + 7) // 8):
        z = ((k + 1) * 0x9e3779b97f4a7c15) & M
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        z ^= z >> 31
        out += z.to_bytes(8, "little")
    return np.frombuffer(bytes(out[:count]), dtype=np.uint8)


def _write(path, polys):
    with open(path, "w") as f:
        for p in polys:
            for v in p:
                f.write("%s%X\n" % ("-" if v < 0 else "", abs(int(v))))


def _parse(stdout):
    calls, infos, polys, name = [], {}, {}, None
    for line in stdout.split("\n"):
        line = line.replace("Generating sk and pk ... ", "").strip()
        if line.startswith("call "):
            calls.append(line[5:]); name = None
        elif line.startswith("info "):
            w = line.split()
            infos[w[1]] = dict(zip(w[2::2], w[3::2])); name = None
        elif line.startswith("poly "):
            name = line[5:]; polys[name] = []
        elif name is not None and line and line not in ("done", "done."):
            polys[name].append(int(line, 16))
    return calls, infos, polys


@pytest.mark.parametrize("mode,logn,logq,minus", [("host", 9, 100, 0), ("device", 9, 100, 0), ("host", 13, 100, 0), ("device", 13, 100, 0),
                                                  ("host", 9, 100, 159), ("device", 9, 100, 159), ("host", 9, 438, 0), ("device", 9, 438, 0)],
                         ids=["host_samplers", "device_samplers", "host_samplers_resident", "device_samplers_resident", "fallback_q_not_pow2",
                              "fallback_device_samplers", "host_samplers_seven_words", "device_samplers_seven_words"])
def test_drop_ins_equal_the_model(enc_host, tmp_path, mode, logn, logq, minus):
    from oracle.oracle import OracleCtx
    n, q = 1 << logn, (1 << logq) - minus
    nbits = q.bit_length()
    nb, dim = nbits // 8 + 1, enc_model.he_dim(logn, q)
    assert (logq, minus) != (438, 0) or (dim == 8 and nbits // 64 + 1 == 7)   # the workload's q = 2^438: seven words, eight limbs
    o = OracleCtx(logn, dim)
    rng = np.random.default_rng(77 + logn + minus)
    sk = enc_model.sample_hwt(enc_model.Stream(rng.integers(0, 256, 8192, dtype=np.uint8)), n)
    m = [int(v) for v in rng.integers(-(1 << 40), 1 << 40, n)]
    if mode == "host":                                                    # what the fillers hand out: the test's own polynomials
        errors = [enc_model.error_from_bytes(rng.integers(0, 256, n, dtype=np.uint8), n).tolist() for _ in range(6)]
        zos = [enc_model.zo_from_bytes(rng.integers(0, 256, n // 4, dtype=np.uint8), n).tolist() for _ in range(2)]
        unis = [enc_model.uniform_from_bytes(rng.integers(0, 256, n * nb, dtype=np.uint8), n, nbits) for _ in range(2)]
        ie, iz, iu = iter(errors), iter(zos), iter(unis)
        draw_error, draw_zo, draw_uniform = (lambda: next(ie)), (lambda: next(iz)), (lambda: next(iu))
        log_error, log_zo, log_uniform = ["sample_error"], ["sample_zo"], ["sample_uniform"]
    else:                                                                 # the bytes the library asks randombytes for, expanded by the model
        errors, zos, unis = [], [], []
        s = enc_model.Stream(host_stream(4 * n * nb + 16 * n))
        draw_error, draw_zo, draw_uniform = (lambda: enc_model.sample_error(s, n).tolist()), (lambda: enc_model.sample_zo(s, n).tolist()), (lambda: enc_model.sample_uniform(s, n, q))
        log_error, log_zo, log_uniform = ["randombytes %d" % n], ["randombytes %d" % (n // 4)], ["randombytes %d" % (n * nb)]
    _write(tmp_path / "sk.txt", [sk]); _write(tmp_path / "m.txt", [m])
    _write(tmp_path / "error.txt", errors); _write(tmp_path / "zo.txt", zos); _write(tmp_path / "uniform.txt", unis)

    # the model, in the reference's order
    want, log = {"sk": sk}, ["he_keypair", "sample_sk"]
    e = draw_error(); a = draw_uniform(); log += log_error + log_uniform
    want["p0"], want["p1"] = enc_model.enc_sk_from(o, None, a, e, sk, dim, q)
    log.append("he_enc_sk")
    e = draw_error(); a = draw_uniform(); log += log_error + log_uniform
    want["sk_c0"], want["sk_c1"] = enc_model.enc_sk_from(o, m, a, e, sk, dim, q)
    for tag in ("pk", "pk2"):
        log.append("he_enc_pk" if tag == "pk" else "he_enc_pk again")
        v = draw_zo(); e0 = draw_error(); e1 = draw_error(); log += log_zo + log_error + log_error
        want[tag + "_c0"], want[tag + "_c1"] = enc_model.enc_pk_from(o, m, v, e0, e1, (want["p0"], want["p1"]), dim, q)
    want["dec_sk"] = enc_model.he_dec(o, (want["sk_c0"], want["sk_c1"]), sk, q)
    want["dec_pk"] = enc_model.he_dec(o, (want["pk_c0"], want["pk_c1"]), sk, q)
    want["dec_pk2"] = enc_model.he_dec(o, (want["pk2_c0"], want["pk2_c1"]), sk, q)

    res = subprocess.run([enc_host, mode, str(logn), str(logq), str(minus), str(SLOTS), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    calls, infos, polys = _parse(res.stdout)
    assert calls == log, "the samplers / randombytes were not called in the reference's order with its byte counts"
    if mode == "device":
        assert not [c for c in calls if c in ("sample_zo", "sample_error", "sample_uniform")] and calls.count("sample_sk") == 1
    assert sorted(polys) == sorted(want)
    for name in want:
        bad = [i for i, (x, y) in enumerate(zip(polys[name], want[name])) if x != y]
        assert not bad and len(polys[name]) == n, "%s: %d coefficients differ from the model, first at %s" % (name, len(bad), bad[:3])
    for name in ("he_enc_sk", "he_enc_pk"):                               # src/he-encrypt.c:40-42 with pt.nu = Delta
        i = infos[name]
        assert i["l"] == i["L"]
        assert i["B"] == i["Bclean"] and int(i["nu"], 16) == int(np.array([2.0 ** LOGDELTA]).view(np.uint64)[0])
    for name in ("dec_sk", "dec_pk", "dec_pk2"):                          # the plaintext plus small noise
        noise = max(abs(x - y) for x, y in zip(polys[name], m))
        assert 0 < noise < 1 << 14, (name, noise)
    assert polys["pk_c0"] != polys["pk2_c0"]
