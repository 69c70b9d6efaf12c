"""The record of the executed reference's samplers, he_keypair, he_enc_sk, he_enc_pk and he_dec: what tests/test_he_samplers_gpu.py and
tests/test_he_enc_gpu.py compare the device with on every machine.

tests/golden/ref_enc_stream.npy -- the first 16 KiB the executed reference's randombytes hands out (the SUPERCOP stream oracle/Makefile
compiles in; its state is per process, so every reference run below happens in a worker process of its own and starts at byte 0).
tests/golden/ref_enc.json -- per case sha256 of the output words ([W][n] uint64, W = WORDS(logq)) of
  sample_zo, sample_error, sample_uniform(q)      each alone, from byte 0
  he_keypair (sk, p0, p1); he_enc_sk (c0, c1); he_enc_pk with that key pair (c0, c1); he_dec of both ciphertexts      one run, in this order
with the stream position after every call (found by drawing PROBE more bytes after it and looking them up in the stream), and sha256 of
the whole Gaussian pair table.  Written by `python -m tests.enc_record` from oracle/_ref/; tests/test_ref_enc.py recomputes it wherever
the reference can be built and holds the model (tests/enc_model.py) against it."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np

from oracle import ref
from oracle.expect import ints_to_words
from tests import enc_model
from tests.ref_jobs import ROOT

ENC_JSON = os.path.join(ROOT, "tests", "golden", "ref_enc.json")
STREAM_NPY = os.path.join(ROOT, "tests", "golden", "ref_enc_stream.npy")
STREAM_BYTES = 16384
PROBE = 8
SLOTS, LOGDELTA = 4, 30
# logn, logq.  After the first two: W = 2, 2, 3, 3, 7, 3 words and hectx.dim = 2, 2, 3, 3, 8, 4 limbs -- logq one below and on a word
# boundary (the raw sample of logq + 1 bits then fills a word resp. opens the next), the workload's q = 2^438, and a four-limb basis.
# The model's whole `he` run of every case stays inside the stored STREAM_BYTES ((7, 438) ends at byte 15376 + PROBE).
CASES = [(7, 120), (9, 100), (7, 63), (7, 64), (7, 127), (7, 128), (7, 438), (8, 190)]


def case_name(case):
    return "%d_%d" % tuple(case)


def words(logq):
    """words that hold a raw sample below 2^(logq + 1) as a non-negative value"""
    return (logq + 1) // 64 + 1


def case_plaintext(case):
    """[n] seeded coefficients of up to 40 bits, both signs: the plaintext of both encryptions (nu = Delta)"""
    logn, logq = case
    rng = random.Random(12000 + 100 * logn + logq)
    return [rng.randrange(-(1 << 40), 1 << 40) for _ in range(1 << logn)]


def sha(values, W):
    return hashlib.sha256(ints_to_words([int(v) for v in values], W).tobytes()).hexdigest()


class _PolyMpi(C.Structure):
    _fields_ = [("coeffs", C.POINTER(C.c_void_p))]


class _HePk(C.Structure):                                  # src/gpqhe.h:72-75
    _fields_ = [("p0", _PolyMpi), ("p1", _PolyMpi)]


class _HeCt(C.Structure):                                  # src/gpqhe.h:84-90
    _fields_ = [("l", C.c_uint), ("nu", C.c_double), ("B", C.c_double), ("c0", _PolyMpi), ("c1", _PolyMpi)]


class _HePt(C.Structure):                                  # src/gpqhe.h:93-96
    _fields_ = [("nu", C.c_double), ("m", _PolyMpi)]


def _gcrypt():
    G = C.CDLL("libgcrypt.so.20")
    G.gcry_mpi_scan.restype, G.gcry_mpi_scan.argtypes = C.c_uint, [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_size_t, C.c_void_p]
    G.gcry_mpi_print.restype, G.gcry_mpi_print.argtypes = C.c_uint, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    G.gcry_mpi_set.restype, G.gcry_mpi_set.argtypes = C.c_void_p, [C.c_void_p, C.c_void_p]
    G.gcry_mpi_neg.restype, G.gcry_mpi_neg.argtypes = None, [C.c_void_p, C.c_void_p]
    G.gcry_mpi_release.restype, G.gcry_mpi_release.argtypes = None, [C.c_void_p]
    return G


def _mpi(G, v):
    t = C.c_void_p()
    assert G.gcry_mpi_scan(C.byref(t), 4, b"%X" % abs(v), 0, None) == 0          # GCRYMPI_FMT_HEX
    if v < 0:
        G.gcry_mpi_neg(t, t)
    return t


def _ints(G, poly, n):
    buf, got, out = C.create_string_buffer(1024), C.c_size_t(), []
    for i in range(n):
        assert G.gcry_mpi_print(4, buf, len(buf), C.byref(got), poly.coeffs[i]) == 0
        out.append(int(buf.value.decode(), 16))
    return out


def ref_stream(count):
    """worker job: the first `count` bytes of the executed reference's randombytes"""
    L = ref.Ref().L
    buf = np.zeros(count, dtype=np.uint8)
    L.randombytes(buf.ctypes.data_as(C.c_void_p), C.c_size_t(count))
    return buf


def ref_run(arg):
    """worker job: (kind, logn, logq) -> {name: [n] Python integers} and, under "probe:<name>", the PROBE bytes drawn after the call"""
    kind, logn, logq = arg
    R = ref.Ref().init(logn, 1 << logq, SLOTS, 1 << LOGDELTA)
    L, G, n, out = R.L, _gcrypt(), 1 << logn, {}

    def probe(name):
        buf = np.zeros(PROBE, dtype=np.uint8)
        L.randombytes(buf.ctypes.data_as(C.c_void_p), C.c_size_t(PROBE))
        out["probe:" + name] = buf

    def poly():
        p = _PolyMpi()
        L.he_alloc_sk(C.byref(p))
        return p

    if kind in ("sample_zo", "sample_error"):
        p = poly()
        getattr(L, kind)(C.byref(p))
        out[kind] = _ints(G, p, n)
        probe(kind)
    elif kind == "sample_uniform":
        p, q = poly(), _mpi(G, 1 << logq)
        L.sample_uniform(C.byref(p), q)
        out[kind] = _ints(G, p, n)
        probe(kind)
    else:
        assert kind == "he"
        pk, sk, pt, ct_sk, ct_pk, back = _HePk(), poly(), _HePt(), _HeCt(), _HeCt(), _HePt()
        L.he_alloc_pk(C.byref(pk))
        for t in (pt, back):
            L.he_alloc_pt(C.byref(t))
        for t in (ct_sk, ct_pk):
            L.he_alloc_ct(C.byref(t))
        L.he_keypair(C.byref(pk), C.byref(sk))
        out.update(sk=_ints(G, sk, n), p0=_ints(G, pk.p0, n), p1=_ints(G, pk.p1, n))
        probe("he_keypair")
        for i, v in enumerate(case_plaintext((logn, logq))):
            t = _mpi(G, v)
            G.gcry_mpi_set(pt.m.coeffs[i], t)
            G.gcry_mpi_release(t)
        pt.nu = float(1 << LOGDELTA)
        L.he_enc_sk(C.byref(ct_sk), C.byref(pt), C.byref(sk))
        out.update(sk_c0=_ints(G, ct_sk.c0, n), sk_c1=_ints(G, ct_sk.c1, n))
        probe("he_enc_sk")
        L.he_enc_pk(C.byref(ct_pk), C.byref(pt), C.byref(pk))
        out.update(pk_c0=_ints(G, ct_pk.c0, n), pk_c1=_ints(G, ct_pk.c1, n))
        probe("he_enc_pk")
        out["ct"] = [(t.l, ref.bits(t.nu), ref.bits(t.B)) for t in (ct_sk, ct_pk)]
        L.he_dec(C.byref(back), C.byref(ct_sk), C.byref(sk))
        out["dec_sk"] = _ints(G, back.m, n)
        L.he_dec(C.byref(back), C.byref(ct_pk), C.byref(sk))
        out["dec_pk"] = _ints(G, back.m, n)
    return out


KINDS = ("sample_zo", "sample_error", "sample_uniform", "he")
SAMPLERS = KINDS[:3]
HE_NAMES = ("sk", "p0", "p1", "sk_c0", "sk_c1", "pk_c0", "pk_c1", "dec_sk", "dec_pk")
HE_CALLS = ("he_keypair", "he_enc_sk", "he_enc_pk")


def model_run(kind, case, stream_bytes):
    """the model's answer to ref_run on the same stream: {name: values} and, under "pos:<call>", the stream position after the call
    (the PROBE bytes the record draws after each call are skipped as the reference's run consumed them)"""
    from oracle.oracle import OracleCtx
    logn, logq = case
    n, q, s, out = 1 << logn, 1 << logq, enc_model.Stream(stream_bytes), {}

    def mark(name):
        out["pos:" + name] = s.pos
        out["probe:" + name] = s.take(PROBE).copy()

    if kind == "sample_zo":
        out[kind] = enc_model.sample_zo(s, n).tolist()
        mark(kind)
    elif kind == "sample_error":
        out[kind] = enc_model.sample_error(s, n).tolist()
        mark(kind)
    elif kind == "sample_uniform":
        out[kind] = enc_model.sample_uniform(s, n, q)
        mark(kind)
    else:
        o = OracleCtx(logn, enc_model.he_dim(logn, q))
        (p0, p1), sk = enc_model.he_keypair(o, s, q)
        out.update(sk=sk, p0=p0, p1=p1)
        mark("he_keypair")
        m = case_plaintext(case)
        out["sk_c0"], out["sk_c1"] = enc_model.he_enc_sk(o, s, m, sk, q)
        mark("he_enc_sk")
        out["pk_c0"], out["pk_c1"] = enc_model.he_enc_pk(o, s, m, (p0, p1), q)
        mark("he_enc_pk")
        out["dec_sk"] = enc_model.he_dec(o, (out["sk_c0"], out["sk_c1"]), sk, q)
        out["dec_pk"] = enc_model.he_dec(o, (out["pk_c0"], out["pk_c1"]), sk, q)
    return out


def case_record(case, runs, stream_bytes):
    """the stored form of one case: runs = {kind: ref_run's or model_run's result}"""
    logn, logq = case
    W, blob = words(logq), stream_bytes.tobytes()
    rec = {"logn": logn, "logq": logq, "W": W, "sha256": {}, "pos": {}}
    for kind in KINDS:
        for name, v in runs[kind].items():
            if name.startswith("probe:"):
                pos = blob.find(np.asarray(v, dtype=np.uint8).tobytes())
                assert pos >= 0 and blob.find(np.asarray(v, dtype=np.uint8).tobytes(), pos + 1) < 0, "the probe after %s must occur once in the stream" % name[6:]
                rec["pos"][name[6:]] = pos
            elif not name.startswith("pos:") and name != "ct":
                rec["sha256"][name] = sha(v, W)
    return rec


def table_sha(table):
    return hashlib.sha256(np.ascontiguousarray(table, dtype=np.int8).tobytes()).hexdigest()


def enc_record():
    """(the whole record, the stream) from the executed reference (needs oracle/_ref/)"""
    jobs = [(kind, logn, logq) for logn, logq in CASES for kind in KINDS]
    stream, = ref.run(ref_stream, [STREAM_BYTES], workers=1)
    got = ref.run(ref_run, jobs, workers=8)
    cases = {}
    for k, case in enumerate(CASES):
        cases[case_name(case)] = case_record(case, dict(zip(KINDS, got[k * len(KINDS):(k + 1) * len(KINDS)])), stream)
    rec = {"_provenance": "Outputs of the GPQHE reference's sample_zo, sample_error, sample_uniform, he_keypair, he_enc_sk, he_enc_pk and he_dec, executed "
           "on its SUPERCOP randombytes stream (tests/golden/ref_enc_stream.npy holds the stream's first 16 KiB) with the seeded plaintext of "
           "tests/enc_record.py: sha256 of the output words and the stream position after each call. gauss_table_sha256: of the 65536 x 2 int8 "
           "pair table behind sample_error. Data only; tests/test_ref_enc.py recomputes and compares.",
           "gauss_table_sha256": table_sha(enc_model.gauss_table()), "cases": cases}
    return json.loads(json.dumps(rec)), stream


def enc_golden():
    with open(ENC_JSON) as f:
        return json.load(f)


def stored_stream():
    return np.load(STREAM_NPY)


if __name__ == "__main__":
    rec, stream = enc_record()
    with open(ENC_JSON, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    np.save(STREAM_NPY, stream)
    print("wrote", os.path.relpath(ENC_JSON, ROOT), "and", os.path.relpath(STREAM_NPY, ROOT))
