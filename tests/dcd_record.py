"""The record of the executed reference's he_dcd: what tests/test_he_dcd_gpu.py compares the device decoder with on every machine.

tests/golden/ref_dcd.json -- per case the seed, the parameters and sha256 of the 64-bit patterns of the output doubles (eight plaintexts,
[8][slots][2] float64).  The root table is tests/golden/ref_ecd_roots512.npy, the one the encoder's record was made with, reused as it is.
The record is written by `python -m tests.dcd_record` from oracle/_ref/; tests/test_ref_dcd.py recomputes it wherever the reference can
be built and holds the numpy model (tests/dcd_model.py) against it.

The reference's he_dcd, he_alloc_pt and mpi_to_double are exported by oracle/_ref/libgpqhe_ref.so; the worker job below reaches them
through `ref.Ref().L` with its own ctypes `struct he_pt` and fills the coefficients through libgcrypt's gcry_mpi_scan / gcry_mpi_set."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np

from oracle import ref
from tests import dcd_model
from tests.ecd_record import LOGQ, ROOTS_SLOTS, stored_roots   # noqa: F401  (stored_roots: the table of both records)
from tests.ref_jobs import ROOT

DCD_JSON = os.path.join(ROOT, "tests", "golden", "ref_dcd.json")
# logn, slots, W, nu
CASES = [(7, 1, 1, 2.0 ** 30), (7, 2, 2, 2.0 ** 30), (7, 4, 1, 2.0 ** 20), (9, 16, 2, 3.0 * 2 ** 29 + 1), (9, 64, 7, 2.0 ** 30), (8, 128, 1, 1e9),
         (10, 512, 2, 2.0 ** 40)]
LARGE = [(12, 2048, 1, 2.0 ** 30), (13, 4096, 1, 2.0 ** 30), (14, 8192, 1, 2.0 ** 30)]   # live only (tests/test_ref_dcd.py): the capacity edge and the two sizes below it
NOT_POW2 = [c for c in CASES if c[3] in (3.0 * 2 ** 29 + 1, 1e9)]                        # the two cases whose nu is no power of two
PLAINTEXTS = 8


def case_name(case):
    return "%d_%d_%d_%s" % (case[0], case[1], case[2], float(case[3]).hex())


def case_seed(case):
    logn, slots, W, nu = case
    return 8000 + 100 * logn + slots + W


def _signed(rng, lo_bits, hi_bits):
    bits = rng.randint(lo_bits, hi_bits)
    v = rng.getrandbits(bits) | (1 << (bits - 1))                    # exactly `bits` bits
    return -v if rng.getrandbits(1) else v


def pattern54(M_odd, b, sign, tail=5):
    """a value of 54 + tail bits whose top 53 bits M are odd or even, whose 54th bit is b and whose `tail` lower bits are all set"""
    M = (1 << 52) | (0x5A5A5A5A5A5A4 | (1 if M_odd else 0))
    return sign * ((((M << 1) | b) << tail) | ((1 << tail) - 1))


def case_plaintexts(case):
    """the eight plaintexts of a case as [8][n] Python integers: signed coefficients of 20-52 bits (exact conversions); of 54 .. 64 W - 2 bits;
    zeros; one non-zero coefficient; all -1; +-(2^53 +- 1); the four 54-bit patterns (M odd or even) x (b = 0 or 1) with lower bits set,
    in both signs; every coefficient -2^(64 W - 1).  EVERY coefficient of the polynomial is filled, not only those the decoder reads."""
    logn, slots, W, nu = case
    n, rng = 1 << logn, random.Random(case_seed(case))
    gap = n // 2 // slots
    p = [[_signed(rng, 20, 52) for _ in range(n)],
         [_signed(rng, 54, 64 * W - 2) for _ in range(n)],
         [0] * n,
         [0] * n,
         [-1] * n,
         [(1, -1)[(i >> 1) & 1] * ((1 << 53) + (1, -1)[i & 1]) for i in range(n)],
         [pattern54(i & 1, (i >> 1) & 1, (1, -1)[(i >> 2) & 1]) for i in range(n)],
         [-(1 << (64 * W - 1))] * n]
    p[3][(slots // 3) * gap + n // 2] = -((1 << 61) + 12345)
    for i in range(0, n, gap):                      # the slots the decoder reads see every pattern whatever the gap
        k = i // gap
        p[5][i] = (1, -1)[(k >> 1) & 1] * ((1 << 53) + (1, -1)[k & 1])
        p[6][i] = pattern54(k & 1, (k >> 1) & 1, (1, -1)[(k >> 2) & 1])
    assert len(p) == PLAINTEXTS
    return p


def large_plaintexts(case):
    logn, slots, W, nu = case
    n, rng = 1 << logn, random.Random(9100 + slots)
    return [[_signed(rng, 54, 62) for _ in range(n)], [pattern54(i & 1, (i >> 1) & 1, (1, -1)[(i >> 2) & 1]) for i in range(n)]]


def sha(z):
    return hashlib.sha256(dcd_model.bits(z).tobytes()).hexdigest()


class _PolyMpi(C.Structure):
    _fields_ = [("coeffs", C.POINTER(C.c_void_p))]


class _HePt(C.Structure):                                  # src/gpqhe.h:93-96
    _fields_ = [("nu", C.c_double), ("m", _PolyMpi)]


def ref_decode(arg):
    """worker job: (logn, slots, nu, plaintexts) -> float64 [count][slots][2] by the executed reference's he_dcd"""
    logn, slots, nu, plaintexts = arg
    R = ref.Ref().init(logn, 1 << LOGQ.get(logn, 120), slots, 1 << 30)
    L = R.L
    G = C.CDLL("libgcrypt.so.20")
    G.gcry_mpi_scan.restype, G.gcry_mpi_scan.argtypes = C.c_uint, [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_size_t, C.c_void_p]
    G.gcry_mpi_set.restype, G.gcry_mpi_set.argtypes = C.c_void_p, [C.c_void_p, C.c_void_p]
    G.gcry_mpi_neg.restype, G.gcry_mpi_neg.argtypes = None, [C.c_void_p, C.c_void_p]
    G.gcry_mpi_release.restype, G.gcry_mpi_release.argtypes = None, [C.c_void_p]
    L.he_alloc_pt.restype, L.he_alloc_pt.argtypes = None, [C.POINTER(_HePt)]
    L.he_free_pt.restype, L.he_free_pt.argtypes = None, [C.POINTER(_HePt)]
    L.he_dcd.restype, L.he_dcd.argtypes = None, [C.c_void_p, C.POINTER(_HePt)]
    pt = _HePt()
    L.he_alloc_pt(C.byref(pt))
    out = np.empty((len(plaintexts), slots, 2), dtype=np.float64)
    for k, p in enumerate(plaintexts):
        assert len(p) == R.n
        for i, v in enumerate(p):
            t = C.c_void_p()
            assert G.gcry_mpi_scan(C.byref(t), 4, b"%X" % abs(v), 0, None) == 0          # GCRYMPI_FMT_HEX
            if v < 0:
                G.gcry_mpi_neg(t, t)
            G.gcry_mpi_set(pt.m.coeffs[i], t)
            G.gcry_mpi_release(t)
        pt.nu = nu
        z = np.empty((slots, 2), dtype=np.float64)
        L.he_dcd(z.ctypes.data_as(C.c_void_p), C.byref(pt))
        out[k] = z
    L.he_free_pt(C.byref(pt))
    return out


def ref_to_double(values):
    """worker job: mpi_to_double of every Python integer, by the executed reference"""
    L = ref.Ref().L
    G = C.CDLL("libgcrypt.so.20")
    G.gcry_mpi_scan.restype, G.gcry_mpi_scan.argtypes = C.c_uint, [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_size_t, C.c_void_p]
    G.gcry_mpi_neg.restype, G.gcry_mpi_neg.argtypes = None, [C.c_void_p, C.c_void_p]
    G.gcry_mpi_release.restype, G.gcry_mpi_release.argtypes = None, [C.c_void_p]
    L.mpi_to_double.restype, L.mpi_to_double.argtypes = C.c_double, [C.c_void_p]
    out = np.empty(len(values), dtype=np.float64)
    for k, v in enumerate(values):
        t = C.c_void_p()
        assert G.gcry_mpi_scan(C.byref(t), 4, b"%X" % abs(v), 0, None) == 0
        if v < 0:
            G.gcry_mpi_neg(t, t)
        out[k] = L.mpi_to_double(t)
        G.gcry_mpi_release(t)
    return out


def case_record(case, z):
    logn, slots, W, nu = case
    assert z.shape == (PLAINTEXTS, slots, 2) and np.isfinite(z).all(), "case %s: the inputs must keep every output finite" % case_name(case)
    return {"seed": case_seed(case), "logn": logn, "slots": slots, "W": W, "nu": float(nu).hex(), "sha256": sha(z)}


def dcd_record():
    """the whole record, from the executed reference (needs oracle/_ref/)"""
    got = ref.run(ref_decode, [(c[0], c[1], c[3], case_plaintexts(c)) for c in CASES], workers=4)
    return json.loads(json.dumps({"_provenance": "Outputs of the GPQHE reference's he_dcd, executed on the seeded plaintexts of tests/dcd_record.py: sha256 of the "
                                  "64-bit patterns of the doubles, [8][slots][2] (re, im). Data only; tests/test_ref_dcd.py recomputes and compares.",
                                  "cases": {case_name(c): case_record(c, g) for c, g in zip(CASES, got)}}))


def dcd_golden():
    with open(DCD_JSON) as f:
        return json.load(f)


def model_doubles(case, T, **variant):
    """the model's [8][slots][2] doubles for a case with the table T"""
    logn, slots, W, nu = case
    return dcd_model.decode(case_plaintexts(case), T, slots, nu, **variant)


if __name__ == "__main__":
    rec = dcd_record()
    with open(DCD_JSON, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(DCD_JSON, ROOT))
