"""The record of the executed reference's he_ecd: what tests/test_he_ecd_gpu.py compares the device encoder with on every machine.

tests/golden/ref_ecd.json -- per case the seed, the parameters, sha256 of the expected big slab (six vectors, [6][W][n] uint64) and the
largest coefficient in bits; tests/golden/ref_ecd_roots512.npy -- the root table T[t] = (cos, sin)(2 pi t / 2048) the reference held when
the record was made (its polyctx.ring.zetas by stride), 2049 x 2 doubles, which serves every case by stride.  Both are written by
`python -m tests.ecd_record` from oracle/_ref/; tests/test_ref_ecd.py recomputes the record wherever the reference can be built and holds
the numpy model (tests/ecd_model.py) against it."""
import hashlib
import json
import os

import numpy as np

from oracle import ref
from tests import ecd_model
from tests.ref_jobs import ROOT

ECD_JSON = os.path.join(ROOT, "tests", "golden", "ref_ecd.json")
ROOTS_NPY = os.path.join(ROOT, "tests", "golden", "ref_ecd_roots512.npy")
ROOTS_SLOTS = 512
LOGQ = {10: 27, 11: 54, 12: 109}                         # of the reference context only (he_ecd does not read q): the cap of src/precomp.c:57-64, else 120
# logn, slots, logDelta, W
CASES = [(7, 1, 30, 1), (7, 2, 30, 2), (7, 4, 30, 1), (9, 16, 20, 2), (9, 64, 30, 7), (8, 128, 20, 1), (10, 512, 20, 1), (13, 64, 40, 1)]
LARGE = [(12, 2048, 30), (13, 4096, 30), (14, 8192, 30)]  # live only (tests/test_ref_ecd.py): the capacity edge and the two sizes below it
MAX_BITS = 62                                            # a condition on the INPUTS below: every coefficient stays inside |v| < 2^63 with room


def case_name(case):
    return "%d_%d_%d_%d" % tuple(case)


def case_seed(case):
    logn, slots, logDelta, W = case
    return 7000 + 100 * logn + slots + logDelta


def case_vectors(case):
    """the six vectors of a case, [6][slots] complex128: uniform with |re|, |im| <= 2^(60 - logDelta) (coefficients of 59-61 bits: what a
    contracted butterfly gets wrong), a unit vector, a constant vector, zeros, and the two exact ties (2.5 - 1.5i) / Delta and
    (-0.5 + 0.5i) / Delta (constant vectors: coefficient 0 is the tie itself)"""
    logn, slots, logDelta, W = case
    rng = np.random.default_rng(case_seed(case))
    big = 2.0 ** (60 - logDelta)
    z = np.zeros((6, slots), dtype=np.complex128)
    z[0] = rng.uniform(-big, big, slots) + 1j * rng.uniform(-big, big, slots)
    z[1, slots // 3] = big * (0.75 - 0.5j)
    z[2] = big * (-0.625 + 0.875j)
    z[4] = (2.5 - 1.5j) / 2.0 ** logDelta
    z[5] = (-0.5 + 0.5j) / 2.0 ** logDelta
    return z


def large_vectors(case):
    logn, slots, logDelta = case
    rng = np.random.default_rng(9000 + slots)
    big = 2.0 ** (60 - logDelta)
    z = np.zeros((2, slots), dtype=np.complex128)
    z[0] = rng.uniform(-big, big, slots) + 1j * rng.uniform(-big, big, slots)
    z[1] = (2.5 - 1.5j) / 2.0 ** logDelta
    return z


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def ref_encode(arg):
    """worker job: (logn, slots, logDelta, vectors) -> int64 [count][n] by the executed reference (he_ecd + the plaintext read back)"""
    logn, slots, logDelta, z = arg
    R = ref.Ref().init(logn, 1 << LOGQ.get(logn, 120), slots, 1 << logDelta)
    out = np.empty((len(z), R.n), dtype=np.int64)
    for k, v in enumerate(z):
        R.he_ecd(1, v)
        m, nu = R.pt_get(1, W=2)
        assert nu == float(1 << logDelta)
        out[k] = m                                        # (raises if a coefficient does not fit an int64)
    return out


def case_record(case, coeffs):
    logn, slots, logDelta, W = case
    bits = ecd_model.max_bits(coeffs)
    assert bits <= MAX_BITS, "case %s: coefficients of %d bits: the inputs must stay at or below %d" % (case_name(case), bits, MAX_BITS)
    return {"seed": case_seed(case), "logn": logn, "slots": slots, "logDelta": logDelta, "W": W, "sha256": sha(ecd_model.words(coeffs, W)), "max_bits": bits}


def ecd_record():
    """the whole record, from the executed reference (needs oracle/_ref/)"""
    got = ref.run(ref_encode, [(c[0], c[1], c[2], case_vectors(c)) for c in CASES], workers=4)
    return json.loads(json.dumps({"_provenance": "Plaintexts of the GPQHE reference's he_ecd, executed on the seeded vectors of tests/ecd_record.py: sha256 of "
                                  "the big slab uint64 [6][W][n] (little-endian words, sign-extended). Data only; tests/test_ref_ecd.py recomputes and compares.",
                                  "cases": {case_name(c): case_record(c, g) for c, g in zip(CASES, got)}}))


def ecd_golden():
    with open(ECD_JSON) as f:
        return json.load(f)


def stored_roots():
    T = np.load(ROOTS_NPY)
    assert T.shape == (4 * ROOTS_SLOTS + 1, 2) and T.dtype == np.float64
    return T


def model_words(case, T):
    """the model's slab for a case with the table T, and what it counts as offending"""
    logn, slots, logDelta, W = case
    coeffs, offending = ecd_model.encode(case_vectors(case), T, 1 << logn, logDelta)
    return ecd_model.words(coeffs, W), offending


if __name__ == "__main__":
    rec = ecd_record()
    with open(ECD_JSON, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    np.save(ROOTS_NPY, ecd_model.roots_via_sincos(ROOTS_SLOTS))
    for path in (ECD_JSON, ROOTS_NPY):
        print("wrote", os.path.relpath(path, ROOT))
