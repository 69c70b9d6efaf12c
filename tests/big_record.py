"""The record of the executed reference's he_ecd and he_dcd above 8192 slots: what tests/test_he_ecd_big_gpu.py and
tests/test_he_dcd_big_gpu.py compare the device with wherever this machine's sincos table is the recorded one.

tests/golden/ref_ecd_big.json, tests/golden/ref_dcd_big.json -- per case the seed, the parameters, sha256 of the expected big slab
([3][W][n] uint64) or of the 64-bit patterns of the output doubles ([3][slots][2]), and sha256 of the root table
T[t] = (cos, sin)(2 pi t / (4 slots)) under which the numpy model (tests/ecd_model.py, tests/dcd_model.py) equalled the executed
reference when the record was made.  No table is stored: 4 slots + 1 roots are 4 MiB at 65536 slots.  A checkout without the reference
checks the model against the record whenever its own `roots_via_sincos` table has the recorded digest (tests/test_ref_ecd_big.py,
tests/test_ref_dcd_big.py, which recompute the record wherever the reference can be built).  Written by `python -m tests.big_record`
from oracle/_ref/."""
import functools
import hashlib
import json
import os
import random

import numpy as np

from oracle import ref
from tests import dcd_model, dcd_record, ecd_model, ecd_record
from tests.ref_jobs import ROOT

ECD_JSON = os.path.join(ROOT, "tests", "golden", "ref_ecd_big.json")
DCD_JSON = os.path.join(ROOT, "tests", "golden", "ref_dcd_big.json")
# logn, slots, logDelta, W  (the last: gap = 2)
ECD_CASES = [(15, 16384, 30, 2), (16, 32768, 30, 1), (17, 65536, 30, 1), (16, 16384, 30, 1)]
# logn, slots, nu  (one nu that is no power of two; the device tests run W = 1 and W = 2 on the same coefficients)
DCD_CASES = [(15, 16384, 2.0 ** 30), (16, 32768, 3.0 * 2 ** 29 + 1), (17, 65536, 2.0 ** 30)]
COUNT = 3
MIN_BITS, MAX_BITS = 58, 62                              # a condition on the INPUTS: the largest coefficient of each uniform vector


def ecd_name(case):
    return "%d_%d_%d_%d" % tuple(case)


def dcd_name(case):
    return "%d_%d_%s" % (case[0], case[1], float(case[2]).hex())


def ecd_seed(case):
    logn, slots, logDelta, W = case
    return 16000 + 100 * logn + slots + logDelta


def dcd_seed(case):
    logn, slots, nu = case
    return 17000 + 100 * logn + slots


@functools.lru_cache(maxsize=None)
def roots(slots):
    """this machine's sincos table for `slots` slots, made once per process"""
    T = ecd_model.roots_via_sincos(slots)
    T.setflags(write=False)
    return T


def roots_sha(T):
    return hashlib.sha256(np.ascontiguousarray(T, dtype=np.float64).tobytes()).hexdigest()


def ecd_vectors(case):
    """[3][slots] complex128: two uniform vectors and the exact tie (2.5 - 1.5i) / Delta (a constant vector: coefficient 0 is the tie
    itself).  A coefficient of a uniform vector with |re|, |im| <= a is a mean of `slots` terms, about a / sqrt(3 slots) in size and 4 to
    5 times that at its largest, so the amplitude grows with sqrt(slots): a = 2^(59 - logDelta) sqrt(slots) puts the largest coefficient
    at 60-61 bits, 3/8 of it at 59-60 (MIN_BITS..MAX_BITS is asserted on what comes out) -- where a contracted butterfly changes words.
    ecd_record.large_vectors' fixed 2^(60 - logDelta) gives 54-55 bits at these sizes."""
    logn, slots, logDelta, W = case
    rng = np.random.default_rng(ecd_seed(case))
    a = 2.0 ** (59 - logDelta) * float(np.sqrt(float(slots)))
    z = np.zeros((COUNT, slots), dtype=np.complex128)
    z[0] = rng.uniform(-a, a, slots) + 1j * rng.uniform(-a, a, slots)
    z[1] = 0.375 * (rng.uniform(-a, a, slots) + 1j * rng.uniform(-a, a, slots))
    z[2] = (2.5 - 1.5j) / 2.0 ** logDelta
    return z


def dcd_plaintexts(case):
    """[3][n] Python integers, EVERY coefficient filled: dcd_record.large_plaintexts' signed values of 54-62 bits (a second seed for the
    third plaintext) and its pattern54 polynomial, laid out so that the slots the decoder reads see every pattern whatever the gap"""
    logn, slots, nu = case
    n, gap = 1 << logn, (1 << logn) // 2 // slots
    rng = random.Random(dcd_seed(case))
    pat = [dcd_record.pattern54((i // gap) & 1, ((i // gap) >> 1) & 1, (1, -1)[((i // gap) >> 2) & 1]) for i in range(n)]
    return [[dcd_record._signed(rng, 54, 62) for _ in range(n)], pat, [dcd_record._signed(rng, 54, 62) for _ in range(n)]]


def int64_words(coeffs, W):
    """[count][n] integers below 2^63 in magnitude -> the big slab uint64 [count][W][n] (dcd_model.words without its Python loops)"""
    return ecd_model.words(np.array(coeffs, dtype=np.int64), W)


def sha_words(a):
    return ecd_record.sha(a)


def sha_doubles(z):
    return dcd_record.sha(z)


@functools.lru_cache(maxsize=None)
def ecd_model_coeffs(case):
    """the model on this machine's table: (int64 [3][n], offending); computed once per process and not to be written to"""
    logn, slots, logDelta, W = case
    coeffs, offending = ecd_model.encode(ecd_vectors(case), roots(slots), 1 << logn, logDelta)
    coeffs.setflags(write=False)
    return coeffs, offending


@functools.lru_cache(maxsize=None)
def dcd_model_doubles(case):
    """the model on this machine's table: float64 [3][slots][2]; computed once per process and not to be written to"""
    logn, slots, nu = case
    z = dcd_model.decode(dcd_plaintexts(case), roots(slots), slots, nu)
    z.setflags(write=False)
    return z


def ref_encode(arg):
    """worker job of ecd_record.ref_encode's shape: (case, vectors) -> int64 [count][n] by the executed reference"""
    case, z = arg
    return ecd_record.ref_encode((case[0], case[1], case[2], z))


def ref_decode(arg):
    """worker job: (case, plaintexts) -> float64 [count][slots][2] by the executed reference's he_dcd"""
    case, plaintexts = arg
    return dcd_record.ref_decode((case[0], case[1], case[2], plaintexts))


def ecd_case_record(case, coeffs, T):
    logn, slots, logDelta, W = case
    bits = [ecd_model.max_bits(coeffs[k]) for k in range(2)]
    assert all(MIN_BITS <= b <= MAX_BITS for b in bits), "case %s: the uniform vectors' largest coefficients have %s bits: the inputs must give %d..%d" % (
        ecd_name(case), bits, MIN_BITS, MAX_BITS)
    return {"seed": ecd_seed(case), "logn": logn, "slots": slots, "logDelta": logDelta, "W": W, "sha256": sha_words(ecd_model.words(coeffs, W)),
            "max_bits": bits, "roots_sha256": roots_sha(T)}


def dcd_case_record(case, z, T):
    logn, slots, nu = case
    assert z.shape == (COUNT, slots, 2) and np.isfinite(z).all()
    return {"seed": dcd_seed(case), "logn": logn, "slots": slots, "nu": float(nu).hex(), "sha256": sha_doubles(z), "roots_sha256": roots_sha(T)}


def live_ecd():
    """the executed reference on every encoder case (needs oracle/_ref/)"""
    return ref.run(ref_encode, [(c, ecd_vectors(c)) for c in ECD_CASES], workers=4)


def live_dcd():
    return ref.run(ref_decode, [(c, dcd_plaintexts(c)) for c in DCD_CASES], workers=3)


def ecd_big_record(got):
    return json.loads(json.dumps({"_provenance": "Plaintexts of the GPQHE reference's he_ecd, executed on the seeded vectors of tests/big_record.py: sha256 of the big "
                                  "slab uint64 [3][W][n] (little-endian words, sign-extended) and of the root table (float64 [4 slots + 1][2]) under which the "
                                  "numpy model gives the same words. Data only; tests/test_ref_ecd_big.py recomputes and compares.",
                                  "cases": {ecd_name(c): ecd_case_record(c, g, roots(c[1])) for c, g in zip(ECD_CASES, got)}}))


def dcd_big_record(got):
    return json.loads(json.dumps({"_provenance": "Outputs of the GPQHE reference's he_dcd, executed on the seeded plaintexts of tests/big_record.py: sha256 of the "
                                  "64-bit patterns of the doubles, [3][slots][2] (re, im), and of the root table (float64 [4 slots + 1][2]) under which the "
                                  "numpy model gives the same doubles. Data only; tests/test_ref_dcd_big.py recomputes and compares.",
                                  "cases": {dcd_name(c): dcd_case_record(c, g, roots(c[1])) for c, g in zip(DCD_CASES, got)}}))


def golden(path):
    with open(path) as f:
        return json.load(f)


if __name__ == "__main__":
    got_e, got_d = live_ecd(), live_dcd()
    for c, g in zip(ECD_CASES, got_e):
        assert np.array_equal(g, ecd_model_coeffs(c)[0]), "encoder case %s: the model on this machine's table is not the reference" % ecd_name(c)
    for c, g in zip(DCD_CASES, got_d):
        assert np.array_equal(dcd_model.bits(g), dcd_model.bits(dcd_model_doubles(c))), "decoder case %s: the model on this machine's table is not the reference" % dcd_name(c)
    for path, rec in ((ECD_JSON, ecd_big_record(got_e)), (DCD_JSON, dcd_big_record(got_d))):
        with open(path, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", os.path.relpath(path, ROOT))
