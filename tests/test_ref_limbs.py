"""Limb level: ntt / invntt / poly_rns_mul / poly_rns_add / montgomery_* / barrett_* of the EXECUTED reference against the oracle.

First, middle and last prime of the chain at logn 1, 2, 3, 7, 10, 12, 13, 14, 16, 17: seeded uniform limbs, every case of
tests/zero_cases.py (the reference stores p for a residue 0 on the sum leg, src/ntt.c:47: each such word must be reproduced), p and
p - 1 throughout, and non-canonical 64-bit words -- the domain gpq_ntt_reference claims, wrap-around included.  Every comparison is
equality of words.  The digests tests/golden/survey_8c.json stores are regenerated from the executed reference as well."""
import numpy as np
import pytest

from oracle import ref
from tests import ref_jobs

# logq only sizes the chain (dimub); inside logn 10..15 the reference takes its table's bound whatever q is
LIMBS = [(1, 120), (2, 120), (3, 120), (7, 61), (10, 27), (12, 109), (13, 218), (14, 438), (16, 120), (17, 120)]


@pytest.fixture(scope="module")
def limb_results():
    ref_jobs.require_reference()
    return dict(zip(LIMBS, ref.run(ref_jobs.check_limbs, [(logn, logq, 1000 + logn) for logn, logq in LIMBS], workers=8)))


@pytest.mark.parametrize("logn,logq", LIMBS)
def test_limb_functions_equal_the_oracle(limb_results, logn, logq):
    r = limb_results[(logn, logq)]
    assert r["diffs"] == []
    assert r["compared"] >= 190                                       # five operations, at least 19 inputs, at least two primes
    if logn >= 2:
        assert r["seen_p"] > 0, "no zero case made the reference store p: the cases do not reach src/ntt.c:47"


EDGE = lambda p: [0, 1, 2, p - 2, p - 1, p, p + 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - p, 2 * p, 3 * p - 1]


@pytest.mark.parametrize("logn,logq,d", [(7, 61, 0), (7, 61, 4), (13, 218, 7), (16, 850, 57)])
def test_reduce_functions_against_exact_integers(oracle_ctx, logn, logq, d):
    """montgomery_reduce(a b) = a b 2^-64 and barrett_reduce(a b) = a b mod p for canonical a, b (the edge list of test_reduce_edge_cases and
    10^5 seeded pairs); barrett_reduce(a + b) for ANY two words (poly_rns_add's use, src/poly.c:75); the oracle's slab operations agree"""
    ref_jobs.require_reference()
    o = oracle_ctx(logn, d + 1)
    p = o.p[d]
    rng = np.random.default_rng(logn * 100 + d)
    vals = [0, 1, p - 1, p - 2] + [int(v) % p for v in rng.integers(0, 2 ** 63, 32, dtype=np.uint64)]
    pairs = [(a, b) for a in vals for b in (0, 1, p - 1, vals[-1])]
    pairs += list(zip(rng.integers(0, p, 100000, dtype=np.uint64).tolist(), rng.integers(0, p, 100000, dtype=np.uint64).tolist()))
    prods = [a * b for a, b in pairs]
    lo = np.array([v & 0xFFFFFFFFFFFFFFFF for v in prods], dtype=np.uint64)
    hi = np.array([v >> 64 for v in prods], dtype=np.uint64)
    words = EDGE(p) + rng.integers(0, 1 << 64, 2000, dtype=np.uint64).tolist()
    sums = [a + b for a in words[:40] for b in words[:40]] + [a + b for a, b in zip(words[40:], words[41:])]
    slo = np.array([v & 0xFFFFFFFFFFFFFFFF for v in sums], dtype=np.uint64)
    shi = np.array([v >> 64 for v in sums], dtype=np.uint64)
    r, s = ref.run(ref_jobs.reduce_values, [(logn, logq, d, lo, hi), (logn, logq, d, slo, shi)], workers=2)
    assert r["node"]["p"] == p
    assert r["mont_inv"] == r["node"]["pinv_mont"] == o.const("pinv_mont", d) and r["barr_inv"] == r["node"]["pinv_barr"] == o.const("pinv_barr", d)
    Rinv = pow(1 << 64, -1, p)
    assert r["barr"].tolist() == [v % p for v in prods]
    assert r["mont"].tolist() == [v * Rinv % p for v in prods]
    # sums of arbitrary words: congruent, below 2^64, and what the oracle's poly_rns_add gives (n words at a time)
    got = s["barr"].tolist()
    assert all(g % p == v % p for g, v in zip(got, sums))
    n = o.n
    a = np.array([x for x in words[:40] for _ in range(40)] + words[40:-1], dtype=np.uint64)
    b = np.array([y for _ in range(40) for y in words[:40]] + words[41:], dtype=np.uint64)
    pad = (-len(a)) % n
    a, b = np.concatenate([a, np.zeros(pad, np.uint64)]), np.concatenate([b, np.zeros(pad, np.uint64)])
    want = np.concatenate([o.rns_add(a[k:k + n], b[k:k + n], d) for k in range(0, len(a), n)])[:len(got)]
    assert got == want.tolist()


@pytest.mark.parametrize("logn", ["7", "12", "15", "16", "17"])
def test_survey_digests_regenerated_from_the_executed_reference(golden, logn):
    """every value tests/golden/survey_8c.json holds for this ring, computed again by the reference built here; the JSON is not edited"""
    ref_jobs.require_reference()
    rec = golden["prime_chain"][logn]
    kat = golden["he_mul_core_kat"].get(logn)
    arg = (int(logn), rec["logq"], rec["count"], (kat["dA"], kat["dB"], golden["he_mul_core_kat"]["_seeds"]) if kat else None)
    out, = ref.run(ref_jobs.survey_digests, [arg], workers=1)
    assert out["count"] == rec["count"] and out["first"][:len(rec["first"])] == rec["first"] and str(out["xor_all"]) == rec["xor_all"]
    k = golden["p0_constants"][logn]
    assert (str(out["node0"]["pinv_mont"]), str(out["node0"]["pinv_barr"]), str(out["node0"]["ninv"])) == (k["pinv_mont"], k["pinv_barr"], k["ninv"])
    assert out["zetas"] == (k["zetas_n_2"], k["zetas_1"], k["zetas_inv_1"])
    if logn == "7":
        assert out["phat_invmp"] == golden["phat_invmp_logn7"]
    nk = golden["ntt_kat_seed1_limb0"][logn]
    assert out["ntt"] == {"input": nk["input"], "ntt": nk["ntt"], "out012": nk["out012"], "back": True}
    if kat:
        assert out["kat"] == {"inputs": kat["inputs"], "d0": kat["d0"], "d1": kat["d1"], "d2": kat["d2"], "c0": kat["c0"], "c1": kat["c1"]}
