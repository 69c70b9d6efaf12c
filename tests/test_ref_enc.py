"""The model of the samplers and the encryptor (tests/enc_model.py) against the EXECUTED reference, and against its stored record.

Where oracle/_ref/ exists the model must equal the reference word for word on every recorded call -- sample_zo, sample_error and
sample_uniform alone, then he_keypair, he_enc_sk, he_enc_pk and he_dec of both ciphertexts in one run -- the bytes each call consumes must
be the documented counts, and the stored record (tests/golden/ref_enc.json, ref_enc_stream.npy) must be what the reference computes here.
On a bare checkout the model on the STORED stream must reproduce the stored record.  The Gaussian pair table of the library
(gpq_sample_error_table, host only) must be the model's and the recorded one on every machine.  No GPU."""
import numpy as np
import pytest

from oracle import ref
from tests import enc_model, enc_record
from tests.ref_jobs import require_reference


@pytest.fixture(scope="module")
def live():
    require_reference()
    jobs = [(kind, logn, logq) for logn, logq in enc_record.CASES for kind in enc_record.KINDS]
    stream, = ref.run(enc_record.ref_stream, [enc_record.STREAM_BYTES], workers=1)
    got = ref.run(enc_record.ref_run, jobs, workers=8)
    k = len(enc_record.KINDS)
    return stream, {case: dict(zip(enc_record.KINDS, got[i * k:(i + 1) * k])) for i, case in enumerate(enc_record.CASES)}


@pytest.fixture(scope="module")
def modelled():
    """the model on the stored stream, once"""
    stream = enc_record.stored_stream()
    return stream, {case: {kind: enc_record.model_run(kind, case, stream) for kind in enc_record.KINDS} for case in enc_record.CASES}


def _compare(got, exp, what):
    for name, v in got.items():
        if name == "ct":
            continue
        e = exp[name]
        if name.startswith("probe:"):
            assert np.array_equal(v, e), "%s: the stream is at another position after %s" % (what, name[6:])
        else:
            bad = [i for i, (x, y) in enumerate(zip(v, e)) if int(x) != int(y)]
            assert not bad and len(v) == len(e), "%s %s: %d coefficients differ from the reference, first at %s" % (what, name, len(bad), bad[:3])


def test_model_equals_the_executed_reference(live):
    stream, runs = live
    for case in enc_record.CASES:
        for kind in enc_record.KINDS:
            _compare(runs[case][kind], enc_record.model_run(kind, case, stream), "case %s, %s" % (enc_record.case_name(case), kind))


def _check_counts(case, rec, draws):
    """the stream position after each call against the documented byte counts (`draws` = the 8-byte draws of sample_hwt)"""
    logn, logq = case
    n, nb, P = 1 << logn, (logq + 1) // 8 + 1, enc_record.PROBE
    pos = rec["pos"]
    assert pos["sample_zo"] == n // 4 and pos["sample_error"] == n and pos["sample_uniform"] == n * nb
    assert pos["he_keypair"] == 8 + 8 * draws + n + n * nb                       # sample_sk, sample_error, sample_uniform(q_L)
    assert pos["he_enc_sk"] - pos["he_keypair"] - P == n + n * nb                # sample_error, sample_uniform(q)
    assert pos["he_enc_pk"] - pos["he_enc_sk"] - P == n // 4 + 2 * n             # sample_zo, sample_error, sample_error


def _hwt_draws(case, stream):
    s = enc_model.Stream(stream)
    enc_model.sample_hwt(s, 1 << case[0])
    return (s.pos - 8) // 8


def test_every_call_consumes_the_documented_bytes(live):
    stream, runs = live
    for case in enc_record.CASES:
        draws = _hwt_draws(case, stream)
        assert draws >= 64
        _check_counts(case, enc_record.case_record(case, runs[case], stream), draws)


def test_bookkeeping_of_the_executed_encryptors(live):
    """ct->l = L, ct->nu = max(pt->nu, Delta): src/he-encrypt.c:40-42, :78-80"""
    stream, runs = live
    for logn, logq in enc_record.CASES:
        for l, nu, B in runs[(logn, logq)]["he"]["ct"]:
            assert l == logq // enc_record.LOGDELTA and nu == ref.bits(float(1 << enc_record.LOGDELTA))


def test_stored_record_is_what_the_reference_computes(live):
    stream, runs = live
    assert np.array_equal(stream, enc_record.stored_stream()), "tests/golden/ref_enc_stream.npy is not the executed reference's stream: python -m tests.enc_record rewrites it"
    rec = {enc_record.case_name(c): enc_record.case_record(c, runs[c], stream) for c in enc_record.CASES}
    assert rec == enc_record.enc_golden()["cases"], "tests/golden/ref_enc.json is not what the executed reference computes: python -m tests.enc_record rewrites it"


def test_model_on_the_stored_stream_reproduces_the_stored_record(modelled):
    """what a checkout without the reference has: the record and the stream it was made on"""
    stream, runs = modelled
    stored = enc_record.enc_golden()["cases"]
    assert stream.dtype == np.uint8 and stream.size == enc_record.STREAM_BYTES
    assert sorted(stored) == sorted(enc_record.case_name(c) for c in enc_record.CASES)
    for case in enc_record.CASES:
        rec = enc_record.case_record(case, runs[case], stream)
        assert rec == stored[enc_record.case_name(case)], "case %s: the model on the stored stream does not give the stored record" % enc_record.case_name(case)
        assert set(rec["sha256"]) == set(enc_record.SAMPLERS + enc_record.HE_NAMES)
        _check_counts(case, rec, _hwt_draws(case, stream))
        for kind in enc_record.KINDS:                                       # (the positions the model itself kept are the recorded ones)
            for name, v in runs[case][kind].items():
                if name.startswith("pos:"):
                    assert v == rec["pos"][name[4:]]


def test_the_record_exercises_raw_samples_and_the_undefined_table_entries(modelled):
    stream, runs = modelled
    raw = runs[(7, 120)]["sample_uniform"]["sample_uniform"]
    assert sum(v >= 1 << 120 for v in raw) >= 32 and max(raw) < 1 << 121           # raw, not reduced: about half lie above q
    assert runs[(7, 120)]["he"]["sk_c1"] != runs[(7, 120)]["he"]["p1"]
    first = stream[:128]
    assert (first[1::2] == 0).any(), "the first 128 bytes must hold a zero at an odd position: the b1 = 0 entries are then pinned by sample_error at logn 7"
    for case in enc_record.CASES:                                                # the two keys are 64-sparse, the noise is small, the round trip holds
        he = runs[case]["he"]
        assert sum(1 for v in he["sk"] if v) == 64 and set(he["sk"]) == {-1, 0, 1}
        m = enc_record.case_plaintext(case)
        for name in ("dec_sk", "dec_pk"):
            assert max(abs(a - b) for a, b in zip(he[name], m)) < 1 << 14


def test_library_table_is_the_model_table_and_the_recorded_one():
    import gpqhe_amd
    T, M = gpqhe_amd.sample_error_table(), enc_model.gauss_table()
    assert T.shape == (65536, 2) and T.dtype == np.int8
    bad = np.argwhere(T != M)
    assert not len(bad), "%d entries differ from the model, first (pair, part) %s" % (len(bad), bad[0].tolist())
    assert enc_record.table_sha(T) == enc_record.enc_golden()["gauss_table_sha256"]
    assert not T.reshape(256, 256, 2)[:, 0, :].any()                            # b1 = 0: (0, 0)
    assert T.min() == -11 and T.max() == 11
    assert enc_model.gauss_margin() > 4.0e-5                                    # floor's argument stays clear of the integers: no libm dependence
