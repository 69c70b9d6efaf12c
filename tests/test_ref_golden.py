"""tests/golden/ref_parity.json is what the EXECUTED reference computes: the record the GPU module (tests/test_ref_parity_gpu.py) compares the
device with where the reference cannot be built.  Recomputed here from oracle/_ref/ and compared key by key, so the file cannot drift from the
execution; `python -m tests.ref_record` rewrites it.  Also: the restatement reproduces the same record, so file, oracle and reference agree."""
from oracle import bigint_ref as br
from oracle.expect import ints_to_words
from tests import ref_jobs, ref_record


def test_stored_record_is_the_executed_references():
    ref_jobs.require_reference()
    live, stored = ref_record.parity_record(), ref_record.parity_golden()
    assert sorted(live) == sorted(stored)
    for part in ("ntt", "functions", "default"):
        assert live[part] == stored[part], part


def test_stored_record_is_complete_and_reproduced_by_the_restatement(oracle_ctx):
    """needs no reference: every case of the GPU module is in the file, and the oracle's he_mul / ntt give the stored digests"""
    stored = ref_record.parity_golden()
    assert sorted(stored["ntt"]) == sorted("%d_%d_%d" % c for c in ref_record.NTT_CASES)
    assert len(stored["functions"]) == len(ref_record.PARITY_SHAPES) and all(len(s) == ref_record.PARITY_BATCH for s in stored["functions"])
    for logn, logq, dim in ref_record.NTT_CASES[:2]:
        e = stored["ntt"]["%d_%d_%d" % (logn, logq, dim)]
        names, cases, wild = ref_jobs.ntt_inputs(logn, dim, 700 + logn)
        o = oracle_ctx(logn, dim)
        assert [str(p) for p in o.p[:dim]] == e["primes"]
        fwd = o.ntt_slab(cases, dim)
        per = dim * o.n
        assert [ref_record.sha(fwd[k * per:(k + 1) * per]) for k in range(len(names))] == e["case_ntt"]
        assert ref_record.sha(o.ntt_slab(wild, dim)) == e["wild_ntt"] and ref_record.sha(o.ntt_slab(wild, dim, inverse=True)) == e["wild_invntt"]
    a = ref_record.PARITY_SHAPES[0]
    t = ref_record.parity_tasks(a)[1]
    rec = stored["functions"][0][1]
    ins = ref_jobs.functions_inputs(dict(t, dimub=rec["ctx"]["dimub"]))
    o, n, W = ins["o"], 1 << a["logn"], a["logq"] // 64 + 1
    dimP, dimA, dimB, dimevk = br.he_dims(a["logn"], o.p, a["logq"], a["logq"])
    assert (dimP, dimevk) == (rec["ctx"]["dim"], rec["ctx"]["dimevk"])
    e0, e1 = br.he_mul(o, ins["ct1"], ins["ct2"], ins["rlk"][0][:dimB * n], ins["rlk"][1][:dimB * n], dimP, dimA, dimB, a["logq"])
    assert [ref_record.sha(ints_to_words(e0, W)), ref_record.sha(ints_to_words(e1, W))] == rec["out"]["he_mul"][:2]
    assert all(len(d) <= 2 * a["slots"] for d in stored["functions"][0][0]["diags"]) and "diags" not in rec


def test_stored_host_digests_are_the_executed_references():
    """tests/golden/ref_hosts.json: the reference's side of `mpi_host` and `gemv_host` (mode refonly: the reference alone, no device) and the
    plaintexts its he_ecd makes of gemv_host's diagonal vectors, recomputed here"""
    ref_jobs.require_reference()
    live, stored = ref_record.hosts_record(), ref_record.hosts_golden()
    assert live["mpi_host"] == stored["mpi_host"] and live["gemv_host"] == stored["gemv_host"]
    for shape, lines in stored["mpi_host"].items():
        assert len(lines) == 18 and [w for w, _ in lines].count("he_mul of a ciphertext with itself, in place") == 1, shape
    for shape, rec in stored["gemv_host"].items():
        assert [w for w, _ in rec["ref"]][:2] == ["he_gemv", "he_sum"] and len(rec["ref"]) == 6 and rec["ecd"], shape
