"""The record of the executed reference: what tests/test_ref_parity_gpu.py compares the device with on every machine.

tests/golden/ref_parity.json -- sha256 of every output slab the reference computes for the GPU module's seeded inputs, the context dims, the
plaintexts its he_ecd makes of the gemv diagonals; tests/golden/ref_hosts.json -- the digests the reference's side of `mpi_host` / `gemv_host`
prints (`refonly`: the reference alone, no device) and gemv_host's he_ecd table.  Both are written by `python -m tests.ref_record` from
oracle/_ref/ and recomputed and compared by tests/test_ref_golden.py wherever the reference can be built."""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

from oracle import ref
from tests.ref_jobs import ROOT, functions_run, ntt_slabs

# tests/test_ref_parity_gpu.py runs where the reference checkout (and so oracle/_ref/) may not exist.  What the executed reference
# computes for that module's seeded inputs is therefore also kept as data, tests/golden/ref_parity.json: sha256 of every expected
# output slab, the context dims, and the plaintexts the reference's he_ecd made of the gemv diagonals (sparse).
# tests/test_ref_golden.py recomputes the whole record from the executed reference and asserts equality, so the file cannot drift;
# `python -m tests.ref_record` rewrites it.

PARITY_JSON = os.path.join(ROOT, "tests", "golden", "ref_parity.json")
NTT_CASES = [(10, 27, 3), (13, 218, 4), (14, 438, 4), (17, 120, 3)]
PARITY_BATCH = 3
PARITY_SHAPES = [dict(logn=9, logq=120, logdelta=30, slots=4, seed=31),
                 dict(logn=9, logq=120, logdelta=30, slots=8, seed=32, matrix="zero diagonals"),
                 dict(logn=13, logq=200, logdelta=40, slots=2, seed=33)]
PARITY_ONLY = ["poly_mul", "he_mulpt", "he_mul", "he_rot", "he_gemv"]
PARITY_DEFAULT = dict(logn=14, logq=438, logdelta=50, slots=16, seed=41, only=["he_mul", "he_rot"])


def sha(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint64).tobytes()).hexdigest()


def parity_tasks(a):
    return [dict(a, ctseed=1000 * a["seed"] + b, only=PARITY_ONLY) for b in range(PARITY_BATCH)]


def ntt_record(arg):
    e = ntt_slabs(arg + (700 + arg[0],))
    n, dim = 1 << arg[0], arg[2]
    per = dim * n
    return {"primes": [str(p) for p in e["primes"]], "names": list(e["names"]),
            "case_ntt": [sha(e["cases_ntt"][k * per:(k + 1) * per]) for k in range(len(e["names"]))],
            "stored_p": int(sum((e["cases_ntt"].reshape(-1, n)[i] == np.uint64(e["primes"][i % dim])).sum() for i in range(e["cases_ntt"].size // n))),
            "wild_ntt": sha(e["wild_ntt"]), "wild_invntt": sha(e["wild_invntt"]), "inverse_undoes_p": bool(np.array_equal(e["cases_ntt_invntt"], e["cases"]))}


def functions_record(a):
    from oracle.expect import ints_to_words
    got = functions_run(a)
    W = a["logq"] // 64 + 1
    rec = {"ctx": {k: got["_ctx"][k] for k in ("dim", "dimevk", "dimub", "L")},
           "out": {k: [sha(ints_to_words(v[0][0], W)), sha(ints_to_words(v[0][1], W)), v[1]] for k, v in got.items() if not k.startswith("_")}}
    if "_poly_mul" in got:
        rec["poly_mul"] = sha(ints_to_words(got["_poly_mul"], W))
    if "_diags" in got:
        rec["diags"] = [[[i, str(v)] for i, v in enumerate(d) if v] for d in got["_diags"]]
    return rec


def parity_record():
    """the whole record, from the executed reference (needs oracle/_ref/)"""
    ntt = ref.run(ntt_record, NTT_CASES, workers=4)
    funcs = [ref.run(functions_record, parity_tasks(a), workers=PARITY_BATCH) for a in PARITY_SHAPES]
    for recs in funcs:                                    # the diagonals belong to the shape, not to the ciphertext: kept with the first only
        assert all(r["diags"] == recs[0]["diags"] for r in recs)
        for r in recs[1:]:
            del r["diags"]
    default, = ref.run(functions_record, [PARITY_DEFAULT], workers=1)
    return json.loads(json.dumps({"_provenance": "Outputs of the GPQHE reference executed on the seeded inputs of tests/test_ref_parity_gpu.py (sha256 of the uint64 "
                                  "slabs, little-endian; big slabs [W][n] with W = logq // 64 + 1). Data only; tests/test_ref_golden.py recomputes and compares.",
                                  "ntt": {"%d_%d_%d" % c: r for c, r in zip(NTT_CASES, ntt)}, "functions": funcs, "default": default}))


def parity_golden():
    with open(PARITY_JSON) as f:
        return json.load(f)


def parity_expected():
    """what the GPU module compares with: the executed reference where oracle/_ref/ is there (and then the stored record must equal it), the
    stored record of the executed reference otherwise"""
    stored = parity_golden()
    if ref.available():
        live = parity_record()
        assert live == stored, "tests/golden/ref_parity.json is not what the executed reference computes: python -m tests.ref_record rewrites it"
        return live
    return stored


def diag_ints(sparse, n):
    v = [0] * n
    for i, x in sparse:
        v[i] = int(x)
    return v


# ---------------------------------------------------------------------------
# the C hosts
# ---------------------------------------------------------------------------
HOSTS_JSON = os.path.join(ROOT, "tests", "golden", "ref_hosts.json")
MPI_HOST_SHAPES = [(9, 120, 30), (8, 177, 59), (13, 200, 40)]          # logn, logq, logDelta
GEMV_HOST_SHAPES = [(9, 120, 1), (9, 120, 2), (8, 120, 8), (9, 120, 16)]  # logn, logq, slots


def build_host(name, outdir):
    """tests/c/<name>.c linked against the built library (loading it needs no device)"""
    out, lib_dir = os.path.join(outdir, name), os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", name + ".c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-ldl", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def digest_lines(stdout, side):
    """[[what, digest]] of the `lib <what> <16 hex digits>` / `ref ..` lines a host printed"""
    import re
    return [[m.group(1), m.group(2)] for m in (re.fullmatch(side + r" (.+) ([0-9a-f]{16})", ln) for ln in stdout.splitlines()) if m]


def mpi_host_args(shape):
    return [str(v) for v in shape] + [str(900 + shape[0])]


def hosts_record():
    """the reference's side of both hosts, run alone on the CPU (needs oracle/_ref/ and the built library)"""
    out = {"_provenance": "What the GPQHE reference computes in `tests/c/mpi_host.c refonly` and `tests/c/gemv_host.c refonly` (FNV-1a-64 over l, the bits "
           "of nu and B and every coefficient in hex), and the plaintexts its he_ecd makes of gemv_host's diagonal vectors. Data only; "
           "tests/test_ref_golden.py recomputes and compares.", "mpi_host": {}, "gemv_host": {}}
    with tempfile.TemporaryDirectory() as td:
        mpi, gemv = build_host("mpi_host", td), build_host("gemv_host", td)
        for shape in MPI_HOST_SHAPES:
            res = subprocess.run([mpi, "refonly", ref.which()] + mpi_host_args(shape), capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-1000:]
            out["mpi_host"]["%d_%d_%d" % shape] = digest_lines(res.stdout, "ref")
        for shape in GEMV_HOST_SHAPES:
            res = subprocess.run([gemv, "refonly", ref.which()] + [str(v) for v in shape], capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-1000:]
            out["gemv_host"]["%d_%d_%d" % shape] = {"ref": digest_lines(res.stdout, "ref"),
                                                    "ecd": sorted({ln for ln in res.stdout.splitlines() if ln.startswith("ecd ")})}
    return out


def hosts_golden():
    with open(HOSTS_JSON) as f:
        return json.load(f)


if __name__ == "__main__":
    for _path, _rec in ((PARITY_JSON, parity_record()), (HOSTS_JSON, hosts_record())):
        with open(_path, "w") as _f:
            json.dump(_rec, _f, indent=0, sort_keys=True)
            _f.write("\n")
        print("wrote", os.path.relpath(_path, ROOT))
