"""The device against the EXECUTED reference.

What the reference computes for this module's seeded inputs is "the record" of tests/ref_record.py: sha256 of every output slab, the context
dims, the plaintexts its own he_ecd makes of the gemv diagonals.  Where oracle/_ref/ is there (built by `make -C oracle ref`) the record is
computed by executing the reference, in spawned CPU worker processes, and tests/golden/ref_parity.json must equal it; on a machine that has
neither the reference checkout nor oracle/_ref/ the stored record is used (tests/test_ref_golden.py keeps it equal to the execution wherever
the reference can be built).  Nothing of the slab API skips or fails for want of the reference.  Every comparison is equality of words.
Shapes stay inside what the reference accepts (it caps q on logn 10..15 and aborts above the cap); device shapes beyond a cap stay pinned
through the oracle, which tests/test_ref_functions.py pins to this same reference.

The C hosts at the end compare the MPI-typed symbols the same way: see there."""
import numpy as np
import pytest
import torch

import gpqhe_amd
from gpqhe_amd import to_device, to_host
from oracle import ref
from oracle.expect import ints_to_words
from tests import ref_jobs, ref_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """The executed reference's outputs for this module's seeded inputs (tests/ref_record.py): computed by oracle/_ref/ in CPU worker
    processes where it is there -- and then tests/golden/ref_parity.json must equal it -- and read from that file, which is the same record kept as
    data, where this machine has neither the reference checkout nor oracle/_ref/.  Either way it is the reference's execution, and nothing skips."""
    return ref_record.parity_expected()


def _is(got, digest, what):
    assert ref_record.sha(to_host(got) if hasattr(got, "is_cuda") else got) == digest, "%s: the words differ from the executed reference's (sha256)" % what


# ---------------------------------------------------------------------------
# slab API, transforms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn,logq,dim", ref_record.NTT_CASES)
def test_transforms_equal_the_executed_reference(expected, logn, logq, dim):
    """gpq_ntt / gpq_invntt / gpq_ntt_reference on the zero cases (the reference stores p for a residue 0, src/ntt.c:47) and on
    non-canonical words, for every butterfly class and both non-temporal policies"""
    e = expected["ntt"]["%d_%d_%d" % (logn, logq, dim)]
    names, cases, wild = ref_jobs.ntt_inputs(logn, dim, 700 + logn)
    assert names == e["names"] and e["stored_p"] > 0 and e["inverse_undoes_p"]
    g = gpqhe_amd.PolyContext(logn, dim)                               # its own context: the butterfly classes are changed below
    assert [str(p) for p in g.p[:dim]] == e["primes"]
    n, per = g.n, dim * g.n
    try:
        for wide, split in ((0, 0), (0, 64), (64, 64)):
            for nt in (0, 1):
                g.set_limb_classes(wide, split)
                g.set_nt_policy(nt)
                tag = "classes (%d, %d), nt %d" % (wide, split, nt)
                dev = to_device(cases)
                g.poly_ntt(dev, dim)
                fwd = to_host(dev)
                for k, name in enumerate(names):
                    _is(fwd[k * per:(k + 1) * per], e["case_ntt"][k], "gpq_ntt, %s, %s" % (tag, name))
                # from here on `fwd` IS the reference's output, words p included
                assert int(sum((fwd.reshape(-1, n)[i] == np.uint64(g.p[i % dim])).sum() for i in range(fwd.size // n))) == e["stored_p"]
                canon = np.concatenate([fwd.reshape(-1, n)[i] % np.uint64(g.p[i % dim]) for i in range(fwd.size // n)])
                dev = to_device(canon)                     # gpq_invntt takes canonical words
                g.poly_invntt(dev, dim)
                assert np.array_equal(to_host(dev), cases), tag
                dev = to_device(cases)
                g.poly_ntt_reference(dev, dim)
                assert np.array_equal(to_host(dev), fwd), (tag, "gpq_ntt_reference")
                dev = to_device(fwd)
                g.poly_ntt_reference(dev, dim, inverse=True)          # the reference's own inverse undoes its words p
                assert np.array_equal(to_host(dev), cases), (tag, "gpq_ntt_reference, inverse, input with words p")
                for inverse, key in ((False, "wild_ntt"), (True, "wild_invntt")):
                    dev = to_device(wild)
                    g.poly_ntt_reference(dev, dim, inverse=inverse)
                    _is(dev, e[key], "gpq_ntt_reference on arbitrary words, %s, inverse %s" % (tag, inverse))
    finally:
        torch.cuda.synchronize()
        g.close()


# ---------------------------------------------------------------------------
# slab API, whole functions
# ---------------------------------------------------------------------------
BATCH = ref_record.PARITY_BATCH


def _big(polys, W):
    return to_device(np.concatenate([ints_to_words(p, W) for p in polys]))


def _same(got, recs, name, c, W, n, what):
    """slab of len(recs) big polynomials against the record's digests of component c of result `name`"""
    got = (to_host(got) if hasattr(got, "is_cuda") else got).reshape(len(recs), W * n)
    for b, r in enumerate(recs):
        _is(got[b], r["out"][name][c], "%s, ciphertext %d" % (what, b))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("k", range(len(ref_record.PARITY_SHAPES)))
def test_functions_equal_the_executed_reference(engine_ctx, expected, k):
    """gpq_poly_mul, gpq_he_mulpt, gpq_he_mul, gpq_he_mul_rs, gpq_he_rs, gpq_he_swk, gpq_he_rot_hoisted, gpq_he_gemv, gpq_he_gemv_planned on a
    batch of three with gpq_set_chunk(2): two launch groups, both lanes"""
    a = ref_record.PARITY_SHAPES[k]
    logn, logq, logdelta, slots = a["logn"], a["logq"], a["logdelta"], a["slots"]
    tasks = ref_record.parity_tasks(a)
    exp = expected["functions"][k]
    ctx = exp[0]["ctx"]
    ins = [ref_jobs.functions_inputs(dict(t, dimub=ctx["dimub"])) for t in tasks]
    n, W = 1 << logn, logq // 64 + 1
    g = engine_ctx(logn, ctx["dimub"])
    dimP, dimA, dimB, dimevk = g.he_dims(logq, logq)
    assert (dimP, dimevk) == (ctx["dim"], ctx["dimevk"]) and g.p == [int(p) for p in ins[0]["o"].p]
    assert all(e["out"]["he_mul"][2] == ctx["L"] and e["out"]["he_rs"][2] == ctx["L"] - 1 and e["out"]["he_gemv"][2] == ctx["L"] - 1 for e in exp)
    dimpt = (logq + 1 + logdelta + logn) // 59 + 1
    c10, c11, c20, c21 = [_big([i[c][j] for i in ins], W) for c, j in (("ct1", 0), ("ct1", 1), ("ct2", 0), ("ct2", 1))]
    key = lambda pair: (to_device(pair[0][:dimB * n]), to_device(pair[1][:dimB * n]))
    rlk, rk = key(ins[0]["rlk"]), [key(p) for p in ins[0]["rk"]]
    new = lambda count=BATCH: torch.empty(count * W * n, dtype=torch.int64, device="cuda")
    same = lambda got, name, c, what, recs=exp: _same(got, recs, name, c, W, n, what)
    g.set_chunk(2)
    try:
        r = new()
        g.poly_mul(r, c10, c20, W, dimA, logq)
        for b, e in enumerate(exp):
            _is(to_host(r).reshape(BATCH, -1)[b], e["poly_mul"], "gpq_poly_mul, polynomial %d" % b)

        o0, o1 = new(), new()
        g.he_mul(o0, o1, c10, c11, c20, c21, rlk[0], rlk[1], W, logq, dimA, dimB, dimP)
        same(o0, "he_mul", 0, "gpq_he_mul c0"); same(o1, "he_mul", 1, "gpq_he_mul c1")
        assert g.last_lanes() in (1, 2)
        g.he_rs(o0, o1, W, logdelta, logq - logdelta)
        same(o0, "he_rs", 0, "gpq_he_rs after gpq_he_mul, c0"); same(o1, "he_rs", 1, "gpq_he_rs after gpq_he_mul, c1")
        o0, o1 = new(), new()
        g.he_mul_rs(o0, o1, c10, c11, c20, c21, rlk[0], rlk[1], W, logq, dimA, dimB, dimP, logdelta)
        same(o0, "he_rs", 0, "gpq_he_mul_rs c0"); same(o1, "he_rs", 1, "gpq_he_mul_rs c1")
        o0, o1 = new(), new()
        g.he_mul(o0, o1, c10, c11, c10, c11, rlk[0], rlk[1], W, logq, dimA, dimB, dimP)       # ct1 == ct2: the same slabs
        same(o0, "he_square", 0, "gpq_he_mul of a ciphertext with itself, c0"); same(o1, "he_square", 1, "gpq_he_mul of a ciphertext with itself, c1")
        t0, t1 = [_big([ref_jobs.tie_inputs(n, logq, logdelta, t["seed"])[c] for t in tasks], W) for c in (0, 1)]
        g.he_rs(t0, t1, W, logdelta, logq - logdelta)
        same(t0, "he_rs_ties", 0, "gpq_he_rs on the ties, c0"); same(t1, "he_rs_ties", 1, "gpq_he_rs on the ties, c1")

        m = _big([ins[0]["m"]] * BATCH, W)
        o0, o1 = new(), new()
        g.he_mulpt(o0, o1, c10, c11, m, W, logq, dimpt)
        same(o0, "he_mulpt", 0, "gpq_he_mulpt c0"); same(o1, "he_mulpt", 1, "gpq_he_mulpt c1")

        o0, o1 = new(), new()
        g.he_swk(o0, o1, c10, c11, rk[0][0], rk[0][1], W, logq, dimB, dimP)                   # he_rot by 0 is he_swk itself
        same(o0, "he_rot 0", 0, "gpq_he_swk c0"); same(o1, "he_rot 0", 1, "gpq_he_swk c1")
        ck = key(ins[0]["ck"])
        d0, d1, o0, o1 = new(), new(), new(), new()
        g.poly_conj(d0, c10, W); g.poly_conj(d1, c11, W)
        g.he_swk(o0, o1, d0, d1, ck[0], ck[1], W, logq, dimB, dimP)
        same(o0, "he_conj", 0, "he_conj c0"); same(o1, "he_conj", 1, "he_conj c1")
        far = {r: key(k) for r, k in ins[0]["rk_far"].items()}                                 # rot >= slots: he_rot does not bound rot
        rkey = lambda r: rk[r] if r < slots else far[r]
        for rots in ([1 % slots], [0, 1 % slots, 1 % slots, slots - 1], [slots, 1 % slots, slots + 3, slots]):   # nrot 1 and 4, repeats, rot >= slots
            o0, o1 = new(len(rots) * BATCH), new(len(rots) * BATCH)
            g.he_rot_hoisted(o0, o1, c10, c11, rots, [rkey(r)[0] for r in rots], [rkey(r)[1] for r in rots], W, logq, dimB, dimP)
            h0, h1 = to_host(o0).reshape(len(rots), -1), to_host(o1).reshape(len(rots), -1)   # rotation-major
            for i, r in enumerate(rots):
                same(h0[i], "he_rot %d" % r, 0, "gpq_he_rot_hoisted %s, rotation %d, c0" % (rots, r))
                same(h1[i], "he_rot %d" % r, 1, "gpq_he_rot_hoisted %s, rotation %d, c1" % (rots, r))

        diags = [ref_record.diag_ints(d, n) for d in exp[0]["diags"]]                            # the reference's own he_ecd of every diagonal
        assert len(diags) == slots and all(len(d) <= 2 * slots for d in exp[0]["diags"])
        if a.get("matrix") == "zero diagonals":
            assert sum(1 for d in diags if not any(d)) == slots - 2
        dg = _big(diags, W)
        o0, o1 = new(), new()
        g.he_gemv(o0, o1, c10, c11, dg, [x[0] for x in rk], [x[1] for x in rk], slots, W, logq, logdelta, dimB, dimP, dimpt)
        same(o0, "he_gemv", 0, "gpq_he_gemv c0"); same(o1, "he_gemv", 1, "gpq_he_gemv c1")
        with g.gemv_plan(dg, slots, W, logq, dimpt) as plan:
            assert plan.exact
            o0, o1 = new(), new()
            g.he_gemv_planned(o0, o1, c10, c11, plan, [x[0] for x in rk], [x[1] for x in rk], W, logdelta, dimB, dimP)
            same(o0, "he_gemv", 0, "gpq_he_gemv_planned c0"); same(o1, "he_gemv", 1, "gpq_he_gemv_planned c1")
    finally:
        g.set_chunk(32)
    torch.cuda.synchronize()


@pytest.mark.timeout(1200)
def test_default_shape_he_mul_and_rotation(engine_ctx, expected):
    """the reference's default shape (logn 14, q = 2^438, Delta = 2^50, 16 slots): one he_mul, one hoisted rotation"""
    a, e = ref_record.PARITY_DEFAULT, expected["default"]
    ctx = e["ctx"]
    ins = ref_jobs.functions_inputs(dict(a, dimub=ctx["dimub"]))
    n, W, logq = 1 << 14, 438 // 64 + 1, 438
    g = engine_ctx(14, ctx["dimub"])
    dimP, dimA, dimB, dimevk = g.he_dims(logq, logq)
    assert (dimP, dimevk) == (ctx["dim"], ctx["dimevk"]) == (8, 24)
    c10, c11, c20, c21 = [_big([ins[c][j]], W) for c, j in (("ct1", 0), ("ct1", 1), ("ct2", 0), ("ct2", 1))]
    key = lambda pair: (to_device(pair[0][:dimB * n]), to_device(pair[1][:dimB * n]))
    rlk = key(ins["rlk"])
    o0, o1 = torch.empty_like(c10), torch.empty_like(c10)
    g.he_mul(o0, o1, c10, c11, c20, c21, rlk[0], rlk[1], W, logq, dimA, dimB, dimP)
    _same(o0, [e], "he_mul", 0, W, n, "gpq_he_mul c0")
    _same(o1, [e], "he_mul", 1, W, n, "gpq_he_mul c1")
    rots = [1, 15, 16]                                                                         # 16 = slots: beyond the last slot
    keys = [key(ins["rk"][r] if r < 16 else ins["rk_far"][r]) for r in rots]
    o0, o1 = torch.empty(3 * W * n, dtype=torch.int64, device="cuda"), torch.empty(3 * W * n, dtype=torch.int64, device="cuda")
    g.he_rot_hoisted(o0, o1, c10, c11, rots, [x[0] for x in keys], [x[1] for x in keys], W, logq, dimB, dimP)
    h0, h1 = to_host(o0).reshape(3, -1), to_host(o1).reshape(3, -1)
    for i, r in enumerate(rots):
        _same(h0[i], [e], "he_rot %d" % r, 0, W, n, "gpq_he_rot_hoisted, rotation %d, c0" % r)
        _same(h1[i], [e], "he_rot %d" % r, 1, W, n, "gpq_he_rot_hoisted, rotation %d, c1" % r)


# ---------------------------------------------------------------------------
# drop-in surface: the MPI-typed symbols against the reference's own symbols of the same names
# ---------------------------------------------------------------------------
# Each host prints a digest of every result of either side.  The reference's side runs without a device (`refonly`), so its digests are kept in
# tests/golden/ref_hosts.json and pinned to the execution by tests/test_ref_golden.py.  Here: where oracle/_ref/ is at hand, the same MPIs go
# through both (dlopen, RTLD_LOCAL | RTLD_DEEPBIND), every coefficient, l and the bits of nu and B are compared, and both sides' digests must be
# the stored ones; where it is not, the library runs alone (`ref -`) and its digests must be the stored ones.  Nothing skips.
@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ref_parity_hosts"))
    return {"mpi_host": ref_record.build_host("mpi_host", d), "gemv_host": ref_record.build_host("gemv_host", d), "dir": d,
            "stored": ref_record.hosts_golden()}


@pytest.mark.parametrize("shape", ref_record.MPI_HOST_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_mpi_typed_symbols_equal_the_references_own(hosts, shape):
    """he_add / he_sub / he_addpt / he_subpt / he_neg / he_mulpt / he_mul (also in place on itself -- the destination aliases both operands,
    where the reference builds B from the nu it has just stored -- also one level down) / he_rs / he_rot / he_conj / he_moddown of
    libgpqhe_hip.so against the reference: every coefficient, l, the bits of nu and B; and hectx_init's L / dim / dimevk / Brs / Bmult[l]"""
    import subprocess
    stored = hosts["stored"]["mpi_host"]["%d_%d_%d" % shape]
    assert len(stored) == 18                                                                    # hectx and the 17 calls
    path = ref.which() if ref.available() else "-"
    res = subprocess.run([hosts["mpi_host"], "ref", path] + ref_record.mpi_host_args(shape), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert ref_record.digest_lines(res.stdout, "lib") == stored, "the library's results are not the reference's"
    if path != "-":
        assert "ref ok: 17 calls equal to the reference" in res.stdout, res.stdout
        assert ref_record.digest_lines(res.stdout, "ref") == stored, "tests/golden/ref_hosts.json is not what the executed reference computes"


@pytest.mark.parametrize("shape", ref_record.GEMV_HOST_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_mpi_typed_gemv_sum_idx_equal_the_references_own(hosts, shape):
    """he_gemv (also in place), he_sum, he_idx of libgpqhe_hip.so against the reference's, the diagonals encoded by the reference's own he_ecd
    on both sides (executed, or its recorded plaintexts looked up by the slot vector): every coefficient, l, the bits of nu and B"""
    import os
    import subprocess
    stored = hosts["stored"]["gemv_host"]["%d_%d_%d" % shape]
    args = [str(v) for v in shape]
    if ref.available():
        res = subprocess.run([hosts["gemv_host"], "ref", ref.which()] + args, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and res.stdout.count("ok he_") == 6 and "MISMATCH" not in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
        assert ref_record.digest_lines(res.stdout, "ref") == stored["ref"], "tests/golden/ref_hosts.json is not what the executed reference computes"
        assert ref_record.digest_lines(res.stdout, "lib") == stored["ref"]
    table = os.path.join(hosts["dir"], "ecd_%s.txt" % "_".join(args))
    with open(table, "w") as f:
        f.write("\n".join(stored["ecd"]) + "\n")
    res = subprocess.run([hosts["gemv_host"], "ref", "-", table] + args, capture_output=True, text=True, timeout=600)   # the library alone
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert ref_record.digest_lines(res.stdout, "lib") == stored["ref"], "the library's results are not the reference's"
