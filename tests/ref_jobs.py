"""What the test_ref_* modules run inside reference worker processes (oracle/ref.py: one reference context per process).

Every job is a module-level function of one picklable argument; it opens its own `ref.Ref`, runs the EXECUTED reference and returns
plain data.  Jobs named check_* also run the restatement (oracle/oracle.py, oracle/bigint_ref.py) next to it, in the worker, and
return the list of differences -- the test asserts that the list is empty -- so that eight workers share the Python-integer work.
`functions_expected` is a plain function: the defect test calls it in the parent, under pytest's monkeypatch."""
import math
import os
import random

import numpy as np
import pytest

from oracle import bigint_ref as br
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_sources():
    """the checkout `make -C oracle ref` builds from (its default: next to the repository), or None"""
    path = os.environ.get("REF") or os.path.join(os.path.dirname(ROOT), "reference")
    return path if os.path.exists(os.path.join(path, "src", "gpqhe.h")) else None


def require_reference():
    """skip only on a bare checkout (neither sources nor oracle/_ref/); with sources and no build: fail"""
    if ref.available():
        return
    if reference_sources():
        pytest.fail("the reference checkout is there but oracle/_ref/ is not built: run __graft_entry__.build() (make -C oracle ref)")
    pytest.skip("bare checkout: neither a reference checkout nor oracle/_ref/")


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
def tables(arg):
    """polyctx_init(logn, 2^logq): everything the chain holds; zetas compared word for word with OracleCtx here (too big to ship)"""
    logn, logq = arg
    from oracle.oracle import OracleCtx
    R = ref.Ref().init(logn, 1 << logq)
    o = OracleCtx(logn, R.dimub)
    out = {"dimub": R.dimub, "logqub": R.L.ref_logqub(), "nodes": [R.node(d) for d in range(R.dimub)], "prefix": [R.prefix(d) for d in range(R.dimub)],
           "zeta_diffs": [], "psi_R": []}
    for d in range(R.dimub):
        z, zi = R.zetas(d), R.zetas(d, inverse=True)
        out["zeta_diffs"].append((int((z != o.zetas(d)).sum()), int((zi != o.zetas(d, inverse=True)).sum())))
        out["psi_R"].append((int(z[R.n // 2]), int(zi[R.n // 2])))          # i = 1 of src/precomp.c:255-263: root R mod p, root^-1 R mod p
    return out


def hectx(arg):
    logn, logq, logdelta, slots = arg
    R = ref.Ref().init(logn, 1 << logq, slots, 1 << logdelta)
    P, PqL = R.he_P()
    return {"dim": R.dim, "dimevk": R.dimevk, "L": R.Lmax, "q": [R.he_q(l) for l in range(R.Lmax + 1)], "P": P, "PqL": PqL, "dimub": R.dimub,
            "primes": [R.node(d)["p"] for d in range(R.dimub)]}


def over_the_cap(arg):
    """ref_init's return value for a modulus the reference would abort() on"""
    try:
        ref.Ref().init(arg[0], 1 << arg[1])
    except ref.RefError as e:
        return e.code
    return 0


# ---------------------------------------------------------------------------
# limbs
# ---------------------------------------------------------------------------
def limb_inputs(o, d, seed):
    """[(name, limb, ops)]: what goes into ntt / invntt / poly_rns_mul / poly_rns_add of prime d"""
    from tests.zero_cases import limb_cases
    n, p = o.n, o.p[d]
    rng = np.random.default_rng(seed)
    cases = [("uniform %d" % k, rng.integers(0, p, size=n, dtype=np.uint64)) for k in range(3)]
    cases += [("zero case: " + name, a) for name, a in limb_cases(o, d, rng)]
    cases += [("p throughout", np.full(n, p, dtype=np.uint64)), ("p - 1 throughout", np.full(n, p - 1, dtype=np.uint64)),
              ("0 and p alternating", np.where(np.arange(n) % 2 == 0, 0, p).astype(np.uint64))]
    # the domain gpq_ntt_reference claims: any 64-bit word, wrap-around included
    full = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    cases += [("any 64-bit word", full), ("2^64 - 1 throughout", np.full(n, (1 << 64) - 1, dtype=np.uint64)),
              ("multiples of p up to 2^64", (rng.integers(0, (1 << 64) // p + 1, size=n, dtype=np.uint64) * np.uint64(p))),
              ("p + small", np.uint64(p) + rng.integers(0, 4, size=n, dtype=np.uint64))]
    return cases


def check_limbs(arg):
    """ntt, invntt, poly_rns_mul, poly_rns_add of the reference against the oracle on first, middle and last prime: [difference]"""
    logn, logq, seed = arg
    from oracle.oracle import OracleCtx
    R = ref.Ref().init(logn, 1 << logq)
    o = OracleCtx(logn, R.dimub)
    diffs, seen_p, compared = [], 0, 0
    if [R.node(d)["p"] for d in range(R.dimub)] != o.p:
        return {"diffs": ["prime chain"], "seen_p": 0, "compared": 0}
    for d in sorted({0, R.dimub // 2, R.dimub - 1}):
        cases = limb_inputs(o, d, seed + d)
        for k, (name, a) in enumerate(cases):
            b = cases[(k + 1) % len(cases)][1]
            got = R.ntt(a, d)
            seen_p += int((got == np.uint64(o.p[d])).sum()) if name.startswith("zero case") else 0
            for op, g, e in (("ntt", got, o.ntt(a, d)), ("invntt", R.invntt(a, d), o.invntt(a, d)),
                             ("invntt(ntt)", R.invntt(got, d), o.invntt(got, d)),
                             ("poly_rns_mul", R.rns_mul(a, b, d), o.rns_mul(a, b, d)), ("poly_rns_add", R.rns_add(a, b, d), o.rns_add(a, b, d))):
                compared += 1
                if not np.array_equal(g, e):
                    diffs.append("logn %d prime %d %s on '%s': %d words differ" % (logn, d, op, name, int((g != e).sum())))
    return {"diffs": diffs, "seen_p": seen_p, "compared": compared}


def reduce_values(arg):
    """montgomery_reduce / barrett_reduce of the reference on (lo, hi) words for prime d: raw outputs"""
    logn, logq, d, lo, hi = arg
    R = ref.Ref().init(logn, 1 << logq)
    node = R.node(d)
    return {"node": node, "mont": R.reduce(d, lo, hi, False), "barr": R.reduce(d, lo, hi, True),
            "mont_inv": int(R.L.ref_montgomery_inv(node["p"])), "barr_inv": int(R.L.ref_barrett_inv(node["p"]))}


def survey_digests(arg):
    """the quantities of tests/golden/survey_8c.json for one logn, from the executed reference (inputs by the oracle's seeded generator)"""
    logn, logq, count, kat = arg
    from oracle.oracle import OracleCtx, fnv
    R = ref.Ref().init(logn, 1 << logq)
    o = OracleCtx(logn, count)                           # only its splitmix64 generator and FNV digest are used here
    primes = [R.node(d)["p"] for d in range(R.dimub)]
    out = {"count": R.dimub, "first": [str(p) for p in primes[:5]], "xor_all": 0, "node0": R.node(0)}
    for p in primes:
        out["xor_all"] ^= p
    z, zi = R.zetas(0), R.zetas(0, inverse=True)
    out["zetas"] = (str(z[R.n // 2]), str(z[1]), str(zi[1]))
    out["phat_invmp"] = [[str(v) for v in R.prefix(d)[0]] for d in range(min(5, R.dimub))]
    a = o.gen(1, 1)
    t = R.ntt(a, 0)
    out["ntt"] = {"input": fnv(a), "ntt": fnv(t), "out012": [str(v) for v in t[:3]], "back": bool(np.array_equal(R.invntt(t, 0), a))}
    if kat:
        n, (dA, dB, seeds) = R.n, kat
        ins = [o.gen(seeds[k], dA) for k in ("a0", "a1", "b0", "b1")]
        d0, d1, d2 = [], [], []
        for d in range(dA):                               # src/he-mult.c:116-138, limb by limb
            h = [R.ntt(x[d * n:(d + 1) * n], d) for x in ins]
            d0.append(R.invntt(R.rns_mul(h[0], h[2], d), d))
            d2.append(R.invntt(R.rns_mul(h[1], h[3], d), d))
            d1.append(R.rns_add(R.invntt(R.rns_mul(h[0], h[3], d), d), R.invntt(R.rns_mul(h[1], h[2], d), d), d))
        x, e0, e1 = o.gen(seeds["d2"], dB), o.gen(seeds["evk0"], dB), o.gen(seeds["evk1"], dB)
        c0, c1 = [], []
        for d in range(dB):                               # src/he-mult.c:58-66
            xh = R.ntt(x[d * n:(d + 1) * n], d)
            c0.append(R.invntt(R.rns_mul(xh, e0[d * n:(d + 1) * n], d), d))
            c1.append(R.invntt(R.rns_mul(xh, e1[d * n:(d + 1) * n], d), d))
        out["kat"] = {"inputs": [fnv(v) for v in ins], "d0": fnv(np.concatenate(d0)), "d1": fnv(np.concatenate(d1)), "d2": fnv(np.concatenate(d2)),
                      "c0": fnv(np.concatenate(c0)), "c1": fnv(np.concatenate(c1))}
    return out


# ---------------------------------------------------------------------------
# the division defect
# ---------------------------------------------------------------------------
def defect_rdiv_noalias(a, m):
    """mpi_rdiv(q, a, m) with q a separate MPI, on a libgcrypt whose floor division loses the quotient's sign (1.9.4): floor quotient, sign
    dropped when a < 0, the remainder is non-zero AND |a| >= m, then the `r > m/2` increment of src/types.c:123-124.  For |a| < m the
    truncated quotient is 0, the library's decrement gives -1 correctly and nothing is lost."""
    q, r = divmod(a, m)
    if a < 0 and r != 0 and -a >= m:
        q = -q
    return q + 1 if r > m // 2 else q


def defect_rdiv(a, m):
    """mpi_rdiv(a, a, m): the quotient aliases the dividend, as in EVERY call of the reference (src/he-mult.c:71-72, src/he-automorphism.c:
    71-72, src/he-rescale.c:46-47).  libgcrypt's floor division decides on its adjustment from the dividend's sign AFTER the truncating
    division has written the quotient over it.  Where |a| has fewer 64-bit limbs than m the truncating division returns early with a
    quotient +0, so nothing is adjusted: q = 0 and the remainder stays negative, never above m/2 -- the result is 0, where the
    mathematical rule gives -1 for -m < a <= -m/2.  Elsewhere as defect_rdiv_noalias.  (Measured on libgcrypt 1.9.4.)"""
    limbs = lambda v: (abs(v).bit_length() + 63) // 64
    if a < 0 and limbs(a) < limbs(m):
        return 0
    return defect_rdiv_noalias(a, m)


def division(arg):
    """[(dividends, modulus)] -> per modulus: the as-is build's mpi_rdiv (aliased and not), gcry_mpi_div(.., -1), oracle_fdiv in both call shapes"""
    out = []
    R = ref.Ref(ref.AS_IS).init(4, 1 << 30)
    for values, m in arg:
        out.append({"rdiv": R.mpi_rdiv(values, m), "rdiv_noalias": R.mpi_rdiv(values, m, alias=False), "gcry": R.fdiv(values, m, 0),
                    "ofdiv": R.fdiv(values, m, 1), "ofdiv_alias": R.fdiv(values, m, 2)})
    return out


def floor_build_rdiv(arg):
    values, m = arg
    return ref.Ref(ref.FLOOR).init(4, 1 << 30).mpi_rdiv(values, m)


# ---------------------------------------------------------------------------
# whole functions
# ---------------------------------------------------------------------------
def _centred(rng, n, q, kind):
    h = q // 2
    if kind == "max":
        return [h - 1] * n
    if kind == "min":
        return [-h] * n
    v = [rng.randrange(-h, h) for _ in range(n)]
    v[:6] = [0, -1, h - 1, -h, 1, -(h - 1)]
    return v


def zrotdiag(A, slots, idx, rot):
    """src/he-algo.c:29-43 on a row-major slots x slots list"""
    diag = [A[(i % slots) * slots + (idx + i) % slots] for i in range(slots)]
    return [diag[(i + rot) % slots] for i in range(slots)]


def tie_inputs(n, logq, logdelta, seed):
    """coefficients whose remainder by Delta sits ON and next to mpi_rdiv's tie (r == Delta/2 rounds down, src/types.c:123), both signs"""
    rng, D, q = random.Random(seed), 1 << logdelta, 1 << logq
    out = []
    for c in range(2):
        v = []
        for i in range(n):
            k = rng.randrange(-(q // (2 * D)) + 1, q // (2 * D) - 1)
            v.append(k * D + D // 2 + (i % 3 - 1))            # remainder Delta/2 - 1, Delta/2, Delta/2 + 1
        v[:4] = [D // 2, -(D // 2), D // 2 + 1, -(D // 2) - 1]
        out.append(v)
    return tuple(out)


def functions_inputs(a):
    """seeded inputs of one shape: a = dict(logn, logq, logdelta, slots, seed, kind)"""
    from oracle.oracle import OracleCtx
    logn, logq, slots = a["logn"], a["logq"], a["slots"]
    n, q = 1 << logn, 1 << logq
    rng = random.Random(a.get("ctseed", a["seed"]))      # the ciphertexts; keys, plaintext and matrix depend on `seed` alone (a batch shares them)
    dimub = a["dimub"]
    o = OracleCtx(logn, dimub)
    dimevk = br.he_dims(logn, o.p, logq, logq)[3]
    kind = a.get("kind", "random")
    ct1 = (_centred(rng, n, q, kind), _centred(rng, n, q, kind))
    ct2 = (_centred(rng, n, q, "min" if kind == "max" else kind), _centred(rng, n, q, kind))
    rng = random.Random(a["seed"] + 12345)
    A = [complex(rng.uniform(-1, 1), rng.uniform(-1, 1)) for _ in range(slots * slots)]
    if a.get("matrix") == "zero diagonals":               # only diagonals 0 and slots - 1 hold anything
        A = [v if (c - r) % slots in (0, slots - 1) else 0j for r in range(slots) for c, v in zip(range(slots), A[r * slots:(r + 1) * slots])]
    ins = {"o": o, "ct1": ct1, "ct2": ct2,
           "m": [rng.randrange(-(1 << a["logdelta"]), 1 << a["logdelta"]) for _ in range(n)],
           "rlk": (o.gen(a["seed"] * 100 + 1, dimevk), o.gen(a["seed"] * 100 + 2, dimevk)),
           "ck": (o.gen(a["seed"] * 100 + 3, dimevk), o.gen(a["seed"] * 100 + 4, dimevk)),
           "rk": [(o.gen(a["seed"] * 100 + 10 + 2 * r, dimevk), o.gen(a["seed"] * 100 + 11 + 2 * r, dimevk)) for r in range(slots)],
           # he_rot does not bound rot (it indexes rk[rot], src/he-automorphism.c:111): keys for two rotations at and beyond `slots`
           "rk_far": {r: (o.gen(a["seed"] * 100 + 5000 + 2 * r, dimevk), o.gen(a["seed"] * 100 + 5001 + 2 * r, dimevk)) for r in (slots, slots + 3)},
           "A": A}
    return ins


NU1, B1, NU2, B2 = 3.0 * 2 ** 20, 1234.5, 5.0 * 2 ** 19, 77.25


def functions_run(a):
    """the executed reference on one shape: {name: ((c0, c1), l, bits(nu), bits(B))}; `build` picks the library (default ref.which())"""
    logn, logq, logdelta, slots = a["logn"], a["logq"], a["logdelta"], a["slots"]
    R = ref.Ref(a.get("build")).init(logn, 1 << logq, slots, 1 << logdelta)
    a = dict(a, dimub=R.dimub)
    ins = functions_inputs(a)
    L = R.Lmax
    Brs, Bmult = R.he_bounds()
    out = {"_ctx": {"dim": R.dim, "dimevk": R.dimevk, "L": L, "dimub": R.dimub, "q": [R.he_q(l) for l in range(L + 1)], "Brs": Brs, "Bmult": Bmult}}
    R.evk_set("rlk", *ins["rlk"])
    R.evk_set("ck", *ins["ck"])
    for r in range(slots):
        R.evk_set(r, *ins["rk"][r])
    for r, k in ins["rk_far"].items():
        R.evk_set(r, *k)
    only = a.get("only")

    def load():
        R.ct_set(0, ins["ct1"], L, NU1, B1)
        R.ct_set(1, ins["ct2"], L, NU2, B2)
        R.pt_set(0, ins["m"], float(1 << logdelta))

    def want(name):
        return only is None or name in only

    load()
    if want("he_add"):
        R.he_add(2, 0, 1); out["he_add"] = R.ct_get(2)
        R.he_sub(2, 0, 1); out["he_sub"] = R.ct_get(2)
        R.he_addpt(2, 0, 0); out["he_addpt"] = R.ct_get(2)
        R.he_subpt(2, 0, 0); out["he_subpt"] = R.ct_get(2)
        R.he_neg(0); out["he_neg"] = R.ct_get(0)
        load()
    if want("he_mulpt"):
        R.he_mulpt(2, 0, 0); out["he_mulpt"] = R.ct_get(2)
    if want("he_mul"):
        R.he_mul(2, 0, 1); out["he_mul"] = R.ct_get(2)
        if L >= 1:
            R.he_rs(2); out["he_rs"] = R.ct_get(2)
        R.he_mul(3, 0, 0); out["he_square"] = R.ct_get(3)              # ct1 == ct2: the same object
        R.ct_set(5, ins["ct1"], L, NU1, B1)
        R.he_mul(5, 5, 5); out["he_square_in_place"] = R.ct_get(5)     # ct == ct1 == ct2, src/he-algo.c:151
        if L >= 1:
            R.ct_set(4, tie_inputs(R.n, logq, logdelta, a["seed"]), L, NU1, B1)
            R.he_rs(4); out["he_rs_ties"] = R.ct_get(4)
    if want("poly_mul"):
        dimA = (2 * (logq + 1) + logn) // 59 + 1
        out["_poly_mul"] = R.poly_mul(ins["ct1"][0], ins["ct2"][0], dimA, 1 << logq)
    if want("he_moddown") and L >= 1:
        R.he_moddown(0); R.he_moddown(1); out["he_moddown"] = R.ct_get(0)
        R.he_mul(2, 0, 1); out["he_mul_low"] = R.ct_get(2)             # one level down: q_{L-1}, other dims
        load()
    if want("he_rot"):
        for r in sorted({0, 1 % slots, slots - 1, slots, slots + 3}):
            load()
            R.he_rot(0, r); out["he_rot %d" % r] = R.ct_get(0)
        load()
        R.he_conj(0); out["he_conj"] = R.ct_get(0)
        load()
    if want("he_gemv") and L >= 1:
        n1, n2 = br.gemv_steps(slots)
        diags = []
        for i in range(n2):
            for j in range(n1):
                R.he_ecd(1, zrotdiag(ins["A"], slots, i * n1 + j, -(i * n1)))
                diags.append(R.pt_get(1)[0])
        out["_diags"] = diags
        R.he_gemv(2, ins["A"], 0); out["he_gemv"] = R.ct_get(2)
        ones = [1.0 + 0j] * slots
        R.he_ecd(1, ones); out["_ecd_ones"] = R.pt_get(1)[0]
        R.he_ecd(1, [0j] * slots); out["_ecd_zero"] = R.pt_get(1)[0]
        unit = [[(1.0 + 0j) if i == k else 0j for i in range(slots)] for k in range(slots)]
        out["_ecd_unit"] = []
        for k in range(slots):
            R.he_ecd(1, unit[k]); out["_ecd_unit"].append(R.pt_get(1)[0])
        R.he_sum(2, 0); out["he_sum"] = R.ct_get(2)
        R.he_idx(2, 0, slots - 1); out["he_idx"] = R.ct_get(2)
    return out


def _f(x):
    return ref.bits(float(x))


def functions_expected(a, ctx, diag_data):
    """the restatement's answer to functions_run, same keys (without the '_' entries)"""
    logn, logq, logdelta, slots = a["logn"], a["logq"], a["logdelta"], a["slots"]
    a = dict(a, dimub=ctx["dimub"])
    ins = functions_inputs(a)
    o, n = ins["o"], 1 << logn
    L = logq // logdelta
    Delta = float(1 << logdelta)
    Brs = math.sqrt(n / 3.) * (3 + 8 * math.sqrt(64))                   # src/precomp.c:416
    Bmult = ctx["Bmult"]                                                # the reference's own table (long double products, src/precomp.c:419-428)
    mulB = lambda nu1, b1, nu2, b2, l: nu1 * b2 + nu2 * b1 + b1 * b2 + Bmult[l]          # src/he-mult.c:94-95
    logql = lambda l: logq - (L - l) * logdelta
    ql = 1 << logq
    only = a.get("only")
    want = lambda name: only is None or name in only
    exp = {"_ctx": {"L": L, "q": [1 << logql(l) for l in range(L + 1)], "Brs": Brs}}
    dimP, dimA, dimB, dimevk = br.he_dims(logn, o.p, logq, logq)
    exp["_ctx"].update(dim=dimP, dimevk=dimevk)
    ct1, ct2, m = ins["ct1"], ins["ct2"], ins["m"]
    key = lambda k: (k[0][:dimB * n], k[1][:dimB * n])
    if want("he_add"):
        exp["he_add"] = (tuple(br.he_add(ct1, ct2, ql)), L, _f(max(NU1, NU2)), _f(B1 + B2))
        exp["he_sub"] = (tuple(br.he_sub(ct1, ct2, ql)), L, _f(max(NU1, NU2)), _f(B1 + B2))
        exp["he_addpt"] = (tuple(br.he_addpt(ct1, m, ql)), L, _f(max(NU1, Delta)), _f(B1))
        exp["he_subpt"] = (tuple(br.he_subpt(ct1, m, ql)), L, _f(max(NU1, Delta)), _f(B1))
        exp["he_neg"] = (tuple(br.he_neg(ct1, ql)), L, _f(NU1), _f(B1))
    dimpt = (logq + 1 + logdelta + logn) // 59 + 1                       # src/he-mult.c:168 with nu = Delta
    if want("he_mulpt"):
        exp["he_mulpt"] = (tuple(br.he_mulpt(o, ct1, m, dimpt, logq)), L, _f(NU1 * Delta), _f(B1 * Delta))
    if want("he_mul"):
        e = br.he_mul(o, ct1, ct2, *key(ins["rlk"]), dimP, dimA, dimB, logq)
        exp["he_mul"] = (tuple(e), L, _f(NU1 * NU2), _f(mulB(NU1, B1, NU2, B2, L)))
        if L >= 1:
            qd = 1 << logql(L - 1)
            exp["he_rs"] = (tuple([br.mpi_smod(br.mpi_rdiv(v, 1 << logdelta), qd) for v in c] for c in e), L - 1, _f(NU1 * NU2 / Delta),
                            _f(mulB(NU1, B1, NU2, B2, L) / Delta + Brs))
        sq = tuple(br.he_mul(o, ct1, ct1, *key(ins["rlk"]), dimP, dimA, dimB, logq))
        exp["he_square"] = (sq, L, _f(NU1 * NU1), _f(mulB(NU1, B1, NU1, B1, L)))
        # destination == both operands: :93 stores nu before :94-95 read ct1->nu / ct2->nu, so B is built from the NEW nu
        exp["he_square_in_place"] = (sq, L, _f(NU1 * NU1), _f(mulB(NU1 * NU1, B1, NU1 * NU1, B1, L)))
        if L >= 1:
            ties = tie_inputs(n, logq, logdelta, a["seed"])
            exp["he_rs_ties"] = (tuple([br.mpi_smod(br.mpi_rdiv(v, 1 << logdelta), qd) for v in c] for c in ties), L - 1, _f(NU1 / Delta), _f(B1 / Delta + Brs))
    if want("he_moddown") and L >= 1:
        lq = logql(L - 1)
        qd = 1 << lq
        low1, low2 = [tuple([br.mpi_smod(v, qd) for v in c] for c in ct) for ct in (ct1, ct2)]
        exp["he_moddown"] = (low1, L - 1, _f(NU1), _f(B1))
        _, dA, dB, _ = br.he_dims(logn, o.p, logq, lq)
        exp["he_mul_low"] = (tuple(br.he_mul(o, low1, low2, ins["rlk"][0][:dB * n], ins["rlk"][1][:dB * n], dimP, dA, dB, lq)), L - 1, _f(NU1 * NU2),
                             _f(mulB(NU1, B1, NU2, B2, L - 1)))
    if want("he_rot"):
        for r in sorted({0, 1 % slots, slots - 1, slots, slots + 3}):
            e = br.he_swk(o, br.poly_rot(ct1[0], r), br.poly_rot(ct1[1], r), *key(ins["rk"][r] if r < slots else ins["rk_far"][r]), dimP, dimB, logq)
            exp["he_rot %d" % r] = (tuple(e), L, _f(NU1), _f(B1))
        e = br.he_swk(o, br.poly_conj(ct1[0]), br.poly_conj(ct1[1]), *key(ins["ck"]), dimP, dimB, logq)
        exp["he_conj"] = (tuple(e), L, _f(NU1), _f(B1))
    if want("he_gemv") and L >= 1:
        keys = [key(k) for k in ins["rk"]]
        n1, n2 = br.gemv_steps(slots)
        nu_out = _f(NU1 * Delta / Delta)
        inner = B1 * Delta                                              # he_mulpt, src/he-mult.c:164; he_add sums B, src/he-add.c:38; he_rot keeps it
        for _ in range(n1 - 1):
            inner = inner + B1 * Delta
        outer = inner
        for _ in range(n2 - 1):
            outer = outer + inner
        B_out = _f(outer / Delta + Brs)
        exp["he_gemv"] = (tuple(br.ref_gemv(o, ct1, diag_data["_diags"], keys, slots, dimP, dimB, dimpt, logq, logdelta)), L - 1, nu_out, B_out)
        # he_sum: A[0][i] = 1 (src/he-algo.c:98-101): diagonal k holds a one at slot i with (i + k) % slots == i ... row 0 only -> i = 0 before rotation
        sum_diags, idx_diags = [], []
        for i in range(n2):
            for j in range(n1):
                k, rot = i * n1 + j, -(i * n1)
                for A, dst in (([1.0 if t < slots else 0.0 for t in range(slots * slots)], sum_diags),
                               ([1.0 if t == (slots - 1) * slots + slots - 1 else 0.0 for t in range(slots * slots)], idx_diags)):
                    v = zrotdiag(A, slots, k, rot)
                    if not any(v):
                        dst.append(diag_data["_ecd_zero"])
                    else:
                        assert sum(v) == 1.0
                        dst.append(diag_data["_ecd_unit"][v.index(1.0)])
        exp["he_sum"] = (tuple(br.ref_gemv(o, ct1, sum_diags, keys, slots, dimP, dimB, dimpt, logq, logdelta)), L - 1, nu_out, B_out)
        exp["he_idx"] = (tuple(br.ref_gemv(o, ct1, idx_diags, keys, slots, dimP, dimB, dimpt, logq, logdelta)), L - 1, nu_out, B_out)
    return exp


def compare_functions(got, exp):
    """[difference] between functions_run and functions_expected"""
    diffs = []
    for k in ("dim", "dimevk", "L", "q", "Brs"):
        if got["_ctx"][k] != exp["_ctx"][k]:
            diffs.append("hectx.%s: reference %r, restatement %r" % (k, got["_ctx"][k], exp["_ctx"][k]))
    names = [k for k in got if not k.startswith("_")]
    if sorted(names) != sorted(k for k in exp if not k.startswith("_")):
        diffs.append("different sets of results: %s vs %s" % (sorted(names), sorted(exp)))
    for name in names:
        (g, gl, gnu, gB), (e, el, enu, eB) = got[name], exp.get(name, ((None, None), None, None, None))
        for c in (0, 1):
            if e[c] is None or list(g[c]) != list(e[c]):
                bad = [i for i, (x, y) in enumerate(zip(g[c], e[c] or [])) if x != y]
                diffs.append("%s c%d: %d coefficients differ, first at %s" % (name, c, len(bad), bad[:3]))
        if gl != el:
            diffs.append("%s: l %r vs %r" % (name, gl, el))
        if gnu != enu:
            diffs.append("%s: nu bits %016x vs %016x" % (name, gnu, enu or 0))
        if eB is not None and gB != eB:
            diffs.append("%s: B bits %016x vs %016x" % (name, gB, eB))
    return diffs


def check_functions(a):
    got = functions_run(a)
    return {"diffs": compare_functions(got, functions_expected(a, got["_ctx"], got)), "names": sorted(k for k in got if not k.startswith("_")),
            "ctx": got["_ctx"]}


def ntt_inputs(logn, dim, seed):
    """(names, zero-case slab, non-canonical slab): limb d of every polynomial on prime d; needs the oracle only (it builds inputs, nothing expected)"""
    from oracle.oracle import OracleCtx
    from tests.zero_cases import slab_of_cases
    o = OracleCtx(logn, dim)
    n = o.n
    names, cases = slab_of_cases(o, dim, seed)
    rng = np.random.default_rng(seed)
    wild = rng.integers(0, 1 << 64, size=3 * dim * n, dtype=np.uint64)
    wild[:8] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for d in range(dim):
        wild[(dim + d) * n:(dim + d + 1) * n:2] = np.uint64(o.p[d])
    return names, cases, wild


def ntt_slabs(arg):
    """(zero-case slab, its ntt, non-canonical slab, its ntt, its invntt) by the executed reference"""
    logn, logq, dim, seed = arg
    R = ref.Ref().init(logn, 1 << logq)
    n = R.n
    names, cases, wild = ntt_inputs(logn, dim, seed)
    xf = lambda slab, inv: np.concatenate([R.ntt(slab[i * n:(i + 1) * n], i % dim, inverse=inv) for i in range(slab.size // n)])
    fwd = xf(cases, False)
    return {"names": names, "primes": [R.node(d)["p"] for d in range(dim)], "cases": cases, "cases_ntt": fwd, "wild": wild,
            "wild_ntt": xf(wild, False), "wild_invntt": xf(wild, True), "cases_ntt_invntt": xf(fwd, True)}


# ---------------------------------------------------------------------------
# polynomial level
# ---------------------------------------------------------------------------
def check_poly(arg):
    """poly_mul (q = 2^logq and q = P q_L), poly_rns2mpi, rns_decompose / rns_reconstruct, poly_rot, poly_conj, mpi_smod: [difference]"""
    logn, logq, slots, seed = arg
    from oracle.oracle import OracleCtx
    R = ref.Ref().init(logn, 1 << logq)
    o = OracleCtx(logn, R.dimub)
    n, q, rng, diffs = 1 << logn, 1 << logq, random.Random(seed), []
    a, b = _centred(rng, n, q, "random"), _centred(rng, n, q, "random")
    dimP = (logq + 1 + logn) // 59 + 1
    P = br.RnsBasis(o.p[:dimP]).P
    for name, modulus, dim in (("q = 2^logq", q, (2 * (logq + 1) + logn) // 59 + 1), ("q = P q_L", P * q, R.dimub)):
        dim = min(dim, R.dimub)
        basis = br.RnsBasis(o.p[:dim])
        if 2 * n * (q // 2) ** 2 >= basis.P:
            continue                                      # the product must fit the basis for the integer expectation below
        got = R.poly_mul(a, b, dim, modulus)
        prod = o.poly_mul_rns(br._slab(o, a, dim), br._slab(o, b, dim), dim)
        if got != br.poly_rns2mpi(br._limbs(prod, dim, n), basis, modulus):
            diffs.append("poly_mul, %s: differs from the restatement" % name)
        if n <= 512 and got != [br.centred_mod(v, modulus) for v in br.negacyclic_mul(a, b)]:
            diffs.append("poly_mul, %s: differs from the integer negacyclic product" % name)
    for dim in sorted({1, 2, R.dimub // 2 + 1, R.dimub}):
        basis = br.RnsBasis(o.p[:dim])
        rhat = np.concatenate([np.array([rng.randrange(0, o.p[d]) for _ in range(n)], dtype=np.uint64) for d in range(dim)])
        rhat[:2] = [0, o.p[0] - 1]
        limbs = br._limbs(rhat, dim, n)
        if R.rns_reconstruct(rhat, dim) != [br.rns_reconstruct(limbs, i, basis) for i in range(n)]:
            diffs.append("rns_reconstruct at dim %d" % dim)
        for modulus in (q, 1 << (logq // 2), basis.P * 3 + 1, 1000003):
            if R.poly_rns2mpi(rhat, dim, modulus) != br.poly_rns2mpi(limbs, basis, modulus):
                diffs.append("poly_rns2mpi at dim %d, modulus of %d bits" % (dim, modulus.bit_length()))
    for d in sorted({0, R.dimub - 1}):
        if R.rns_decompose(a, d).tolist() != br.rns_decompose(a, o.p[d]):
            diffs.append("rns_decompose, prime %d" % d)
    for rot in sorted({0, 1, max(slots - 1, 0), slots, slots + 3, 27}):   # 5^27 < 2^64 < 5^28: the power is taken in size_t
        if R.poly_rot(a, rot) != br.poly_rot(a, rot):
            diffs.append("poly_rot by %d" % rot)
    if R.poly_conj(a) != br.poly_conj(a):
        diffs.append("poly_conj")
    vals = a[:64] + [v * 3 for v in b[:64]] + [q, -q, q // 2, -(q // 2) - 1]
    for modulus in (q, 1000003, P):
        if R.mpi_smod(vals, modulus) != [br.mpi_smod(v, modulus) for v in vals]:
            diffs.append("mpi_smod, modulus of %d bits" % modulus.bit_length())
    return diffs

