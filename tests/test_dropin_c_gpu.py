"""The reference-named link-time symbols, driven from a C host exactly as GPQHE's
own poly_mul limb loop drives them (tests/c/dropin_host.c), checked against the oracle."""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import fnv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dropin") / "dropin_host")
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "dropin_host.c"), "-L", lib_dir, "-lgpqhe_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


@pytest.mark.parametrize("logn,dim", [(7, 5), (13, 2), (16, 2)])
def test_c_host_limb_loop(host_binary, oracle_ctx, logn, dim):
    seed = 77
    res = subprocess.run([host_binary, str(logn), str(dim), str(seed)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    got = dict(line.split(None, 1) for line in res.stdout.strip().splitlines())
    o = oracle_ctx(logn, dim)
    n = o.n
    a, b = o.gen(seed, dim), o.gen(seed + 1, dim)
    ah, bh = o.ntt_slab(a, dim), o.ntt_slab(b, dim)
    mul = np.concatenate([o.rns_mul(ah[d * n:(d + 1) * n], bh[d * n:(d + 1) * n], d) for d in range(dim)])
    add = np.concatenate([o.rns_add(ah[d * n:(d + 1) * n], bh[d * n:(d + 1) * n], d) for d in range(dim)])
    r = o.ntt_slab(mul, dim, inverse=True)
    assert got["ntt_b"] == fnv(bh)
    assert got["mul"] == fnv(r) and got["alias"] == fnv(r)
    assert got["add"] == fnv(add)
    assert np.array_equal(r, o.poly_mul_rns(a, b, dim))
    p0 = o.p[0]
    prod = (p0 - 1) * (p0 - 2)
    assert got["barrett"].split()[0] == str(prod % p0)
    assert got["barrett"].split()[2] == str(prod * pow(1 << 64, -1, p0) % p0)


def _run_pointwise(host_binary, tmp_path, logn, nprimes, a, b, limbs):
    """a, b: uint64[rows][n]; row k runs with prime limbs[k] of the chain.  Returns (mul, add, aliased mul), each [rows][n]."""
    fa, fb, fo = (str(tmp_path / name) for name in ("a.bin", "b.bin", "out.bin"))
    np.ascontiguousarray(a, dtype=np.uint64).tofile(fa)
    np.ascontiguousarray(b, dtype=np.uint64).tofile(fb)
    res = subprocess.run([host_binary, "pointwise", str(logn), str(nprimes), fa, fb, fo] + [str(d) for d in limbs],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return np.fromfile(fo, dtype=np.uint64).reshape(3, len(limbs), -1)


def _edge_words(p):
    """The words src/poly.c:71-82 may meet at its door: p (what ntt stores for a residue 0, src/ntt.c:47), the limits of the
    device kernels' lazy ranges (modarith.hpp: mulmod_canon, addmod_canon) and the ends of the 64-bit word."""
    return np.array([p, p + 1, 2 * p - 1, 2 * p, 4 * p - 1, 4 * p, 8 * p - 1, 8 * p, 1 << 63, (1 << 64) - 1, 0], dtype=np.uint64)


def _pointwise_rows(p, n, rng):
    """[(name, a, b)] limbs for one prime: every edge word crossed with every other, random full 64-bit words, wide
    multiplicands, and limbs inside the domain (canonical, and p itself)."""
    e = _edge_words(p)
    crossed_a, crossed_b = np.repeat(e, e.size), np.tile(e, e.size)
    full = lambda: rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    canon = lambda: rng.integers(0, p, size=n, dtype=np.uint64)
    rows = []
    a, b = full(), canon()
    k = min(n, crossed_a.size)
    a[:k], b[:k] = crossed_a[:k], crossed_b[:k]
    rows.append(("edge words crossed", a, b))
    if n < crossed_a.size:                                              # logn 7: the rest of the cross
        a, b = full(), full()
        a[:crossed_a.size - n], b[:crossed_a.size - n] = crossed_a[n:], crossed_b[n:]
        rows.append(("edge words crossed (rest)", a, b))
    rows.append(("random 64-bit words", full(), full()))
    rows.append(("a in [p, 8p), b canonical", rng.integers(p, 8 * p, size=n, dtype=np.uint64), canon()))
    a, b = canon(), canon()
    a[:4], b[:4] = [0, 1, p - 1, p - 1], [p - 1, p - 1, 1, p - 1]
    rows.append(("canonical", a, b))
    a, b = canon(), canon()
    a[::3], b[1::3] = p, p
    a[5], b[5] = p, p
    rows.append(("canonical and p (the domain's edge)", a, b))
    a, b = canon(), canon()
    a[n // 2] = p + 1                                                   # one word outside the domain in an otherwise canonical limb
    rows.append(("one word p + 1", a, b))
    return rows


@pytest.mark.parametrize("logn", [7, 13, 16])
def test_pointwise_symbols_are_src_poly_c_for_any_words(host_binary, oracle_ctx, tmp_path, logn):
    """poly_rns_mul / poly_rns_add of include/gpqhe_hip_compat.h from a C host equal src/poly.c:71-82 -- barrett_reduce of the
    128-bit product / sum (the oracle restates it literally) -- for ANY 64-bit words, on every limb of a 5-limb chain and on the
    largest-c prime of the n = 2^17 chain (c > 2^28).  Canonical limbs and limbs holding other words alternate, so both paths of
    the library run in one process.  The large-c prime is the last of the n = 2^17 key-switch chain (44 + 15 limbs, BASELINE
    configs[4])."""
    rng = np.random.default_rng(900 + logn)
    cases = [(logn, 5, d) for d in range(5)] + ([(17, 59, 58)] if logn == 16 else [])
    for L, nprimes, d in cases:
        o = oracle_ctx(L, nprimes)
        p = o.p[d]
        if L == 17:
            assert p - (1 << 59) > 1 << 28, "the last prime of the n = 2^17 chain is no longer a large-c prime"
        rows = _pointwise_rows(p, 1 << L, rng)
        order = sorted(range(len(rows)), key=lambda i: (i % 2, i))     # canonical and wide limbs interleaved
        rows = [rows[i] for i in order]
        a = np.stack([r[1] for r in rows])
        b = np.stack([r[2] for r in rows])
        got = _run_pointwise(host_binary, tmp_path, L, nprimes, a, b, [d] * len(rows))
        for k, (name, ra, rb) in enumerate(rows):
            want = {"mul": o.rns_mul(ra, rb, d), "add": o.rns_add(ra, rb, d)}
            for which, g in (("mul", got[0, k]), ("add", got[1, k]), ("alias mul", got[2, k])):
                w = want["add" if which == "add" else "mul"]
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, "%s, n = 2^%d limb %d (p = %d), %s: %d words differ, first at %d: a = %d, b = %d, got %d, want %d" % (
                    which, L, d, p, name, bad.size, bad[0], ra[bad[0]], rb[bad[0]], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("logn", [7, 13])
def test_slab_pointwise_takes_p(engine_ctx, oracle_ctx, logn):
    """gpq_rns_mul / gpq_rns_add at the edge of their documented domain: the word p, which gpq_ntt stores for a residue 0
    (include/gpqhe_hip.h), as both operands and as either one, next to canonical words; every limb of a 5-limb chain."""
    from gpqhe_amd import to_device, to_host
    dim = 5
    g, o = engine_ctx(logn, dim), oracle_ctx(logn, dim)
    n = o.n
    rng = np.random.default_rng(40 + logn)
    a = np.concatenate([rng.integers(0, p, size=n, dtype=np.uint64) for p in o.p])
    b = np.concatenate([rng.integers(0, p, size=n, dtype=np.uint64) for p in o.p])
    for d, p in enumerate(o.p):
        lo = d * n
        a[lo:lo + n:4], b[lo:lo + n:4] = p, p                          # both p
        a[lo + 1:lo + n:4] = p                                          # a only
        b[lo + 2:lo + n:4] = p                                          # b only
        b[lo + 3], a[lo + 3] = 0, p
    da, db = to_device(a), to_device(b)
    r_mul, r_add = to_device(np.zeros_like(a)), to_device(np.zeros_like(a))
    g.poly_rns_mul(r_mul, da, db, dim)
    g.poly_rns_add(r_add, da, db, dim)
    got_mul, got_add = to_host(r_mul), to_host(r_add)
    for d in range(dim):
        sl = slice(d * n, (d + 1) * n)
        assert np.array_equal(got_mul[sl], o.rns_mul(a[sl], b[sl], d)), ("mul", logn, d)
        assert np.array_equal(got_add[sl], o.rns_add(a[sl], b[sl], d)), ("add", logn, d)
