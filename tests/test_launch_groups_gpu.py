"""Batches that the slab API cuts into several launch groups (engine.hip: kMaxPolysPerLaunch = 16384 polynomials per launch;
gpq_poly_mul_rns half of that, gpq_mulpt_rns a quarter), against the oracle.  Every group after the first has its own slab offset,
its own zero-flag words and, on two-pass rings, its own cache policy (nt_for: a full group's working set exceeds 288 MiB, a short
tail's does not).  One call at batch 2G + 1 (two full groups and a one-polynomial tail) must give

  * the oracle's words (src/ntt.c, src/poly.c:71-103, src/he-mult.c:179-185) at the polynomials around every group boundary and at
    seeded random places, and
  * every word of the same data run as calls of at most G polynomials on views at other offsets (those stay in the first pass of the
    loop, which the rest of the suite anchors to the oracle)."""
import gc

import numpy as np
import pytest

from gpqhe_amd import to_host
from tests.zero_cases import slab_of_cases

pytestmark = pytest.mark.gpu

G_FULL = 16384              # engine.hip kMaxPolysPerLaunch
NT_BYTES = 288 << 20        # engine.hip nt_for: non-temporal slab accesses above this working set


def nt_for(logn, polys, limbs, slabs):
    """engine.hip nt_for with the default policy (gpq_set_nt_policy -1)."""
    return int(polys * limbs * (8 << logn) * slabs > NT_BYTES)


def _ctx(logn):
    import gpqhe_amd
    return gpqhe_amd.PolyContext(logn, 1)      # a context of its own: default cache policy, default limb classes


def _free():
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _anchors(G, batch, seed):
    rng = np.random.default_rng(seed)
    fixed = [0, G - 1, G, G + 1, 2 * G - 1, 2 * G]
    return sorted(set(fixed) | set(int(k) for k in rng.integers(0, batch, size=12)))


def _rows(t, n, idx):
    """polynomials idx of a one-limb slab tensor, on the host"""
    import torch
    return to_host(t.view(-1, n).index_select(0, torch.tensor(idx, device=t.device)))


def _cuts(G, batch):
    first = 5000 if G > 5000 else 1000
    return [0, first, first + G, batch]        # pieces of first, G and G + 1 - first polynomials: each <= G


# name: (group size, number of slabs, input slabs, slabs holding the outputs, the call, cache-policy slabs of nt_for or None)
def _ops():
    return {
        "ntt": (G_FULL, 1, [0], [0], lambda g, s: g.poly_ntt(s[0], 1), 1),
        "invntt": (G_FULL, 1, [0], [0], lambda g, s: g.poly_invntt(s[0], 1), 1),
        "ntt_reference": (G_FULL, 1, [0], [0], lambda g, s: g.poly_ntt_reference(s[0], 1, inverse=False), None),
        "invntt_reference": (G_FULL, 1, [0], [0], lambda g, s: g.poly_ntt_reference(s[0], 1, inverse=True), None),
        "rns_mul": (G_FULL, 3, [1, 2], [0], lambda g, s: g.poly_rns_mul(s[0], s[1], s[2], 1), None),
        "rns_add": (G_FULL, 3, [1, 2], [0], lambda g, s: g.poly_rns_add(s[0], s[1], s[2], 1), None),
        "poly_mul_rns": (G_FULL // 2, 3, [1, 2], [0], lambda g, s: g.poly_mul_rns(s[0], s[1], s[2], 1), 3),
        "mulpt_rns": (G_FULL // 4, 5, [2, 3, 4], [0, 1], lambda g, s: g.mulpt_rns(s[0], s[1], s[2], s[3], s[4], 1), 5),
    }


def _oracle(o, name, x):
    """the reference's words for one polynomial; x = host rows of the input slabs"""
    if name in ("ntt", "ntt_reference"):
        return [o.ntt(x[0], 0)]
    if name in ("invntt", "invntt_reference"):
        return [o.invntt(x[0], 0)]
    if name == "rns_mul":
        return [o.rns_mul(x[0], x[1], 0)]
    if name == "rns_add":
        return [o.rns_add(x[0], x[1], 0)]
    if name == "poly_mul_rns":
        return [o.poly_mul_rns(x[0], x[1], 1)]
    m, x0, x1 = x
    return [o.poly_mul_rns(m, x0, 1), o.poly_mul_rns(m, x1, 1)]   # src/he-mult.c:179-185: r0 = m * x0, r1 = m * x1


@pytest.mark.timeout(900)
@pytest.mark.parametrize("logn", [7, 13])
@pytest.mark.parametrize("name", list(_ops()))
def test_one_call_over_several_launch_groups(oracle_ctx, logn, name):
    import torch
    G, nslab, ins, outs, call, nt_slabs = _ops()[name]
    g, o = _ctx(logn), oracle_ctx(logn, 1)
    n, p = o.n, o.p[0]
    batch = 2 * G + 1
    if logn == 13 and nt_slabs is not None:
        # both cache-policy instantiations run inside this one call: full groups non-temporal, the tail not
        assert nt_for(logn, G, 1, nt_slabs) == 1 and nt_for(logn, batch - 2 * G, 1, nt_slabs) == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7000 + 31 * logn + len(name))
    src = []
    for k in range(nslab):
        if k not in ins:
            src.append(torch.empty(batch * n, dtype=torch.int64, device="cuda"))
        elif name.endswith("_reference"):                          # src/ntt.c as written takes any words
            src.append(torch.randint(-2 ** 63, 2 ** 63 - 1, (batch * n,), dtype=torch.int64, device="cuda", generator=gen))
        else:
            src.append(torch.randint(0, p, (batch * n,), dtype=torch.int64, device="cuda", generator=gen))
    idx = _anchors(G, batch, 31 + logn)
    host_in = [_rows(src[k], n, idx) for k in ins]
    split = [t.clone() for t in src]
    try:
        call(g, src)                                                # one call: groups 0, 1 and the one-polynomial tail
        cuts = _cuts(G, batch)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            call(g, [t[lo * n:hi * n] for t in split])
        torch.cuda.synchronize()
        for j in outs:
            assert torch.equal(src[j], split[j]), "%s n=2^%d: one call over %d groups differs from calls of at most %d polynomials" % (
                name, logn, (batch + G - 1) // G, G)
        got = [_rows(src[j], n, idx) for j in outs]
        for r, k in enumerate(idx):
            want = _oracle(o, name, [h[r] for h in host_in])
            for j, w in enumerate(want):
                assert np.array_equal(got[j][r], w), "%s n=2^%d: polynomial %d (group %d) output %d differs from the oracle" % (
                    name, logn, k, k // G, j)
    finally:
        del src, split
        g.close()
        _free()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("logn", [7, 13])
def test_gpq_ntt_zero_flags_in_every_launch_group(oracle_ctx, logn):
    """Inputs whose transform holds residues 0 (tests/zero_cases.py: the reference stores p there, src/ntt.c:47, and gpq_ntt
    redoes the flagged limbs with src/ntt.c's own arithmetic) at the ends of every launch group -- indices G-1, G and 2G and
    their neighbours -- must come out as the oracle's words; the next call, on data without such cases, must not see a stale flag."""
    import torch
    from gpqhe_amd import to_device
    G = G_FULL
    batch = 2 * G + 1
    g, o = _ctx(logn), oracle_ctx(logn, 1)
    n, p = o.n, o.p[0]
    names, cases = slab_of_cases(o, 1, 500 + logn)
    cases = cases.reshape(len(names), n)
    m = len(names)
    places = {}
    for j in range(m):
        places[G - 1 - j] = j                                       # the end of group 0
        places[G + j] = j                                           # the start of group 1
        places[2 * G - j] = j                                       # the tail (2G) and the end of group 1
    gen = torch.Generator(device="cuda")
    gen.manual_seed(8100 + logn)
    try:
        for rnd in range(2):
            x = torch.randint(0, p, (batch * n,), dtype=torch.int64, device="cuda", generator=gen)
            idx = _anchors(G, batch, 61 + logn + rnd)
            if rnd == 0:
                where = sorted(places)
                x.view(batch, n)[torch.tensor(where, device="cuda")] = to_device(cases[[places[k] for k in where]])
                idx = sorted(set(idx) | set(where))
            host_in = _rows(x, n, idx)
            split = x.clone()
            g.poly_ntt(x, 1)
            cuts = _cuts(G, batch)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                g.poly_ntt(split[lo * n:hi * n], 1)
            torch.cuda.synchronize()
            assert torch.equal(x, split), "gpq_ntt n=2^%d call %d: one call over three groups differs from smaller calls" % (logn, rnd)
            got = _rows(x, n, idx)
            for r, k in enumerate(idx):
                want = o.ntt(host_in[r], 0)
                label = names[places[k]] if (rnd == 0 and k in places) else "random"
                assert np.array_equal(got[r], want), "gpq_ntt n=2^%d call %d: polynomial %d (group %d, %s) differs from the oracle" % (
                    logn, rnd, k, k // G, label)
            if rnd == 0:
                assert any(np.any(got[r] == p) for r, k in enumerate(idx) if k in places), "no output held p: the zero cases did not engage"
            del x, split
    finally:
        g.close()
        _free()


# ---- bridge launches whose grid carries the batch in y (bridge_launch.hpp, bridge.hip): a batch above 65 535 polynomials ----------------------------

BRIDGE_BATCH = 65537


def _neg_words(a):
    """two's complement negation of [..][W][n] word slabs, wrapping at 2^(64 W)"""
    out = np.empty_like(a)
    carry = np.ones(a.shape[:1] + a.shape[2:], dtype=bool)
    for j in range(a.shape[1]):
        s = ~a[:, j] + carry.astype(np.uint64)
        out[:, j] = s
        carry = carry & (s == 0)
    return out


def _add_words(a, b):
    out = np.empty_like(a)
    carry = np.zeros(a.shape[:1] + a.shape[2:], dtype=bool)
    for j in range(a.shape[1]):
        s1 = a[:, j] + b[:, j]
        s2 = s1 + carry.astype(np.uint64)
        carry = (s1 < a[:, j]) | (s2 < s1)
        out[:, j] = s2
    return out


def _smod_words(a, logql):
    """mpi_smod(v mod 2^logql, 2^logql) (oracle/bigint_ref.py) on two's complement word slabs: the low logql bits, sign-extended"""
    out = a.copy()
    w, sb = (logql - 1) // 64, (logql - 1) % 64
    sign = (a[:, w] >> np.uint64(sb)) & np.uint64(1)
    low = np.uint64((1 << (sb + 1)) - 1) if sb < 63 else np.uint64(0xFFFFFFFFFFFFFFFF)
    out[:, w] = (a[:, w] & low) | (sign * ~low)
    for j in range(w + 1, a.shape[1]):
        out[:, j] = sign * np.uint64(0xFFFFFFFFFFFFFFFF)
    return out


def _permute_words(a, dst, neg):
    sel = np.where(neg[None, None, :], _neg_words(a), a)
    out = np.empty_like(a)
    out[:, :, dst] = sel
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("W", [1, 2])
def test_bridge_batch_above_the_grid_y_limit(W):
    """gpq_poly_rot / gpq_poly_conj (src/poly.c:263-283), gpq_big_add / sub / neg (src/he-add.c: mpi_addm / mpi_subm + mpi_smod,
    q_l = 2^logql), gpq_big_addsub (the same before mpi_smod, wrapping) and gpq_big_transpose at batch 65 537, n = 64: every
    polynomial against a numpy restatement, and the polynomials at the 65 535 / 65 536 boundary also against oracle/bigint_ref."""
    import ctypes as C
    import torch
    import oracle.bigint_ref as ref
    from gpqhe_amd import big_to_ints, to_device
    logn, batch = 6, BRIDGE_BATCH
    n = 1 << logn
    logql = 60 if W == 1 else 100
    ql = 1 << logql
    g = _ctx(logn)
    rng = np.random.default_rng(600 + W)
    a = rng.integers(0, 1 << 64, size=(batch, W, n), dtype=np.uint64, endpoint=False)
    b = rng.integers(0, 1 << 64, size=(batch, W, n), dtype=np.uint64, endpoint=False)
    a[0, :, :4] = b[0, :, :4] = 0
    a[-1, :, 0] = b[-1, :, 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    da, db = to_device(a.reshape(-1)), to_device(b.reshape(-1))
    r = torch.empty_like(da)
    P = lambda t: C.c_void_p(t.data_ptr())
    st = g._stream()
    check = [0, 65534, 65535, batch - 1]
    ints_a = big_to_ints(a[check], W, n)
    ints_b = big_to_ints(b[check], W, n)

    def got():
        torch.cuda.synchronize()
        return to_host(r).reshape(batch, W, n)

    def same(name, want, anchor=None):
        out = got()
        bad = np.flatnonzero(np.any(out != want, axis=(1, 2)))
        assert bad.size == 0, "%s W=%d batch=%d: %d polynomials differ, the first %d" % (name, W, batch, bad.size, bad[0])
        if anchor is not None:
            ints = big_to_ints(out[check], W, n)
            for t, k in enumerate(check):
                assert ints[t] == anchor(ints_a[t], ints_b[t]), "%s W=%d: polynomial %d differs from oracle/bigint_ref" % (name, W, k)

    try:
        i = np.arange(n)
        for rot in (1, 3):
            power = pow(5, rot, 1 << 64)
            k = (i * power) % (2 * n)
            g.poly_rot(r, da, W, rot)
            same("gpq_poly_rot(%d)" % rot, _permute_words(a, np.where(k < n, k, k - n), k >= n), lambda x, y: ref.poly_rot(x, rot))
        g.poly_conj(r, da, W)
        same("gpq_poly_conj", _permute_words(a, (n - i) % n, i != 0), lambda x, y: ref.poly_conj(x))

        assert g.lib.gpq_big_add(g.h, P(r), P(da), P(db), W, logql, batch, st) == 0, g.lib.gpq_last_error()
        same("gpq_big_add", _smod_words(_add_words(a, b), logql), lambda x, y: [ref.mpi_smod((u + v) % ql, ql) for u, v in zip(x, y)])
        assert g.lib.gpq_big_sub(g.h, P(r), P(da), P(db), W, logql, batch, st) == 0, g.lib.gpq_last_error()
        same("gpq_big_sub", _smod_words(_add_words(a, _neg_words(b)), logql), lambda x, y: [ref.mpi_smod((u - v) % ql, ql) for u, v in zip(x, y)])
        assert g.lib.gpq_big_neg(g.h, P(r), P(da), W, logql, batch, st) == 0, g.lib.gpq_last_error()
        same("gpq_big_neg", _smod_words(_neg_words(a), logql), lambda x, y: [ref.mpi_smod(-u, ql) for u in x])

        mod = 1 << (64 * W)
        wrap = lambda v: v - mod if v >> (64 * W - 1) else v
        g.big_addsub(r, da, db, W, 0)
        same("gpq_big_addsub +", _add_words(a, b), lambda x, y: [wrap((u + v) % mod) for u, v in zip(x, y)])
        g.big_addsub(r, da, db, W, 1)
        same("gpq_big_addsub -", _add_words(a, _neg_words(b)), lambda x, y: [wrap((u - v) % mod) for u, v in zip(x, y)])
        g.big_addsub(r, da, None, W, 2)
        same("gpq_big_addsub neg", _neg_words(a), lambda x, y: [wrap(-u % mod) for u in x])

        rows = np.ascontiguousarray(a.transpose(0, 2, 1))                  # [batch][n][W]: coefficient i's words at i*W + j
        assert g.lib.gpq_big_transpose(g.h, P(r), P(da), W, batch, 1, st) == 0, g.lib.gpq_last_error()
        torch.cuda.synchronize()
        out = to_host(r).reshape(batch, n, W)
        bad = np.flatnonzero(np.any(out != rows, axis=(1, 2)))
        assert bad.size == 0, "gpq_big_transpose to rows W=%d: %d polynomials differ, the first %d" % (W, bad.size, bad[0])
        drows = to_device(rows.reshape(-1))
        assert g.lib.gpq_big_transpose(g.h, P(r), P(drows), W, batch, 0, st) == 0, g.lib.gpq_last_error()
        same("gpq_big_transpose to words", a)
    finally:
        g.close()
        _free()
