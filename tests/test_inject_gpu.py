"""The butterflies with the (c+1) correction folded into mad addends (gpqhe_amd/csrc/modarith.hpp: mulmod_split, mulmod_raw_t)
against the oracle, word for word: every butterfly class, the smallest two-pass ring and the nine-low-stage ring, an odd batch,
every fused middle (tensor, squaring, key switch in its pair and single forms, poly_mul, he_mulpt) under both cache policies,
and the inputs that sit on the edges of the lazy ranges -- all-zero, all p - 1, and polynomials whose transform holds
residues 0 (a lazy value may now be 0 where it was p; canonical outputs, and the reference's stored p, must not move).
The integer model of the same code is tests/test_inject_ranges.py.

The matrix: a launch of a transform kernel is one instantiation out of ring (5, 6, 7, 8 strided stages at logn 13 .. 16, nine low stages
at 17) x butterfly class x cache policy, and the range a strided pass hands to the middle depends on the class and on how many stages
ran.  So every ring 13 .. 17 has a case with one limb range of each class inside one transform, ring 15 -- which nothing else runs --
also every uniform arrangement, all under both policies.  gpq_set_limb_classes clamps silently: each case first proves from the
per-kernel profile that the classes it asked for are the classes that ran.  tests/test_ring_class_cover.py pins the table."""
import numpy as np
import pytest

import gpqhe_amd
from gpqhe_amd import to_device, to_host
from tests.zero_cases import limb_cases

pytestmark = pytest.mark.gpu

BATCH = 3      # odd: the key switch runs a pair of polynomials and then the single-polynomial instantiation
# (logn, limbs, (wide, split)): logn 13 is the smallest two-pass ring, three limbs of each class inside one transform
# (gpq_set_limb_classes as tests/test_ntt_gpu.py uses it: the first `wide` limbs wide-split, up to `split` split, the rest 7-mad);
# logn 17 (nine low stages) with two limbs, both through each class in turn; then the smallest all-class cell of the other rings and of
# 17 -- three limbs, one of each class -- and at ring 15 the uniform arrangements on the same three limbs (one range of three limbs)
CASES = [(13, 9, (3, 6)), (17, 2, (2, 2)), (17, 2, (0, 2)), (17, 2, (0, 0)),
         (14, 3, (1, 2)), (15, 3, (1, 2)), (16, 3, (1, 2)), (17, 3, (1, 2)), (15, 3, (0, 0)), (15, 3, (0, 3)), (15, 3, (3, 3))]
NT_POLICIES = [0, 1]


def class_ranges(dim, classes):
    """Limbs per class (wide-split, split, 7-mad) of a transform over limbs 0 .. dim - 1 under gpq_set_limb_classes(*classes), when nothing
    is clamped.  engine.hip, for_limb_ranges: e_wide = min(nwide, dim), e_split = min(nsplit, dim), and one call of f -- one ProfScope and
    one launch in launch_strided / launch_contig -- per non-empty range [0, e_wide), [e_wide, e_split), [e_split, dim)."""
    wide, split = classes
    e_split = min(split, dim)
    e_wide = min(wide, e_split)
    return e_wide, e_split - e_wide, dim - e_split


def launches(dim, classes):
    return sum(1 for limbs in class_ranges(dim, classes) if limbs)


_SHARED = {}


def _inputs(o, logn, dim):
    """Per ring, built once: slabs of BATCH polynomials.  `edge` = [zero residues in the transform, all-zero, all p - 1],
    `mix` = [random, lower half of the transform zero, random]; `rnd` x 2; one key pair."""
    if (logn, dim) in _SHARED:
        return _SHARED[logn, dim]
    n = o.n
    rng = np.random.default_rng(1700 + logn)
    cases = [dict(limb_cases(o, d, rng)) for d in range(dim)]
    zeros = np.zeros(n, dtype=np.uint64)
    scattered = np.concatenate([cases[d]["scattered zeros"] for d in range(dim)])
    half = np.concatenate([cases[d]["lower half zero"] for d in range(dim)])
    pmax = np.concatenate([np.full(n, o.p[d] - 1, dtype=np.uint64) for d in range(dim)])
    edge = np.concatenate([scattered, np.tile(zeros, dim), pmax])
    mix = np.concatenate([o.gen(31, dim), half, o.gen(32, dim)])
    rnd = [np.concatenate([o.gen(40 + 10 * s + k, dim) for k in range(BATCH)]) for s in range(2)]
    keys = [o.gen(7000, dim), o.gen(7001, dim)]
    per = dim * n
    exp = {"ntt": [o.ntt_slab(v, dim) for v in (edge, mix)], "invntt": [o.ntt_slab(v, dim, inverse=True) for v in (edge, mix)]}
    quad = (edge, mix, rnd[0], rnd[1])
    exp["tensor"] = [o.he_mul_tensor(*[v[k * per:(k + 1) * per].copy() for v in quad], dim) for k in range(BATCH)]
    exp["square"] = [o.he_mul_tensor(*[v[k * per:(k + 1) * per].copy() for v in (edge, mix, edge, mix)], dim) for k in range(BATCH)]
    exp["keyswitch"] = [[o.keyswitch(x[k * per:(k + 1) * per].copy(), keys[0], keys[1], dim) for k in range(BATCH)] for x in (edge, mix)]
    one = lambda v, k: v[k * per:(k + 1) * per].copy()
    exp["polymul"] = [o.poly_mul_rns(one(edge, k), one(mix, k), dim) for k in range(BATCH)]
    exp["mulpt"] = [[o.poly_mul_rns(one(rnd[0], k), one(x, k), dim) for k in range(BATCH)] for x in (edge, mix)]     # m x0, m x1
    _SHARED[logn, dim] = (edge, mix, rnd, keys, exp)
    return _SHARED[logn, dim]


def assert_the_asked_classes_ran(g, slab, dim, classes):
    """One gpq_ntt and one gpq_invntt of one launch group under the profile: each pass records one launch per class present.
    Three launches on three ranges can only be one of each class.  One launch of a uniform arrangement is the asked class only next to
    the mixed case of the same ring: a wide range clamped to 0 (or split tables for 0 limbs) would also launch once, and then (1, 2) on
    a context built the same way launches twice; any other clamp splits the uniform range in two."""
    want = launches(dim, classes)
    dev = to_device(slab)
    try:
        g.profile(True)
        g.profile_collect()
        g.poly_ntt(dev, dim)
        fwd = g.profile_collect()
        g.poly_invntt(dev, dim)
        inv = g.profile_collect()
    finally:
        g.profile(False)                             # (gpq_set_overlap lanes are not taken while it is on)
    cnt = lambda prof, k: prof.get(k, (0, 0))[1]
    for prof, names in ((fwd, ("strided_fwd", "contig_fwd")), (inv, ("contig_inv", "strided_inv"))):
        for name in names:
            assert cnt(prof, name) == want, "%s: %d launches, classes %s on %d limbs are %d (limbs per class %s): gpq_set_limb_classes clamped" % (
                name, cnt(prof, name), classes, dim, want, class_ranges(dim, classes))


@pytest.mark.parametrize("ran", [(0, 2), (1, 1), (0, 0)])
def test_a_context_that_runs_fewer_classes_than_asked_fails_the_proof(ran):
    """What a clamp would leave -- the wide range ended at limb 0, split tables for one limb only, neither -- is told from (1, 2)."""
    logn, dim = 13, 3
    g = gpqhe_amd.PolyContext(logn, dim)
    try:
        g.set_limb_classes(*ran)
        slab = np.zeros(BATCH * dim << logn, dtype=np.uint64)
        assert_the_asked_classes_ran(g, slab, dim, ran)
        with pytest.raises(AssertionError, match="clamped"):
            assert_the_asked_classes_ran(g, slab, dim, (1, 2))
    finally:
        g.close()


@pytest.mark.parametrize("nt", NT_POLICIES)     # both cache-policy instantiations of every kernel (the expectations are cached per ring)
@pytest.mark.parametrize("logn,dim,classes", CASES)
def test_injected_butterflies_match_the_oracle(oracle_ctx, logn, dim, classes, nt):
    import torch
    o = oracle_ctx(logn, dim)
    edge, mix, rnd, keys, exp = _inputs(o, logn, dim)
    g = gpqhe_amd.PolyContext(logn, dim)           # own context: the session-wide ones keep their classes
    try:
        assert g.p == o.p
        g.set_limb_classes(*classes)
        g.set_nt_policy(nt)
        assert_the_asked_classes_ran(g, mix, dim, classes)
        per = dim * o.n
        for i, v in enumerate((edge, mix)):          # gpq_ntt, gpq_invntt
            dev = to_device(v)
            g.poly_ntt(dev, dim)
            assert np.array_equal(to_host(dev), exp["ntt"][i]), "gpq_ntt, slab %d" % i
            dev = to_device(v)
            g.poly_invntt(dev, dim)
            assert np.array_equal(to_host(dev), exp["invntt"][i]), "gpq_invntt, slab %d" % i
        de, dm, r0, r1 = (to_device(v) for v in (edge, mix, rnd[0], rnd[1]))
        outs = [torch.empty_like(de) for _ in range(3)]
        g.he_mul_tensor(outs[0], outs[1], outs[2], de, dm, r0, r1, dim)          # gpq_he_mul_tensor: a general product
        got = [to_host(t) for t in outs]
        for k in range(BATCH):
            for name, a, b in zip(("d0", "d1", "d2"), got, exp["tensor"][k]):
                assert np.array_equal(a[k * per:(k + 1) * per], b), "tensor %s of ciphertext %d" % (name, k)
        g.he_mul_tensor(outs[0], outs[1], outs[2], de, dm, de, dm, dim)          # ... and a squaring (aliased operands)
        got = [to_host(t) for t in outs]
        for k in range(BATCH):
            for name, a, b in zip(("d0", "d1", "d2"), got, exp["square"][k]):
                assert np.array_equal(a[k * per:(k + 1) * per], b), "squaring %s of ciphertext %d" % (name, k)
        k0, k1 = to_device(keys[0]), to_device(keys[1])
        for i, x in enumerate((de, dm)):             # gpq_keyswitch
            c0, c1 = torch.empty_like(x), torch.empty_like(x)
            g.he_keyswitch(c0, c1, x, k0, k1, dim)
            h0, h1 = to_host(c0), to_host(c1)
            for k in range(BATCH):
                f0, f1 = exp["keyswitch"][i][k]
                assert np.array_equal(h0[k * per:(k + 1) * per], f0) and np.array_equal(h1[k * per:(k + 1) * per], f1), "key switch, slab %d, polynomial %d" % (i, k)
        r = torch.empty_like(de)                     # gpq_poly_mul_rns (it overwrites its inputs: clones)
        g.poly_mul_rns(r, de.clone(), dm.clone(), dim)
        assert np.array_equal(to_host(r), np.concatenate(exp["polymul"])), "gpq_poly_mul_rns"
        p0, p1 = torch.empty_like(de), torch.empty_like(de)   # gpq_mulpt_rns: m x0, m x1 (clones again)
        g.mulpt_rns(p0, p1, r0.clone(), de.clone(), dm.clone(), dim)
        assert np.array_equal(to_host(p0), np.concatenate(exp["mulpt"][0])), "gpq_mulpt_rns, m x0"
        assert np.array_equal(to_host(p1), np.concatenate(exp["mulpt"][1])), "gpq_mulpt_rns, m x1"
    finally:
        g.close()
