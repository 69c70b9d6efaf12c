"""The conditional subtraction of gpqhe_amd/csrc/modarith.hpp (csub_by) narrows the wave's lane mask to the lanes that subtract, adds -m
under it and restores the mask itself.  What can go wrong there is not the arithmetic but the mask: a lane that should not subtract does,
a mask restored too wide wakes lanes that had returned, a mask left narrow silences lanes that should go on.  So:

  the primitive   gpq_modprobe_run_csub_lanes (libgpqhe_modprobe.so) runs csub1 .. csub4 at x in {0, m-1, m, m+1, 2m-1} for a wide-, a
                  split- and a plain-class modulus with every lane of a wave subtracting, none (the add runs under an empty mask), every
                  other one, in workgroups of 96 (the second wave starts half off), with lanes outside the branch that subtracts and with
                  the last lanes of the launch returned early; every word a lane must not write keeps the caller's fill.
  the kernels     poly_ntt / poly_invntt, he_mul_tensor and he_keyswitch against the oracle, bit for bit: n = 2^13, 3 limbs, 3 polynomials
                  in launch groups of 2 (the odd one runs the key switch's single form), both cache policies, all limbs in each butterfly
                  class; n = 2^17, one polynomial over the limbs up to the second of the split class.  Inputs: zero, p - 1, uniform, and 0 /
                  p - 1 alternating by lane (every other lane of a wave subtracts in the first stages).

No tolerance anywhere.  tools/csub_model.cpp is the same statement about the integer model, on the host."""
import ctypes as C

import numpy as np
import pytest

from gpqhe_amd import to_device, to_host
from tests import modarith_cases as mc

pytestmark = pytest.mark.gpu
u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_ubyte)
FILL0, FILL1 = 0xDEADBEEFDEADBEEF, 0xFEEDFACEFEEDFACE


@pytest.fixture(scope="module")
def probe():
    try:
        import torch  # noqa: F401  (one HIP runtime for the whole process, as gpqhe_amd._native.load)
    except ImportError:
        pass
    lib = C.CDLL(mc.PROBE_PATH)
    lib.gpq_modprobe_run_csub_lanes.restype = C.c_int
    lib.gpq_modprobe_run_csub_lanes.argtypes = [C.c_int, C.c_uint64, u64p, u8p, u64p, u64p, C.c_size_t, C.c_uint, C.c_uint]
    return lib


def class_moduli():
    """one modulus per butterfly class: the smallest c (wide), the first c at or above the wide limit (split), the largest c of all (plain)"""
    ms = sorted(mc.moduli(), key=lambda m: m.c)
    wide, split, plain = ms[0], next(m for m in ms if m.c >= mc.WIDE_CMAX), ms[-1]
    assert wide.admits("wide") and split.admits("split") and not split.admits("wide") and plain.admits("fold") and not plain.admits("split")
    return [wide, split, plain]


def lane_patterns(m, threads, blocks):
    """name -> (x, on, count) over threads * blocks lanes.  `taken` = x >= m."""
    cap = threads * blocks
    lo, hi = [0, m - 1], [m, m + 1, 2 * m - 1]
    edge = [0, m - 1, m, m + 1, 2 * m - 1]
    ones = np.ones(cap, dtype=np.uint8)
    pick = lambda vals, idx: np.array([vals[i % len(vals)] for i in idx], dtype=np.uint64)
    lanes = np.arange(cap)
    out = {
        "all lanes taken": (pick(hi, lanes), ones, cap),
        "no lane taken": (pick(lo, lanes), ones, cap),
        "alternating lanes": (np.where(lanes % 2 == 0, pick(hi, lanes // 2), pick(lo, lanes // 2)).astype(np.uint64), ones, cap),
        "every edge value in turn": (pick(edge, lanes), ones, cap),
        "lanes outside the branch": (pick(edge, lanes), (lanes % 3 != 1).astype(np.uint8), cap),
        "last lanes return early": (pick(edge, lanes), ones, cap - 37),
        "early return and branch, taken lanes only": (pick(hi, lanes), (lanes % 5 != 0).astype(np.uint8), cap - cap // 3 - 1),
    }
    return out


@pytest.mark.parametrize("threads,blocks", [(64, 1), (96, 2), (256, 2)])
def test_masked_subtraction_per_lane(probe, threads, blocks):
    for mod in class_moduli():
        for mul in (1, 2, 3, 4):
            m = mul * mod.p
            for name, (x, on, count) in lane_patterns(m, threads, blocks).items():
                cap = threads * blocks
                out0, out1 = np.full(cap, FILL0, dtype=np.uint64), np.full(cap, FILL1, dtype=np.uint64)
                x, on = np.ascontiguousarray(x), np.ascontiguousarray(on)
                rc = probe.gpq_modprobe_run_csub_lanes(mul, mod.p, x.ctypes.data_as(u64p), on.ctypes.data_as(u8p), out0.ctypes.data_as(u64p),
                                                       out1.ctypes.data_as(u64p), count, threads, blocks)
                assert rc == 0, "gpq_modprobe_run_csub_lanes returned HIP error %d" % rc
                xi = x.astype(object)
                sub = np.array([int(v) - m if int(v) >= m else int(v) for v in xi], dtype=np.uint64)
                live = np.arange(cap) < count
                inside = live & (on != 0)
                want0 = np.where(inside, sub, np.uint64(FILL0))
                want1 = np.where(inside, sub, np.where(live, x, np.uint64(FILL1)))
                where = "csub%d mod %s, %d x %d lanes, %s" % (mul, mod.label, blocks, threads, name)
                assert np.array_equal(out0, want0), "%s: inside the branch, first bad lane %d" % (where, int(np.flatnonzero(out0 != want0)[0]))
                assert np.array_equal(out1, want1), "%s: behind the branch, first bad lane %d" % (where, int(np.flatnonzero(out1 != want1)[0]))


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("zero", "p-1", "uniform", "alternating 0 / p-1")


def slab_of(o, pattern, seed, dim, batch):
    n = o.n
    if pattern == "uniform":
        return np.concatenate([o.gen(seed + k, dim) for k in range(batch)])
    out = np.zeros((batch, dim, n), dtype=np.uint64)
    if pattern != "zero":
        step = 2 if pattern.startswith("alt") else 1          # alternating: even lanes stay zero
        for d in range(dim):
            out[:, d, step - 1::step] = np.uint64(o.p[d] - 1)
    return out.reshape(-1)


_EXPECTED = {}


def expected(o, pattern, dim, batch):
    """inputs and the oracle's outputs for one (context, pattern): computed once, shared by every setting, never written to"""
    key = (o.logn, dim, batch, pattern)
    if key not in _EXPECTED:
        per = dim * o.n
        ins = [slab_of(o, pattern, 40 + 10 * s, dim, batch) for s in range(5)]      # a0 a1 b0 b1 x
        evk = [o.gen(7300, dim), o.gen(7301, dim)]
        exp = {"ntt": o.ntt_slab(ins[0], dim), "invntt": o.ntt_slab(ins[1], dim, inverse=True), "tensor": [[], [], []], "ks": [[], []]}
        for k in range(batch):
            sl = slice(k * per, (k + 1) * per)
            for acc, e in zip(exp["tensor"], o.he_mul_tensor(*[v[sl].copy() for v in ins[:4]], dim)):
                acc.append(e)
            for acc, f in zip(exp["ks"], o.keyswitch(ins[4][sl].copy(), evk[0], evk[1], dim)):
                acc.append(f)
        exp["tensor"] = [np.concatenate(a) for a in exp["tensor"]]
        exp["ks"] = [np.concatenate(a) for a in exp["ks"]]
        for v in ins + evk + [exp["ntt"], exp["invntt"]] + exp["tensor"] + exp["ks"]:
            v.setflags(write=False)
        _EXPECTED[key] = (ins, evk, exp)
    return _EXPECTED[key]


def run_and_compare(g, o, pattern, dim, batch, where):
    import torch
    ins, evk, exp = expected(o, pattern, dim, batch)
    dev = [to_device(np.array(v)) for v in ins]
    dk = [to_device(np.array(v)) for v in evk]
    a = dev[0].clone(); g.poly_ntt(a, dim)
    b = dev[1].clone(); g.poly_invntt(b, dim)
    d = [torch.empty_like(dev[0]) for _ in range(3)]
    g.he_mul_tensor(d[0], d[1], d[2], dev[0], dev[1], dev[2], dev[3], dim)
    c = [torch.empty_like(dev[0]) for _ in range(2)]
    g.he_keyswitch(c[0], c[1], dev[4], dk[0], dk[1], dim)
    torch.cuda.synchronize()
    got = [a, b] + d + c
    want = [exp["ntt"], exp["invntt"]] + exp["tensor"] + exp["ks"]
    for name, t, w in zip(("poly_ntt", "poly_invntt", "d0", "d1", "d2", "c0", "c1"), got, want):
        assert np.array_equal(to_host(t), w), "%s: %s differs from the oracle" % (where, name)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_kernels_match_oracle_in_every_class_and_policy(oracle_ctx, pattern):
    import gpqhe_amd
    logn, dim, batch = 13, 3, 3
    o = oracle_ctx(logn, dim)
    g = gpqhe_amd.PolyContext(logn, dim)          # own context: the session-wide ones keep their defaults
    try:
        g.set_chunk(2)
        for label, (wide, split) in (("wide", (dim, dim)), ("split", (0, dim)), ("plain", (0, 0)), ("one limb of each", (1, 2))):
            g.set_limb_classes(wide, split)
            for policy in (0, 1):
                g.set_nt_policy(policy)
                run_and_compare(g, o, pattern, dim, batch, "n = 2^13, %s, %s limbs, nt policy %d" % (pattern, label, policy))
    finally:
        g.close()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_kernels_match_oracle_into_the_split_class_at_n17(oracle_ctx, pattern):
    import gpqhe_amd
    logn = 17
    chain = oracle_ctx(logn, 45)
    first_split = next(d for d, p in enumerate(chain.p) if p - mc.B59 >= mc.WIDE_CMAX)
    dim = first_split + 2
    assert 2 < dim <= 45 and chain.p[dim - 1] - mc.B59 < mc.SPLIT_CMAX
    o = oracle_ctx(logn, dim)
    assert o.p == chain.p[:dim]
    g = gpqhe_amd.PolyContext(logn, dim)
    try:
        for policy in (0, 1):
            g.set_nt_policy(policy)
            run_and_compare(g, o, pattern, dim, 1, "n = 2^17, %d limbs (split class from limb %d), %s, nt policy %d" % (dim, first_split, pattern, policy))
    finally:
        g.close()
