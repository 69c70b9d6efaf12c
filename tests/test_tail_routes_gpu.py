"""Which kernels the relinearisation tail launches on each of its routes, and that every route writes the reference's words.

relin_tail (gpqhe_amd/csrc/bridge_tail.hpp) is a router over three flows -- the one-product tail (as a stream, or as one matrix product),
the matrix-core front, the integer-VALU exact tail -- plus the un-weighting fall-back of the one-product tail.  Each case below reaches one route by the smallest shape that does, compares every output word with the restated
reference (oracle/bigint_ref), and pins the number of profiled launches per class (gpq_profile_collect: one record per ProfScope).  The
counts do not depend on the data: the masked kernels are launched whether or not a coefficient is flagged.  They were recorded from the
build BEFORE the tail was split into flow functions, and each is the sum of the launches its comment names."""
import random

import numpy as np
import pytest

from gpqhe_amd import big_to_ints, ints_to_big, to_device, to_host
from oracle import bigint_ref as ref

pytestmark = pytest.mark.gpu

CLASSES = ("bridge_tail_stream", "bridge_relin_tail_direct", "bridge_relin_front", "bridge_reconstruct",
           "bridge_exact_paths", "bridge_rescale", "bridge_decompose", "bridge_crt_decompose")


def _torch():
    import torch
    return torch


def _profiled(g, call):
    """launches per class of one call"""
    g.profile(True)
    try:
        g.profile_collect()
        call()
        _torch().cuda.synchronize()
        prof = g.profile_collect()
    finally:
        g.profile(False)
    return {k: int(prof[k][1]) for k in CLASSES if k in prof}


# ---------------------------------------------------------------------------
# the bare tail: n = 2^7, one polynomial, dims of he_dims(logqL, logqL)
# ---------------------------------------------------------------------------
# route: (logqL, overwriting entry point, in place, launches per class)
BARE = {
    # dimP = 3: no matrix-core front (it needs 4 limbs of P).  exact: r (full-width CRT), bridge_exactdiv, the exact kernel behind Q's fast
    # CRT, bridge_addround; decompose: r over the limbs above P; reconstruct: Q's fast CRT
    "valu": (120, False, False, {"bridge_exact_paths": 4, "bridge_decompose": 1, "bridge_reconstruct": 1}),
    # front: bridge_relin_front_mfma; exact: r of the ambiguous coefficients, bridge_roundfix, the exact kernel behind Q's fast CRT,
    # bridge_addround; reconstruct: Q's fast CRT finishing into `out`
    "front": (200, False, False, {"bridge_relin_front": 1, "bridge_exact_paths": 4, "bridge_reconstruct": 1}),
    # the same launches with Q parked in the workspace (qc) and bridge_addround finishing every coefficient
    "front in place": (200, False, True, {"bridge_relin_front": 1, "bridge_exact_paths": 4, "bridge_reconstruct": 1}),
    # stream: bridge_tail_stream<6, 0, false, 3> (the weights go on outside the profile); exact: bridge_limb_scale, the front re-run,
    # bridge_fallback_tail_post<8, 16> (P is an 8-word basis, Pi' a 16-word one: r, its round bit, Q's exact CRT and the finish in one launch)
    "product": (438, True, False, {"bridge_tail_stream": 1, "bridge_exact_paths": 3}),
    # the product cannot run over its own addend: exact: bridge_limb_scale on every coefficient, then the "front" route's four;
    # front and reconstruct as there
    "product in place": (438, True, True, {"bridge_relin_front": 1, "bridge_exact_paths": 5, "bridge_reconstruct": 1}),
}


@pytest.mark.parametrize("route", list(BARE))
def test_bare_tail_routes(engine_ctx, oracle_ctx, route):
    torch = _torch()
    logqL, overwriting, in_place, want = BARE[route]
    logn = 7
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 12).he_dims(logqL, logqL)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    n, W, ql = g.n, (logqL + 64) // 64, 1 << logqL
    rng = random.Random(logqL)
    chat = np.array([rng.randrange(o.p[d]) for d in range(dimB) for _ in range(n)], dtype=np.uint64)
    dvals = [rng.randrange(-(ql // 2), ql // 2) for _ in range(n)]
    exp = ref.he_relin_tail(o, chat, chat, dvals, None, dimP, dimB, ql)[0]
    d = to_device(ints_to_big(dvals, W))
    out = d if in_place else torch.empty(W * n, dtype=torch.int64, device="cuda")
    tail = g.relin_tail_overwriting if overwriting else g.relin_tail
    got = _profiled(g, lambda: tail(out, to_device(chat), d, W, logqL, dimB, dimP))
    print("%s: %s" % (route, got))
    assert big_to_ints(to_host(out), W, n)[0] == exp
    assert got == want
    if route == "product in place":
        assert "bridge_relin_tail_direct" not in got and "bridge_tail_stream" not in got and "bridge_relin_front" in got


def test_bare_tail_product_as_one_matrix_product(engine_ctx, oracle_ctx):
    """The "product" route without the streaming kernel: bridge_reconstruct_low_mfma<16> with the tail's rows (bridge_relin_tail_direct)."""
    torch = _torch()
    logn, logqL = 7, 438
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 12).he_dims(logqL, logqL)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    n, W, ql = g.n, (logqL + 64) // 64, 1 << logqL
    rng = random.Random(logqL)
    chat = np.array([rng.randrange(o.p[d]) for d in range(dimB) for _ in range(n)], dtype=np.uint64)
    dvals = [rng.randrange(-(ql // 2), ql // 2) for _ in range(n)]
    exp = ref.he_relin_tail(o, chat, chat, dvals, None, dimP, dimB, ql)[0]
    out = torch.empty(W * n, dtype=torch.int64, device="cuda")
    try:
        g.set_stream_bridge(False)
        got = _profiled(g, lambda: g.relin_tail_overwriting(out, to_device(chat), to_device(ints_to_big(dvals, W)), W, logqL, dimB, dimP))
    finally:
        g.set_stream_bridge(True)
    print("product, separate kernels: %s" % got)
    assert big_to_ints(to_host(out), W, n)[0] == exp
    # direct: the product; exact: bridge_limb_scale, the front re-run, r, bridge_roundfix, Q's exact CRT, bridge_addround (the one-launch
    # post kernel only runs under the streaming kernel's per-wave words)
    assert got == {"bridge_relin_tail_direct": 1, "bridge_exact_paths": 6}


# ---------------------------------------------------------------------------
# whole calls: n = 2^13 (the smallest ring whose key switch pre-weights limbs), q_L = q_l = 2^200, two ciphertexts = one launch group
# ---------------------------------------------------------------------------
LOGN, LOGQ, LOGDELTA, BATCH = 13, 200, 30, 2

# dims 4/8/12, 4-word coefficients: every CRT basis here (P, Pi', P_A) is an 8-word one, and the fused fall-back kernels exist for larger
# ones only (bridge_fallback_crt_decompose and bridge_fallback_tail_pre: a 16- or 32-word P_A; bridge_fallback_tail_post: P + Pi' of 8 + 16
# or 16 + 32 words, as on the "product" route above) -- so the exact chains behind the streaming kernels are separate launches here, not the
# pre + front + post = 3 of the headline shape.
#   D  = bridge_decompose of the inputs (he_mul: all four in one launch; he_swk: d1)
#   d2 = behind bridge_crt_decompose: d2's exact CRT + the masked rns_decompose                                       (2 exact)
#   T7 = behind bridge_tail_stream with the addend as limbs: the addend's exact CRT, bridge_limb_scale, the front re-run, r,
#        bridge_roundfix, Q's exact CRT, bridge_addround                                                              (7 exact)
#   T6 = the same without an addend's CRT (he_swk)                                                                    (6 exact)
#   F4 = behind the matrix-core front: r of the ambiguous coefficients, bridge_roundfix, the exact kernel behind Q's fast CRT,
#        bridge_addround                                                                                              (4 exact)
#   A  = the exact kernel behind the fast CRT of d0 | d1 | d2 (or of d2 alone)                                        (1 exact)
WHOLE = {
    "default": {
        "he_mul": {"bridge_decompose": 1, "bridge_crt_decompose": 1, "bridge_tail_stream": 1, "bridge_exact_paths": 9},          # D; d2 + T7
        "he_mul_rs": {"bridge_decompose": 1, "bridge_crt_decompose": 1, "bridge_tail_stream": 1, "bridge_exact_paths": 10},      # ... + bridge_rescale_masked
        "he_swk": {"bridge_decompose": 1, "bridge_tail_stream": 1, "bridge_exact_paths": 6},                                      # D; T6
    },
    # the product as bridge_reconstruct_low_mfma<16>, its addend as words; he_mul: the fast CRT of d0 | d1 | d2 in one launch (reconstruct 1, A),
    # D + rns_decompose of d2 (decompose 2), T6 behind the product (exact 1 + 6); he_mul_rs: bridge_rescale on both outputs
    "separate kernels": {
        "he_mul": {"bridge_decompose": 2, "bridge_reconstruct": 1, "bridge_relin_tail_direct": 1, "bridge_exact_paths": 7},
        "he_mul_rs": {"bridge_decompose": 2, "bridge_reconstruct": 1, "bridge_relin_tail_direct": 1, "bridge_exact_paths": 7, "bridge_rescale": 2},
        "he_swk": {"bridge_decompose": 1, "bridge_relin_tail_direct": 1, "bridge_exact_paths": 6},
    },
    # the matrix-core front (w-scaled tables with 2, the plain ones with 1 and 0): he_mul: fast CRT of d0 | d1 | d2 + Q's fast CRT (reconstruct 2),
    # A + F4, D + rns_decompose of d2
    "prescale 2": {
        "he_mul": {"bridge_decompose": 2, "bridge_reconstruct": 2, "bridge_relin_front": 1, "bridge_exact_paths": 5},
        "he_mul_rs": {"bridge_decompose": 2, "bridge_reconstruct": 2, "bridge_relin_front": 1, "bridge_exact_paths": 5, "bridge_rescale": 2},
        "he_swk": {"bridge_decompose": 1, "bridge_reconstruct": 1, "bridge_relin_front": 1, "bridge_exact_paths": 4},
    },
    "prescale 1": {
        "he_mul": {"bridge_decompose": 2, "bridge_reconstruct": 2, "bridge_relin_front": 1, "bridge_exact_paths": 5},
        "he_mul_rs": {"bridge_decompose": 2, "bridge_reconstruct": 2, "bridge_relin_front": 1, "bridge_exact_paths": 5, "bridge_rescale": 2},
        "he_swk": {"bridge_decompose": 1, "bridge_reconstruct": 1, "bridge_relin_front": 1, "bridge_exact_paths": 4},
    },
    "prescale 0": {
        "he_mul": {"bridge_decompose": 2, "bridge_reconstruct": 2, "bridge_relin_front": 1, "bridge_exact_paths": 5},
        "he_mul_rs": {"bridge_decompose": 2, "bridge_reconstruct": 2, "bridge_relin_front": 1, "bridge_exact_paths": 5, "bridge_rescale": 2},
        "he_swk": {"bridge_decompose": 1, "bridge_reconstruct": 1, "bridge_relin_front": 1, "bridge_exact_paths": 4},
    },
}
# he_swk with out_c0 aliasing d0 under the defaults: the key switch has weighted the limbs for the product, which cannot run over its own
# addend -- exact: bridge_limb_scale on every coefficient + F4; front and Q's fast CRT as under "prescale 0"
SWK_IN_PLACE = {"bridge_decompose": 1, "bridge_relin_front": 1, "bridge_reconstruct": 1, "bridge_exact_paths": 5}

SETTINGS = {
    "default": (lambda g: None, lambda g: None),
    "separate kernels": (lambda g: g.set_stream_bridge(False), lambda g: g.set_stream_bridge(True)),
    "prescale 2": (lambda g: g.set_prescale(2), lambda g: g.set_prescale(g.PRESCALE_DEFAULT)),
    "prescale 1": (lambda g: g.set_prescale(1), lambda g: g.set_prescale(g.PRESCALE_DEFAULT)),
    "prescale 0": (lambda g: g.set_prescale(0), lambda g: g.set_prescale(g.PRESCALE_DEFAULT)),
}

_WHOLE = {}


def _whole(engine_ctx, oracle_ctx):
    """inputs and the reference's outputs, computed once for every setting"""
    if _WHOLE:
        return _WHOLE
    dimP, dimA, dimB, dimevk = ref.he_dims(LOGN, oracle_ctx(LOGN, 60).p, LOGQ, LOGQ)
    g, o = engine_ctx(LOGN, dimevk), oracle_ctx(LOGN, dimevk)
    assert g.he_dims(LOGQ, LOGQ) == (dimP, dimA, dimB, dimevk) == (4, 8, 12, 12)
    n, W = g.n, (LOGQ + 64) // 64
    rng = random.Random(LOGQ)
    h = 1 << (LOGQ - 1)
    cts = [[[rng.randrange(-h, h) for _ in range(n)] for _ in range(BATCH)] for _ in range(4)]      # a0, a1, b0, b1
    key = [o.gen(3000, dimevk), o.gen(3001, dimevk)]
    mul = [ref.he_mul(o, (cts[0][k], cts[1][k]), (cts[2][k], cts[3][k]), key[0], key[1], dimP, dimA, dimB, LOGQ) for k in range(BATCH)]
    swk = [ref.he_swk(o, cts[0][k], cts[1][k], key[0], key[1], dimP, dimB, LOGQ) for k in range(BATCH)]
    rs = lambda poly: [ref.mpi_smod(ref.mpi_rdiv(v, 1 << LOGDELTA), 1 << (LOGQ - LOGDELTA)) for v in poly]    # src/he-rescale.c:33-54
    _WHOLE.update(g=g, dims=(dimA, dimB, dimP), W=W,
                  cts=[to_device(np.concatenate([ints_to_big(v, W) for v in c])) for c in cts], key=[to_device(k) for k in key],
                  want={"he_mul": [[m[i] for m in mul] for i in (0, 1)], "he_swk": [[s[i] for s in swk] for i in (0, 1)],
                        "he_mul_rs": [[rs(m[i]) for m in mul] for i in (0, 1)]})
    return _WHOLE


def _run(case, name, out0=None):
    """one whole call: (launches per class, c0, c1 as lists of integers per ciphertext)"""
    torch = _torch()
    g, (dimA, dimB, dimP), W, cts, key = case["g"], case["dims"], case["W"], case["cts"], case["key"]
    o0 = torch.empty_like(cts[0]) if out0 is None else out0
    o1 = torch.empty_like(cts[0])
    if name == "he_mul":
        call = lambda: g.he_mul(o0, o1, *cts, key[0], key[1], W, LOGQ, dimA, dimB, dimP)
    elif name == "he_mul_rs":
        call = lambda: g.he_mul_rs(o0, o1, *cts, key[0], key[1], W, LOGQ, dimA, dimB, dimP, LOGDELTA)
    else:
        call = lambda: g.he_swk(o0, o1, cts[0] if out0 is None else out0, cts[1], key[0], key[1], W, LOGQ, dimB, dimP)
    got = _profiled(g, call)
    return got, big_to_ints(to_host(o0), W, g.n), big_to_ints(to_host(o1), W, g.n)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_whole_call_routes(engine_ctx, oracle_ctx, setting):
    case = _whole(engine_ctx, oracle_ctx)
    apply, restore = SETTINGS[setting]
    results = {}
    try:
        apply(case["g"])
        for name in ("he_mul", "he_swk", "he_mul_rs"):
            results[name] = _run(case, name)
    finally:
        restore(case["g"])
    for name, (got, c0, c1) in results.items():
        print("%s, %s: %s" % (setting, name, got))
    for name, (got, c0, c1) in results.items():
        assert c0 == case["want"][name][0] and c1 == case["want"][name][1], (setting, name)
    for name, (got, c0, c1) in results.items():
        assert got == WHOLE[setting][name], (setting, name)


def test_he_swk_in_place_takes_the_weights_off_and_runs_the_front(engine_ctx, oracle_ctx):
    case = _whole(engine_ctx, oracle_ctx)
    got, c0, c1 = _run(case, "he_swk", out0=case["cts"][0].clone())
    print("default, he_swk in place: %s" % got)
    assert c0 == case["want"]["he_swk"][0] and c1 == case["want"]["he_swk"][1]
    assert got == SWK_IN_PLACE
    assert "bridge_relin_tail_direct" not in got and "bridge_tail_stream" not in got
