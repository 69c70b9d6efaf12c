"""The calls that reach the bridge only through launch_decompose / launch_reconstruct and the transforms -- gpq_he_mulpt (+ gpq_he_rs),
gpq_poly_mul, gpq_he_dec, gpq_he_enc_sk / gpq_he_enc_pk on the caller's sampler bytes, gpq_he_genswk, gpq_he_genswk_batch (3 keys),
gpq_gemv_plan_create and gpq_gemv_plan_create_from_matrix (observed through gpq_gemv_plan_info and gpq_gemv_inner) -- under every "bridge" setting
of tests/bridge_settings.py.  Those two read the integer-VALU decompose and the exact CRT, and the limb blocks and the general butterflies
change a transform.  The forced redos and the stream bridge off are a control: only the streaming kernels of gpq_he_mul and of the tail
read them, which none of these calls reaches, so they must make no difference here.

Shapes S1 (logn 13, q = 2^200: two-pass transforms) and S2 (logn 10, q = 2^120: single-pass) of tests/test_settings_derived_gpu.py, batch 3
in launch groups of 2.  Exact throughout:
* under the defaults one ciphertext or key of every call equals what the call's own test compares it with (oracle/bigint_ref,
  tests/enc_model.py, tests/genswk_model.py, the plan of the host-encoded diagonals);
* under every setting every output word equals the default run's, on a context of its own under that setting;
* under "default" and "exact CRT" every C entry point gets a workspace of exactly its *_workspace_bytes between bands of poison
  (bridge_settings.Guarded), outputs framed the same way: no guard word changes, the words are the same."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from gpqhe_amd import ints_to_big, to_device
from oracle import bigint_ref as ref
from tests import bridge_settings as bs
from tests import ecd_model, ecd_record, enc_model
from tests import genswk_model as gm
from tests.gemv_multi_shapes import LOGDELTA, dimpt_of
from tests.test_he_genswk_batch_gpu import _evk_slab

pytestmark = pytest.mark.gpu

SHAPES = {"S1": (13, 200), "S2": (10, 120)}
BATCH, REF = 3, 2                                # the reference's ciphertext / key: the one of the odd last launch group (keys: key 0)
SETTINGS = [s for s in bs.tagged("bridge") if s != "default"]
WS_SETTINGS = ("default", "exact CRT")
SLOTS = 4


class Inputs:
    def __init__(self, shape, engine_ctx, oracle_ctx):
        self.shape = shape
        self.logn, self.logq = logn, logq = SHAPES[shape]
        self.dimP, self.dimA, self.dimB, self.dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
        self.dimpt, self.dimdec, self.dimenc = dimpt_of(logq, logn), (logq + 1) // 59 + 1, enc_model.he_dim(logn, 1 << logq)
        self.nprimes = max(self.dimevk, self.dimpt)
        self.o = o = oracle_ctx(logn, self.nprimes)
        self.n, self.W, self.q = 1 << logn, logq // 64 + 1, 1 << logq
        n, W, q, h = self.n, self.W, self.q, 1 << (logq - 1)
        rng, nrng = random.Random(7 * logq + logn), np.random.default_rng(7 * logq + logn)
        dev = lambda polys, words=W: to_device(np.concatenate([ints_to_big(p, words) for p in polys]))
        small8 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int8).reshape(-1)).cuda()
        centred = lambda: [0, -1, h - 1, -h] + [rng.randrange(-h, h) for _ in range(n - 4)]
        small = lambda bits=LOGDELTA: [rng.randrange(-(1 << bits) + 1, 1 << bits) for _ in range(n)]
        # ciphertexts (he_mulpt, he_dec, one operand of poly_mul), plaintexts, a secret of weight 64 (sample_sk's)
        self.c = [[centred() for _ in range(BATCH)] for _ in range(2)]
        self.pt = [small() for _ in range(BATCH)]
        self.m40 = [small(40) for _ in range(BATCH)]
        self.sk = [0] * n
        for i in rng.sample(range(n), 64):
            self.sk[i] = rng.choice((-1, 1))
        self.pk = (centred(), centred())
        self.d_c, self.d_pt, self.d_m40 = [dev(p) for p in self.c], dev(self.pt), dev(self.m40)
        self.d_sk_big, self.d_pk_big = dev([self.sk]), [dev([p]) for p in self.pk]
        # the encryptors' bytes: he_enc_sk takes error, uniform; he_enc_pk zo, error, error (include/gpqhe_hip.h)
        self.nbits = logq + 1
        nb = self.nbits // 8 + 1
        self.bytes = {k: nrng.integers(0, 256, (BATCH, size), dtype=np.uint8)
                      for k, size in (("sk_e", n), ("sk_a", n * nb), ("pk_v", n // 4), ("pk_e0", n), ("pk_e1", n))}
        self.d_bytes = {k: torch.from_numpy(v.reshape(-1)).cuda() for k, v in self.bytes.items()}
        # three switching keys: raw p1 below 2^bits(P q_L), errors, rotation / conjugation keys of the secret
        self.P = gm.product_of([int(p) for p in o.p[: self.dimP]])
        self.dimmul, self.Wk = gm.dimmul_of(self.P, logq, logn), gm.nbits_of(self.P, logq) // 64 + 1
        assert self.dimmul <= self.dimevk
        self.p1 = [[rng.randrange(1 << gm.nbits_of(self.P, logq)) for _ in range(n)] for _ in range(BATCH)]
        self.e = [[rng.randrange(-11, 12) for _ in range(n)] for _ in range(BATCH)]
        self.galois = [pow(5, 3, 1 << 64), 2 * n - 1, pow(5, n // 2 + 1, 1 << 64)]
        self.d_p1, self.d_e, self.d_sk_small = dev(self.p1, self.Wk), small8(self.e), small8(self.sk)
        self.d_e0_big, self.d_sk_wide = dev([self.e[0]], self.Wk), dev([self.sk], self.Wk)
        self.d_sp0 = dev([gm.galois_image(self.sk, self.galois[0])], self.Wk)
        # a 4 x 4 matrix: its diagonals as 30-bit plaintexts for the plan, the matrix itself for the plan made on the device
        self.diag = [small() for _ in range(SLOTS)]
        self.d_diag = dev(self.diag)
        self.R = [[[centred() for _ in range(BATCH)] for _ in range(2)] for _ in range(2)]            # [c0 | c1][j][k], n1 = 2
        self.d_R = [dev([p for j in range(2) for p in side[j]]) for side in self.R]
        self.A = nrng.uniform(-1, 1, (SLOTS, SLOTS)) + 1j * nrng.uniform(-1, 1, (SLOTS, SLOTS))
        self.d_A = torch.from_numpy(self.A).to("cuda")
        self.roots = ecd_record.stored_roots()
        self.inputs = [self.d_pt, self.d_m40, self.d_sk_big, self.d_p1, self.d_e, self.d_sk_small, self.d_e0_big, self.d_sk_wide, self.d_sp0, self.d_diag,
                       self.d_A] + self.d_c + self.d_pk_big + self.d_R + list(self.d_bytes.values())
        self.pristine = [t.clone() for t in self.inputs]
        self.want = self._reference()

    def inputs_unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.inputs, self.pristine))

    def _reference(self):
        """{call: (polynomial index, device words, ...)} for ciphertext REF / key 0"""
        o, W, q, n, k = self.o, self.W, self.q, self.n, REF
        words = lambda p, w=W: to_device(ints_to_big(p, w))
        rs = lambda poly: [ref.mpi_smod(ref.mpi_rdiv(v, 1 << LOGDELTA), 1 << (self.logq - LOGDELTA)) for v in poly]     # src/he-rescale.c:33-54
        ct = (self.c[0][k], self.c[1][k])
        want = {}
        want["mulpt"] = (k, [words(rs(p)) for p in ref.he_mulpt(o, ct, self.pt[k], self.dimpt, self.logq)])
        want["poly_mul"] = (k, [words(enc_model.poly_mul(o, self.c[0][k], self.pt[k], self.dimpt, q))])
        want["dec"] = (k, [words(enc_model.he_dec(o, ct, self.sk, q))])
        stream = enc_model.Stream(np.concatenate([self.bytes["sk_e"][k], self.bytes["sk_a"][k]]))
        want["enc_sk"] = (k, [words(p) for p in enc_model.he_enc_sk(o, stream, self.m40[k], self.sk, q)])
        stream = enc_model.Stream(np.concatenate([self.bytes["pk_v"][k], self.bytes["pk_e0"][k], self.bytes["pk_e1"][k]]))
        want["enc_pk"] = (k, [words(p) for p in enc_model.he_enc_pk(o, stream, self.m40[k], self.pk, q)])
        primes = [int(p) for p in o.p]
        key = gm.genswk(self.P, self.logq, primes, self.p1[0], self.e[0], gm.galois_image(self.sk, self.galois[0]), self.sk, self.dimmul, self.dimevk)
        want["genswk"] = want["genswk_batch"] = (0, [to_device(_evk_slab(o, p, self.dimevk)) for p in key])
        acc = None                                       # giant step 1 of the 4-slot plan: he_mulpt + he_add, src/he-algo.c:70-78
        for j in range(2):
            prod = ref.he_mulpt(o, (self.R[0][j][k], self.R[1][j][k]), self.diag[2 + j], self.dimpt, self.logq)
            acc = prod if acc is None else ref.he_add(acc, prod, q)
        want["plan inner"] = (k, [words(p) for p in acc])
        return want


_INPUTS, _RUNS = {}, {}
_contexts = bs.Cells()


@pytest.fixture(scope="module", autouse=True)
def _close_cells():
    yield
    torch.cuda.synchronize()
    _RUNS.clear()
    _INPUTS.clear()
    _contexts.close()


def _inputs(shape, engine_ctx, oracle_ctx):
    if shape not in _INPUTS:
        _INPUTS[shape] = Inputs(shape, engine_ctx, oracle_ctx)
    return _INPUTS[shape]


def _plain(words, dtype=torch.int64):
    return torch.full((words,), -1, dtype=dtype, device="cuda")


def _ok(g, rc, what):
    assert rc == 0, "%s refused (%d): %s" % (what, rc, g.lib.gpq_last_error().decode())


def _pack(g, big, W, dim):
    """gpq_evk_pack of ONE polynomial: rns_decompose + forward transform under the context's setting"""
    out = torch.empty(dim * g.n, dtype=torch.int64, device="cuda")
    _ok(g, g.lib.gpq_evk_pack(g.h, g._ptr(out), g._ptr(big), W, dim, 1, g._stream()), "gpq_evk_pack")
    return out


def _inner(g, inp, plan, out, ws):
    per = BATCH * inp.W * inp.n
    o0, o1 = out(per), out(per)
    w = ws(g.lib.gpq_gemv_inner_workspace_bytes(g.h, plan.h, BATCH))
    _ok(g, g.lib.gpq_gemv_inner(g.h, g._ptr(o0), g._ptr(o1), g._ptr(inp.d_R[0]), g._ptr(inp.d_R[1]), plan.h, 1, inp.W, BATCH, g._ptr(w), g._stream()),
        "gpq_gemv_inner")
    return o0, o1


def _info(plan):
    return (plan.dim, plan.bytes, plan.live, plan.exact, plan.diag_bits, tuple(plan.rotations()))


def _all_calls(g, inp, out=_plain, ws=lambda nbytes: _plain(nbytes // 8 + 8)):
    """every call on the context g -> ({name: tensors}, {name: plan info})"""
    lib, n, W, logq, s = g.lib, inp.n, inp.W, inp.logq, g._stream()
    per, res, info = BATCH * W * n, {}, {}
    P = g._ptr
    # he_mulpt, then he_rs in place (src/he-mult.c:159-196, src/he-rescale.c:33-54)
    o0, o1 = out(per), out(per)
    w = ws(lib.gpq_he_mulpt_workspace_bytes(g.h, inp.dimpt, BATCH))
    _ok(g, lib.gpq_he_mulpt(g.h, P(o0), P(o1), P(inp.d_c[0]), P(inp.d_c[1]), P(inp.d_pt), W, logq, inp.dimpt, BATCH, P(w), s), "gpq_he_mulpt")
    _ok(g, lib.gpq_he_rs(g.h, P(o0), P(o1), W, LOGDELTA, logq - LOGDELTA, BATCH, s), "gpq_he_rs")
    res["mulpt"] = (o0, o1)
    # poly_mul (src/poly.c:84-107)
    r = out(per)
    w = ws(lib.gpq_poly_mul_workspace_bytes(g.h, inp.dimpt, BATCH))
    _ok(g, lib.gpq_poly_mul(g.h, P(r), P(inp.d_c[0]), P(inp.d_pt), W, inp.dimpt, logq, BATCH, P(w), s), "gpq_poly_mul")
    res["poly_mul"] = (r,)
    # he_dec (src/he-encrypt.c:105-125)
    m = out(per)
    w = ws(lib.gpq_he_dec_workspace_bytes(g.h, inp.dimdec, BATCH))
    _ok(g, lib.gpq_he_dec(g.h, P(m), P(inp.d_c[0]), P(inp.d_c[1]), P(_pack(g, inp.d_sk_big, W, inp.dimdec)), W, logq, inp.dimdec, BATCH, P(w), s), "gpq_he_dec")
    res["dec"] = (m,)
    # he_enc_sk / he_enc_pk (src/he-encrypt.c:37-103) from the caller's bytes through the device samplers
    e = g.sample_error(_plain(BATCH * n, torch.int8), inp.d_bytes["sk_e"])
    a = g.sample_uniform(_plain(per), inp.d_bytes["sk_a"], inp.nbits, W)
    o0, o1 = out(per), out(per)
    w = ws(lib.gpq_he_enc_workspace_bytes(g.h, inp.dimenc, BATCH, 0))
    _ok(g, lib.gpq_he_enc_sk(g.h, P(o0), P(o1), P(inp.d_m40), P(a), P(e), P(_pack(g, inp.d_sk_big, W, inp.dimenc)), W, logq, inp.dimenc, BATCH, P(w), s),
        "gpq_he_enc_sk")
    res["enc_sk"] = (o0, o1)
    v = g.sample_zo(_plain(BATCH * n, torch.int8), inp.d_bytes["pk_v"])
    e0 = g.sample_error(_plain(BATCH * n, torch.int8), inp.d_bytes["pk_e0"])
    e1 = g.sample_error(_plain(BATCH * n, torch.int8), inp.d_bytes["pk_e1"])
    o0, o1 = out(per), out(per)
    w = ws(lib.gpq_he_enc_workspace_bytes(g.h, inp.dimenc, BATCH, 1))
    pk = [_pack(g, p, W, inp.dimenc) for p in inp.d_pk_big]
    _ok(g, lib.gpq_he_enc_pk(g.h, P(o0), P(o1), P(inp.d_m40), P(v), P(e0), P(e1), P(pk[0]), P(pk[1]), W, logq, inp.dimenc, BATCH, P(w), s), "gpq_he_enc_pk")
    res["enc_pk"] = (o0, o1)
    # he_genswk: key 0 from big slabs; he_genswk_batch: all three (src/he-kem.c:74-118)
    key, Wk = inp.dimevk * n, inp.Wk
    k0, k1 = out(key), out(key)
    nbytes = lib.gpq_he_genswk_workspace_bytes(g.h, Wk, inp.dimP, logq)
    assert nbytes, lib.gpq_last_error()
    w = ws(nbytes)
    _ok(g, lib.gpq_he_genswk(g.h, P(k0), P(k1), P(inp.d_p1[: Wk * n]), P(inp.d_sk_wide), P(inp.d_e0_big), P(inp.d_sp0), Wk, inp.dimP, logq, inp.dimevk, P(w), s),
        "gpq_he_genswk")
    res["genswk"] = (k0, k1)
    k0, k1 = out(BATCH * key), out(BATCH * key)
    nbytes = lib.gpq_he_genswk_batch_workspace_bytes(g.h, Wk, inp.dimP, logq, inp.dimevk, BATCH)
    assert nbytes, lib.gpq_last_error()
    w = ws(nbytes)
    gal = (C.c_uint64 * BATCH)(*inp.galois)
    _ok(g, lib.gpq_he_genswk_batch(g.h, P(k0), P(k1), P(inp.d_p1), P(inp.d_e), P(_pack(g, inp.d_sk_wide, Wk, inp.dimmul)), P(inp.d_sk_small), gal, None, 0, Wk,
                                   inp.dimP, logq, inp.dimevk, BATCH, P(w), s), "gpq_he_genswk_batch")
    res["genswk_batch"] = (k0, k1)
    # plans: made under the setting, observed through their info and one inner sum
    with g.gemv_plan(inp.d_diag, SLOTS, W, logq, inp.dimpt) as plan:
        info["plan"] = _info(plan)
        res["plan inner"] = _inner(g, inp, plan, out, ws)
        torch.cuda.synchronize()
    with g.ecd_plan(SLOTS, inp.roots) as ecd, g.gemv_plan_from_matrix(ecd, inp.d_A, LOGDELTA, logq, inp.dimpt) as plan:
        info["plan from matrix"] = _info(plan)
        res["matrix inner"] = _inner(g, inp, plan, out, ws)
        torch.cuda.synchronize()
    return res, info


def _run(shape, setting, engine_ctx, oracle_ctx):
    if (shape, setting) not in _RUNS:
        inp = _inputs(shape, engine_ctx, oracle_ctx)
        _RUNS[shape, setting] = _all_calls(_contexts.get(inp.logn, inp.nprimes, setting), inp)
    return _RUNS[shape, setting]


def _differences(a, b):
    bad = torch.nonzero(a != b).flatten()
    return "%d words differ, first at %s" % (bad.numel(), bad[:4].tolist()) if bad.numel() else ""


def _assert_same(shape, setting, got, base):
    assert set(got[0]) == set(base[0]) and got[1] == base[1], (got[1], base[1])
    for name, tensors in got[0].items():
        for i, t in enumerate(tensors):
            diff = _differences(t, base[0][name][i])
            assert not diff, "%s, %s under `%s`: output %d against the default run: %s" % (shape, name, setting, i, diff)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_default_run_equals_each_calls_reference(engine_ctx, oracle_ctx, shape):
    inp = _inputs(shape, engine_ctx, oracle_ctx)
    res, info = _run(shape, "default", engine_ctx, oracle_ctx)
    assert inp.inputs_unchanged()
    assert len(res) == 9 and all(bool(t.any()) for ts in res.values() for t in ts)
    for name, (at, want) in inp.want.items():
        for i, words in enumerate(want):
            per = words.numel()
            diff = _differences(res[name][i][at * per:(at + 1) * per], words)
            assert not diff, "%s, %s: output %d of polynomial %d against the reference: %s" % (shape, name, i, at, diff)
    assert torch.equal(res["genswk_batch"][0][: inp.dimevk * inp.n], res["genswk"][0]) and torch.equal(res["genswk_batch"][1][: inp.dimevk * inp.n], res["genswk"][1])
    # the plan made from the matrix on the device is the plan of the diagonals the numpy model encodes on the host (tests/ecd_model.py)
    g = _contexts.get(inp.logn, inp.nprimes, "default")
    coeffs, offending = ecd_model.encode(ecd_model.diagonal_vectors(inp.A), inp.roots, inp.n, LOGDELTA)
    assert offending == 0
    with g.gemv_plan(to_device(ecd_model.words(coeffs, inp.W).reshape(-1)), SLOTS, inp.W, inp.logq, inp.dimpt) as host_plan:
        assert _info(host_plan) == info["plan from matrix"] and host_plan.exact and host_plan.live == SLOTS
        want = _inner(g, inp, host_plan, _plain, lambda nbytes: _plain(nbytes // 8 + 8))
        torch.cuda.synchronize()
        assert torch.equal(want[0], res["matrix inner"][0]) and torch.equal(want[1], res["matrix inner"][1])
    assert info["plan"][2:4] == (SLOTS, True)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bridge_calls_write_the_default_words(engine_ctx, oracle_ctx, shape, setting):
    inp = _inputs(shape, engine_ctx, oracle_ctx)
    got = _run(shape, setting, engine_ctx, oracle_ctx)
    assert inp.inputs_unchanged(), "%s under `%s`: a call wrote to its inputs" % (shape, setting)
    _assert_same(shape, setting, got, _run(shape, "default", engine_ctx, oracle_ctx))


@pytest.mark.parametrize("setting", WS_SETTINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_workspaces_of_exactly_the_reported_size(engine_ctx, oracle_ctx, shape, setting):
    """gpq_he_mulpt_workspace_bytes, gpq_poly_mul_workspace_bytes, gpq_he_dec_workspace_bytes, gpq_he_enc_workspace_bytes (both encryptors),
    gpq_he_genswk_workspace_bytes, gpq_he_genswk_batch_workspace_bytes and gpq_gemv_inner_workspace_bytes, to the byte"""
    inp = _inputs(shape, engine_ctx, oracle_ctx)
    g = _contexts.get(inp.logn, inp.nprimes, setting)
    bufs = {}

    def out(words):
        b = bs.Guarded(8 * words)
        bufs["output %d" % len(bufs)] = b
        return b.t

    def ws(nbytes):
        b = bs.Guarded(nbytes)
        bufs["workspace %d (%d bytes reported)" % (len(bufs), nbytes)] = b
        return b.t

    got = _all_calls(g, inp, out, ws)
    bs.assert_guards(bufs, "%s under `%s`" % (shape, setting))
    assert inp.inputs_unchanged()
    _assert_same(shape, setting, got, _run(shape, "default", engine_ctx, oracle_ctx))
