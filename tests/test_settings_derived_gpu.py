"""The key-switching calls built on gpq_he_swk's pieces -- gpq_he_rot_hoisted, gpq_he_gemv, gpq_he_gemv_planned, gpq_gemv_inner,
gpq_he_gemv_multi -- under every switch of tests/bridge_settings.py.  They choose the key switch's tables and the tail's route themselves
(gpq_he_rot_hoisted: tail_prescale_mode, gpq_keyswitch_rotated, relin_tail with a rotated addend; nrot == 1: gpq_poly_rot + gpq_he_swk) and
carve nested workspaces (gemv_call_layout holds gpq_he_rot_hoisted_workspace_bytes), so a switch could reach them wrongly while
gpq_he_mul / gpq_he_swk, which the other settings tests run, stay right.

Three shapes, each the smallest that reaches a distinct route (dims = he_dims(logq, logq)):
  S1  logn 13, q = 2^200, dims 4/8/12  two-pass ring: the key switch pre-weights limbs; streaming one-product tail by default, the matrix-core
                                       front under prescale <= 2, one matrix product with the stream bridge off
  S2  logn 10, q = 2^120, dims 3/5/8   single-pass ring (gather + gpq_rns_mul key switch); dimP = 3: no matrix-core front, integer-VALU tail
  S3  logn 7,  q = 2^438, dims 8/16/24 single-pass ring, an 8-word P and a 16-word Pi'.  The key switch of a single-pass ring never
                                       pre-weights (can_prescale), so these calls take the matrix-core front here; the one-product tail
                                       over these bases is reached by gpq_relin_tail_overwriting alone (tests/test_tail_routes_gpu.py)
So no cell of S1-S3 runs the one-launch exact finish behind the streaming product (tail_product's fuse_post: bridge_fallback_tail_post<8,16>,
only for an 8-word P and a 16-word Pi'): S1's bases are 8/8 words, and S3 does not stream.  A fourth shape does, for the hoisted call alone:
  S4  logn 13, q = 2^438, dims 8/16/24 two-pass ring with S3's bases: the hoisted call with its rotated addend streams, and under the forced
                                       redos its flagged groups go through that one launch (test_hoisted_call_behind_the_fused_exact_finish)
bridge_fallback_tail_post<16,32> (a 16-word P, q = 2^850) is NOT run behind a derived call by this file: gpq_he_mul / gpq_he_swk's own tests
(tests/test_he_windows_gpu.py) run it through the same relin_tail, and a reference rotation at that size costs seconds.
Batch 3 in launch groups of 2.  Everything is exact: no tolerance anywhere.

1. every call's ciphertexts 0 and 2 equal the restated reference (oracle/bigint_ref), under every setting (computed once per shape);
2. under every setting, every word of every output equals the default run's, and the inputs are unchanged;
3. the setting reached the call: over the tail's classes the hoisted call (4 rotations) launches exactly 4 x what gpq_he_swk launches on the
   same context, and the same classes are non-zero (profiling turns the peer lane off, so "two lanes" asserts gpq_last_lanes instead);
4. through the C entry points with a workspace of exactly *_workspace_bytes between two bands of poison, outputs framed the same way: no
   guard word changes and the outputs are those of 2."""
import ctypes as C
import random
import types

import numpy as np
import pytest
import torch

from gpqhe_amd import gemv_multi_width, gemv_steps, ints_to_big, to_device
from oracle import bigint_ref as ref
from tests import bridge_settings as bs
from tests.gemv_multi_shapes import LOGDELTA, dimpt_of

pytestmark = pytest.mark.gpu

SHAPES = {"S1": (13, 200, (4, 8, 12)), "S2": (10, 120, (3, 5, 8)), "S3": (7, 438, (8, 16, 24))}
BATCH, REF_CTS = 3, (0, 2)
ROTS4, ROTS1 = [0, 3, 3, 40], [5]                 # the identity, a duplicate, a large one; nrot == 1 is gpq_poly_rot + gpq_he_swk
TAIL_CLASSES = ("bridge_tail_stream", "bridge_relin_tail_direct", "bridge_relin_front")
WS_SETTINGS = ("default", "prescale 0", "stream bridge off", "exact CRT", "force redo 1")      # these move the tail onto its exact kernels


class Inputs:
    """one shape's inputs on the host (Python integers) and the device, and the reference's outputs for ciphertexts REF_CTS; made once"""

    def __init__(self, shape, engine_ctx, oracle_ctx):
        self.shape = shape
        self.logn, self.logq, dims = SHAPES[shape]
        logn, logq = self.logn, self.logq
        self.dimP, self.dimA, self.dimB, self.dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
        assert (self.dimP, self.dimA, self.dimB) == dims
        self.dimpt = dimpt_of(logq, logn)
        self.nprimes = max(self.dimevk, self.dimpt)
        self.o = oracle_ctx(logn, self.nprimes)
        self.n, self.W = 1 << logn, logq // 64 + 1
        self.big_slots = 8 if shape != "S3" else 4           # the plan gpq_gemv_inner runs on: n1 != n2 where the shape has it
        n, W, rng, h = self.n, self.W, random.Random(logq * 100 + logn), 1 << (logq - 1)

        def centred():
            return [0, -1, h - 1, -h] + [rng.randrange(-h, h) for _ in range(n - 4)]

        def small(zero=False):
            return [0] * n if zero else [rng.randrange(-(1 << LOGDELTA) + 1, 1 << LOGDELTA) for _ in range(n)]

        self.dev = lambda polys: to_device(np.concatenate([ints_to_big(p, W) for p in polys]))
        self.c = [[centred() for _ in range(BATCH)] for _ in range(2)]
        # a key per rotation, the same for every call: the baby steps of 4 and 8 slots, their giant steps, and the hoisted calls' amounts
        self.hkeys = {r: (self.o.gen(6000 + 2 * r, self.dimevk)[: self.dimB * n], self.o.gen(6001 + 2 * r, self.dimevk)[: self.dimB * n])
                      for r in sorted({0, 1, 2, 3, 4} | set(ROTS4) | set(ROTS1))}
        self.diag4 = [small() for _ in range(4)]
        # 8 slots: n1 = 4, n2 = 2.  Diagonal 2 is zero (baby rotation 2 live nowhere) and so is all of giant step 1
        self.diag8 = [small(zero=k == 2 or k >= 4) for k in range(8)] if shape != "S3" else None
        # gpq_he_gemv_multi, 4 slots (n1 = n2 = 2): the matrix of the planned call, one without baby rotation 1, one without giant step 1
        self.multi = [self.diag4, [small(zero=k in (1, 3)) for k in range(4)], [small(zero=k >= 2) for k in range(4)]]
        n1 = gemv_steps(self.big_slots)[0]
        self.R = [[[centred() for _ in range(BATCH)] for _ in range(n1)] for _ in range(2)]       # gpq_gemv_inner's rotations, [c0 | c1][j][k]
        self.d_c = [self.dev(p) for p in self.c]
        self.d_keys = {r: (to_device(a), to_device(b)) for r, (a, b) in self.hkeys.items()}
        self.d_diag4, self.d_diag8 = self.dev(self.diag4), self.dev(self.diag8) if self.diag8 else None
        self.d_multi = [self.d_diag4] + [self.dev(d) for d in self.multi[1:]]
        self.d_R = [self.dev([p for j in range(n1) for p in side[j]]) for side in self.R]
        self.pristine = [t.clone() for t in self._read_only()]
        self.want = self._reference()

    def big_diag(self):
        return (self.diag8, self.d_diag8) if self.big_slots == 8 else (self.diag4, self.d_diag4)

    def _read_only(self):
        """everything a call reads: the ciphertexts, gpq_gemv_inner's rotations, every matrix's diagonals, both halves of every key"""
        return self.d_c + self.d_R + self.d_multi + ([self.d_diag8] if self.diag8 else []) + [half for r in sorted(self.d_keys) for half in self.d_keys[r]]

    def inputs_unchanged(self):
        now = self._read_only()
        return len(now) == len(self.pristine) and all(torch.equal(a, b) for a, b in zip(now, self.pristine))

    def key_list(self, slots, host=False):
        src = self.hkeys if host else self.d_keys
        return [src.get(r) if r in (0, 1, 2, 3, 4) else None for r in range(slots)]

    def _reference(self):
        """{call: {(poly index within the call's output, ...): (c0 words, c1 words)}} on the device, for ciphertexts REF_CTS"""
        o, W, ql = self.o, self.W, 1 << self.logq
        words = lambda pair: tuple(to_device(ints_to_big(p, W)) for p in pair)
        rotated = {}

        def rot(r, k):
            if (r, k) not in rotated:
                rotated[r, k] = ref.he_swk(o, ref.poly_rot(self.c[0][k], r), ref.poly_rot(self.c[1][k], r), *self.hkeys[r], self.dimP, self.dimB, self.logq)
            return rotated[r, k]

        def gemv(diags, slots, k):
            return ref.ref_gemv(o, (self.c[0][k], self.c[1][k]), diags, self.key_list(slots, host=True), slots, self.dimP, self.dimB, self.dimpt,
                                self.logq, LOGDELTA)

        want = {"rot4": {}, "rot1": {}, "gemv4": {}, "gemv8": {}, "inner0": {}, "inner1": {}, "multi0": {}, "multi1": {}, "multi2": {}}
        for k in REF_CTS:
            for r, amount in enumerate(ROTS4):
                want["rot4"][r * BATCH + k] = words(rot(amount, k))
            want["rot1"][k] = words(rot(ROTS1[0], k))
            want["gemv4"][k] = want["multi0"][k] = words(gemv(self.diag4, 4, k))
            if self.shape != "S3":
                want["gemv8"][k] = words(gemv(self.diag8, 8, k))
            for t in (1, 2):
                want["multi%d" % t][k] = words(gemv(self.multi[t], 4, k))
            diags, n1 = self.big_diag()[0], gemv_steps(self.big_slots)[0]
            for giant in (0, 1):                              # smod(sum_j R_j * diag[giant n1 + j], q): he_mulpt + he_add of src/he-algo.c:70-78
                acc = None
                for j in range(n1):
                    prod = ref.he_mulpt(o, (self.R[0][j][k], self.R[1][j][k]), diags[giant * n1 + j], self.dimpt, self.logq)
                    acc = prod if acc is None else ref.he_add(acc, prod, ql)
                want["inner%d" % giant][k] = words(acc)
        return want


_INPUTS, _CELLS, _RUNS = {}, {}, {}
_contexts = bs.Cells()


@pytest.fixture(scope="module", autouse=True)
def _close_cells():
    yield
    torch.cuda.synchronize()
    for cell in _CELLS.values():
        cell.close()
    _contexts.close()
    for d in (_INPUTS, _CELLS, _RUNS):
        d.clear()


def _inputs(shape, engine_ctx, oracle_ctx):
    if shape not in _INPUTS:
        _INPUTS[shape] = Inputs(shape, engine_ctx, oracle_ctx)
    return _INPUTS[shape]


class Cell:
    """one (shape, setting): a context of its own under the setting and the plans created on it, i.e. under the setting"""

    def __init__(self, inp, setting):
        self.inp, self.setting = inp, setting
        self.g = g = _contexts.get(inp.logn, inp.nprimes, setting)
        self.plan4 = g.gemv_plan(inp.d_diag4, 4, inp.W, inp.logq, inp.dimpt)
        self.plan8 = g.gemv_plan(inp.d_diag8, 8, inp.W, inp.logq, inp.dimpt) if inp.shape != "S3" else None
        self.others = [g.gemv_plan(d, 4, inp.W, inp.logq, inp.dimpt) for d in inp.d_multi[1:]]
        self.set = g.gemv_multi([self.plan4] + self.others)
        assert self.plan4.exact and self.plan4.live == 4 and [p.live for p in self.others] == [2, 2] and self.set.count == 3 > gemv_multi_width()
        assert self.others[0].rotations() == [1, 0, 1, 0] and self.others[1].rotations() == [1, 1, 0, 0]      # different live sets
        if self.plan8 is not None:
            assert self.plan8.exact and self.plan8.live == 3 and self.plan8.rotations() == [1, 1, 0, 1, 0, 0, 0, 0]

    def big_plan(self):
        return self.plan8 if self.plan8 is not None else self.plan4

    def close(self):
        self.set.close()
        for p in [self.plan4, self.plan8] + self.others:
            if p is not None:
                p.close()


def _cell(shape, setting, engine_ctx, oracle_ctx):
    if (shape, setting) not in _CELLS:
        _CELLS[shape, setting] = Cell(_inputs(shape, engine_ctx, oracle_ctx), setting)
    return _CELLS[shape, setting]


def _plain(words):
    return torch.full((words,), -1, dtype=torch.int64, device="cuda")


def _ok(g, rc, what):
    # a refusal would have to be gpq_he_swk's own on the same context; on these shapes gpq_he_swk runs under every setting, so none is expected
    assert rc == 0, "%s refused (%d): %s" % (what, rc, g.lib.gpq_last_error().decode())


def _swk(cell, out, ws):
    """gpq_he_swk of the batch with rotation 0's key, through the C entry point"""
    g, inp = cell.g, cell.inp
    lib, per, k = g.lib, BATCH * inp.W * inp.n, inp.d_keys[0]
    o0, o1 = out(per), out(per)
    w = ws(lib.gpq_he_swk_workspace_bytes(g.h, inp.W, inp.dimB, inp.dimP, BATCH))
    _ok(g, lib.gpq_he_swk(g.h, g._ptr(o0), g._ptr(o1), g._ptr(inp.d_c[0]), g._ptr(inp.d_c[1]), g._ptr(k[0]), g._ptr(k[1]), inp.W, inp.logq, inp.dimB, inp.dimP,
                          BATCH, g._ptr(w), g._stream()), "gpq_he_swk")
    return {"swk": (o0, o1)}


def _rot(cell, out, ws, rots, name):
    g, inp = cell.g, cell.inp
    lib, per, nrot = g.lib, BATCH * inp.W * inp.n, len(rots)
    o0, o1 = out(nrot * per), out(nrot * per)
    nbytes = lib.gpq_he_rot_hoisted_workspace_bytes(g.h, inp.W, inp.dimB, inp.dimP, nrot, BATCH)
    assert nbytes, lib.gpq_last_error()
    w = ws(nbytes)
    r = (C.c_uint * nrot)(*rots)
    _ok(g, lib.gpq_he_rot_hoisted(g.h, g._ptr(o0), g._ptr(o1), g._ptr(inp.d_c[0]), g._ptr(inp.d_c[1]), r, g._key_ptrs([inp.d_keys[x][0] for x in rots]),
                                  g._key_ptrs([inp.d_keys[x][1] for x in rots]), nrot, inp.W, inp.logq, inp.dimB, inp.dimP, BATCH, g._ptr(w), g._stream()),
        "gpq_he_rot_hoisted (%s)" % name)
    return {name: (o0, o1)}


def _gemv(cell, out, ws, slots):
    g, inp = cell.g, cell.inp
    lib, per, keys = g.lib, BATCH * inp.W * inp.n, inp.key_list(slots)
    k0, k1 = [k and k[0] for k in keys], [k and k[1] for k in keys]
    diag, plan = (inp.d_diag4, cell.plan4) if slots == 4 else (inp.d_diag8, cell.plan8)
    res = {}
    o0, o1 = out(per), out(per)
    nbytes = lib.gpq_he_gemv_workspace_bytes(g.h, inp.W, slots, inp.dimB, inp.dimP, inp.dimpt, BATCH)
    assert nbytes, lib.gpq_last_error()
    w = ws(nbytes)
    _ok(g, lib.gpq_he_gemv(g.h, g._ptr(o0), g._ptr(o1), g._ptr(inp.d_c[0]), g._ptr(inp.d_c[1]), g._ptr(diag), g._key_ptrs(k0), g._key_ptrs(k1), slots, inp.W,
                           inp.logq, LOGDELTA, inp.dimB, inp.dimP, inp.dimpt, BATCH, g._ptr(w), g._stream()), "gpq_he_gemv (%d slots)" % slots)
    res["gemv%d" % slots] = (o0, o1)
    res.update(_planned(cell, out, ws, plan, "planned%d" % slots))
    return res


def _planned(cell, out, ws, plan, name):
    g, inp = cell.g, cell.inp
    lib, per, keys = g.lib, BATCH * inp.W * inp.n, inp.key_list(plan.slots)
    k0, k1 = [k and k[0] for k in keys], [k and k[1] for k in keys]
    o0, o1 = out(per), out(per)
    nbytes = lib.gpq_he_gemv_planned_workspace_bytes(g.h, plan.h, inp.W, inp.dimB, inp.dimP, BATCH)
    assert nbytes, lib.gpq_last_error()
    w = ws(nbytes)
    _ok(g, lib.gpq_he_gemv_planned(g.h, g._ptr(o0), g._ptr(o1), g._ptr(inp.d_c[0]), g._ptr(inp.d_c[1]), plan.h, g._key_ptrs(k0), g._key_ptrs(k1), inp.W,
                                   LOGDELTA, inp.dimB, inp.dimP, BATCH, g._ptr(w), g._stream()), "gpq_he_gemv_planned (%s)" % name)
    return {name: (o0, o1)}


def _inner(cell, out, ws):
    g, inp, plan = cell.g, cell.inp, cell.big_plan()
    lib, per, res = g.lib, BATCH * inp.W * inp.n, {}
    for giant in (0, 1):                                  # with 8 slots giant step 1 is all zero: the call writes an exact zero
        o0, o1 = out(per), out(per)
        nbytes = lib.gpq_gemv_inner_workspace_bytes(g.h, plan.h, BATCH)
        assert nbytes
        w = ws(nbytes)
        _ok(g, lib.gpq_gemv_inner(g.h, g._ptr(o0), g._ptr(o1), g._ptr(inp.d_R[0]), g._ptr(inp.d_R[1]), plan.h, giant, inp.W, BATCH, g._ptr(w), g._stream()),
            "gpq_gemv_inner (giant step %d)" % giant)
        res["inner%d" % giant] = (o0, o1)
    return res


def _multi(cell, out, ws):
    g, inp = cell.g, cell.inp
    lib, per, keys = g.lib, BATCH * inp.W * inp.n, inp.key_list(4)
    k0, k1 = [k and k[0] for k in keys], [k and k[1] for k in keys]
    outs0, outs1 = [out(per) for _ in range(3)], [out(per) for _ in range(3)]
    nbytes = lib.gpq_he_gemv_multi_workspace_bytes(g.h, cell.set.h, inp.W, inp.dimB, inp.dimP, BATCH)
    assert nbytes, lib.gpq_last_error()
    w = ws(nbytes)
    _ok(g, lib.gpq_he_gemv_multi(g.h, g._key_ptrs(outs0), g._key_ptrs(outs1), g._ptr(inp.d_c[0]), g._ptr(inp.d_c[1]), cell.set.h, g._key_ptrs(k0),
                                 g._key_ptrs(k1), inp.W, LOGDELTA, inp.dimB, inp.dimP, BATCH, g._ptr(w), g._stream()), "gpq_he_gemv_multi")
    return {"multi%d" % t: (outs0[t], outs1[t]) for t in range(3)}


def _all_calls(cell, out=_plain, ws=lambda nbytes: _plain(nbytes // 8 + 8)):
    """every call of the cell -> {name: (c0, c1)}"""
    res = {}
    res.update(_swk(cell, out, ws))
    res.update(_rot(cell, out, ws, ROTS4, "rot4"))
    res.update(_rot(cell, out, ws, ROTS1, "rot1"))
    res.update(_gemv(cell, out, ws, 4))
    if cell.plan8 is not None:
        res.update(_gemv(cell, out, ws, 8))
    res.update(_inner(cell, out, ws))
    res.update(_multi(cell, out, ws))
    torch.cuda.synchronize()
    return res


def _run(shape, setting, engine_ctx, oracle_ctx):
    if (shape, setting) not in _RUNS:
        _RUNS[shape, setting] = _all_calls(_cell(shape, setting, engine_ctx, oracle_ctx))
    return _RUNS[shape, setting]


def _differences(a, b):
    bad = torch.nonzero(a != b).flatten()
    return "%d words differ, first at %s" % (bad.numel(), bad[:4].tolist()) if bad.numel() else ""


def _assert_reference(inp, res, setting):
    per = inp.W * inp.n
    for name, pair in res.items():
        want = inp.want.get("gemv" + name[7:] if name.startswith("planned") else name)
        if name == "swk":
            want = {k: inp.want["rot4"][k] for k in REF_CTS}           # rotation 0 with its key: he_swk of the inputs as they are
        assert want, name
        for at, words in want.items():
            for side in (0, 1):
                diff = _differences(pair[side][at * per:(at + 1) * per], words[side])
                assert not diff, "%s, %s under `%s`: c%d of polynomial %d against the reference: %s" % (inp.shape, name, setting, side, at, diff)


def _assert_same(inp, res, base, setting, what="the default run"):
    assert set(res) == set(base)
    for name in res:
        for side in (0, 1):
            diff = _differences(res[name][side], base[name][side])
            assert not diff, "%s, %s under `%s`: c%d against %s: %s" % (inp.shape, name, setting, side, what, diff)


@pytest.mark.parametrize("setting", list(bs.SETTINGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_derived_calls_write_the_reference_and_the_default_words(engine_ctx, oracle_ctx, shape, setting):
    inp = _inputs(shape, engine_ctx, oracle_ctx)
    res = _run(shape, setting, engine_ctx, oracle_ctx)
    assert inp.inputs_unchanged(), "%s under `%s`: a call wrote to its inputs" % (shape, setting)
    assert len(res) == (12 if shape != "S3" else 10)
    for name, pair in res.items():
        assert name in ("inner1",) and shape != "S3" or bool(pair[0].any()) and bool(pair[1].any()), name      # (the zero giant step is zero)
    _assert_reference(inp, res, setting)
    if setting != "default":
        _assert_same(inp, res, _run(shape, "default", engine_ctx, oracle_ctx), setting)
    if shape != "S3":
        assert not res["inner1"][0].any() and not res["inner1"][1].any()


def _tail_counts(g, call, classes=TAIL_CLASSES):
    torch.cuda.synchronize()
    g.profile(True)
    try:
        g.profile_collect()
        call()
        torch.cuda.synchronize()
        prof = g.profile_collect()
    finally:
        g.profile(False)
    return {k: int(prof[k][1]) if k in prof else 0 for k in classes}


@pytest.mark.parametrize("setting", list(bs.SETTINGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_setting_reaches_the_hoisted_call(engine_ctx, oracle_ctx, shape, setting):
    """gpq_he_swk under the same setting on the same context is the yardstick, not a table: per launch group it runs one tail, the hoisted call
    one per rotation, through the same relin_tail with the mode tail_prescale_mode gave both -- so every class counts exactly 4 x."""
    cell = _cell(shape, setting, engine_ctx, oracle_ctx)
    ws = lambda nbytes: _plain(nbytes // 8 + 8)
    if setting == "two lanes":
        # profiling keeps a call on one lane, so there is nothing to count here: the setting is shown to be on by the lanes gpq_he_swk took
        # (two launch groups: tests/test_overlap_gpu.py expects 2), and the derived calls ran on this context in the test above
        _swk(cell, _plain, ws)
        torch.cuda.synchronize()
        assert cell.g.last_lanes() == 2
        return
    swk = _tail_counts(cell.g, lambda: _swk(cell, _plain, ws))
    hoisted = _tail_counts(cell.g, lambda: _rot(cell, _plain, ws, ROTS4, "rot4"))
    print("%s, %s: he_swk %s, hoisted %s" % (shape, setting, swk, hoisted))
    assert hoisted == {k: len(ROTS4) * v for k, v in swk.items()}, (swk, hoisted)
    assert {k for k, v in hoisted.items() if v} == {k for k, v in swk.items() if v}
    # not vacuous: with 4 or more limbs of P and the matrix-core kernels on, the tail is one of the three classes; S2 (dimP = 3) and the
    # integer-VALU settings take the integer-VALU tail, which has none of them
    matrix_cores = "integer-VALU" not in setting
    assert any(swk.values()) == (shape != "S2" and matrix_cores), swk
    if shape == "S1" and matrix_cores:
        on = {k for k, v in swk.items() if v}
        if "prescale" in setting or "exact CRT" in setting:
            assert on == {"bridge_relin_front"}, on
        else:
            assert on == ({"bridge_relin_tail_direct"} if "stream bridge off" in setting else {"bridge_tail_stream"}), on


@pytest.mark.parametrize("shape", list(SHAPES))
def test_plans_cross_settings(engine_ctx, oracle_ctx, shape):
    """a plan holds transformed diagonals: one built under one setting and used under another gives the same words"""
    inp = _inputs(shape, engine_ctx, oracle_ctx)
    base = _run(shape, "default", engine_ctx, oracle_ctx)
    for build, use, what in ((lambda g: None, lambda g: g.set_prescale(0), "built under the defaults, used under prescale 0"),
                             (lambda g: g.set_bridge_mfma(False), lambda g: g.set_bridge_mfma(True), "built under integer-VALU decompose, used under the defaults")):
        with bs.setting_context(inp.logn, inp.nprimes) as g:
            build(g)
            cell = types.SimpleNamespace(g=g, inp=inp)
            plan = g.gemv_plan(inp.d_diag4, 4, inp.W, inp.logq, inp.dimpt)
            try:
                torch.cuda.synchronize()
                use(g)
                res = _planned(cell, _plain, lambda nbytes: _plain(nbytes // 8 + 8), plan, "planned4")
                torch.cuda.synchronize()
                _assert_same(inp, res, {"planned4": base["planned4"]}, what)
            finally:
                plan.close()


@pytest.mark.parametrize("setting", WS_SETTINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_workspaces_of_exactly_the_reported_size(engine_ctx, oracle_ctx, shape, setting):
    """The wrappers of gpqhe_amd/engine.py add 8 words to every workspace; here each C entry point gets exactly what its *_workspace_bytes
    reports under the setting, as a 64-byte aligned slice between two 64 KiB bands of poison inside one allocation, and writes its outputs
    into slices framed the same way.  Only allocated memory is read."""
    inp = _inputs(shape, engine_ctx, oracle_ctx)
    cell = _cell(shape, setting, engine_ctx, oracle_ctx)
    bufs = {}

    def out(words):
        b = bs.Guarded(8 * words)
        bufs["output %d" % len(bufs)] = b
        return b.t

    def ws(nbytes):
        b = bs.Guarded(nbytes)
        bufs["workspace %d (%d bytes reported)" % (len(bufs), nbytes)] = b
        return b.t

    res = _all_calls(cell, out, ws)
    bs.assert_guards(bufs, "%s under `%s`" % (shape, setting))
    assert inp.inputs_unchanged()
    _assert_same(inp, res, _run(shape, "default", engine_ctx, oracle_ctx), setting)


# ---------------------------------------------------------------------------
# S4: the hoisted call behind the one-launch exact finish of the streaming tail
# ---------------------------------------------------------------------------
S4 = (13, 438, (8, 16, 24))
S4_SETTINGS = ("default", "force redo 1", "force redo 7", "stream bridge off")      # the last: same bases, the finish as separate launches


class HoistedInputs:
    """S4's ciphertexts and rotation keys, and the reference's rotations of ciphertext 0 (under a second each: three of them, once)"""

    def __init__(self, engine_ctx, oracle_ctx):
        self.shape, (self.logn, self.logq, dims) = "S4", S4
        logn, logq = self.logn, self.logq
        self.dimP, self.dimA, self.dimB, self.dimevk = engine_ctx(logn, 12).he_dims(logq, logq)
        assert (self.dimP, self.dimA, self.dimB) == dims
        self.nprimes = self.dimevk
        self.o = o = oracle_ctx(logn, self.nprimes)
        self.n, self.W = 1 << logn, logq // 64 + 1
        n, W, rng, h = self.n, self.W, random.Random(logq * 100 + logn), 1 << (logq - 1)
        self.c = [[[0, -1, h - 1, -h] + [rng.randrange(-h, h) for _ in range(n - 4)] for _ in range(BATCH)] for _ in range(2)]
        self.hkeys = {r: (o.gen(6000 + 2 * r, self.dimevk)[: self.dimB * n], o.gen(6001 + 2 * r, self.dimevk)[: self.dimB * n]) for r in sorted(set(ROTS4))}
        self.d_c = [to_device(np.concatenate([ints_to_big(p, W) for p in side])) for side in self.c]
        self.d_keys = {r: (to_device(a), to_device(b)) for r, (a, b) in self.hkeys.items()}
        self.pristine = [t.clone() for t in self._read_only()]
        rotated = {r: ref.he_swk(o, ref.poly_rot(self.c[0][0], r), ref.poly_rot(self.c[1][0], r), *self.hkeys[r], self.dimP, self.dimB, logq) for r in self.hkeys}
        self.want = {"rot4": {i * BATCH: tuple(to_device(ints_to_big(p, W)) for p in rotated[r]) for i, r in enumerate(ROTS4)}}

    def _read_only(self):
        return self.d_c + [half for r in sorted(self.d_keys) for half in self.d_keys[r]]

    def inputs_unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self._read_only(), self.pristine))


def _s4_run(setting, engine_ctx, oracle_ctx):
    """gpq_he_swk and the hoisted call at S4 under `setting`, every buffer guarded and of the reported size; checked once, then cached"""
    if "S4" not in _INPUTS:
        _INPUTS["S4"] = HoistedInputs(engine_ctx, oracle_ctx)
    inp = _INPUTS["S4"]
    cell = types.SimpleNamespace(g=_contexts.get(inp.logn, inp.nprimes, setting), inp=inp)
    if ("S4", setting) not in _RUNS:
        bufs = {}

        def out(words):
            b = bs.Guarded(8 * words)
            bufs["output %d" % len(bufs)] = b
            return b.t

        def ws(nbytes):
            b = bs.Guarded(nbytes)
            bufs["workspace %d (%d bytes reported)" % (len(bufs), nbytes)] = b
            return b.t

        res = _swk(cell, out, ws)
        res.update(_rot(cell, out, ws, ROTS4, "rot4"))
        torch.cuda.synchronize()
        bs.assert_guards(bufs, "S4 under `%s`" % setting)
        assert inp.inputs_unchanged(), "S4 under `%s`: a call wrote to its inputs" % setting
        _RUNS["S4", setting] = res
    return inp, cell, _RUNS["S4", setting]


@pytest.mark.parametrize("setting", S4_SETTINGS)
def test_hoisted_call_behind_the_fused_exact_finish(engine_ctx, oracle_ctx, setting):
    """tail_product finishes the groups its streaming kernel flagged in ONE launch (bridge_fallback_tail_post<8,16>) when P has 8 words and Pi'
    16.  S1's bases are 8/8 words and S3 does not stream, so this shape runs gpq_he_rot_hoisted (4 rotations, rotated addend) and gpq_he_swk
    there: by default on what the kernel flags itself, under force redo 1 on every coefficient, under force redo 7 on every seventh besides, and
    with the stream bridge off through the separate launches of the same finish.  Workspaces of exactly the reported size between poison,
    ciphertext 0 against the reference, every word against the default run, and the tail's classes 4 x gpq_he_swk's, the streaming kernel
    being the one that runs."""
    assert setting in bs.SETTINGS
    inp, cell, res = _s4_run(setting, engine_ctx, oracle_ctx)
    _assert_reference(inp, {"rot4": res["rot4"]}, setting)
    per = inp.W * inp.n
    for side in (0, 1):                      # rotation 0 with its key is gpq_he_swk of the inputs as they are
        assert torch.equal(res["swk"][side], res["rot4"][side][:BATCH * per])
    if setting != "default":
        _assert_same(inp, res, _s4_run("default", engine_ctx, oracle_ctx)[2], setting)
    plain = lambda nbytes: _plain(nbytes // 8 + 8)
    classes = TAIL_CLASSES + ("bridge_exact_paths",)
    swk = _tail_counts(cell.g, lambda: _swk(cell, _plain, plain), classes)
    hoisted = _tail_counts(cell.g, lambda: _rot(cell, _plain, plain, ROTS4, "rot4"), classes)
    print("S4, %s: he_swk %s, hoisted %s" % (setting, swk, hoisted))
    assert hoisted == {k: len(ROTS4) * v for k, v in swk.items()}, (swk, hoisted)
    if setting == "stream bridge off":
        assert swk["bridge_relin_tail_direct"] == 2 and not swk["bridge_tail_stream"] and not swk["bridge_relin_front"], swk
    else:
        # per launch group one streaming product and, behind it, three masked launches: bridge_limb_scale, the front re-run and the ONE
        # launch of the finish (tests/test_tail_routes_gpu.py, route "product"); the finish as separate launches would count more
        assert swk == {"bridge_tail_stream": 2, "bridge_relin_tail_direct": 0, "bridge_relin_front": 0, "bridge_exact_paths": 6}, swk
