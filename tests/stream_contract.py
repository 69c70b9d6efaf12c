"""The stream contract of include/gpqhe_hip.h, once: every exported function with a `void *stream` parameter in exactly one class, and for
every function that launches one closure `call(g, ins, outs, ws)` that issues exactly that C entry point on g._stream().  A plain module:
nothing here is collected.  tests/test_stream_contract_cover.py (no device) pins the table against the header;
tests/test_stream_contract_gpu.py runs every closure behind a delayed producer on a non-blocking side stream and inside a replayed graph.

CAPTURABLE          after one warm call of the same shape on the same context the call makes no host synchronisation, no allocation and no
                    host read-back: it can be captured and replayed
ORDERED             all device work is ordered on `stream`, but the call may synchronise the host or allocate (launch_smod_general waits for
                    its constants' copy, the plan constructors read their measurement back): eager use on any stream, never inside a capture
REFUSES_IN_CAPTURE  returns GPQ_ERR_INVALID when `stream` is capturing, before anything is allocated; queues nothing on the stream otherwise
NOT_A_LAUNCH        takes a stream but launches no kernel of the library's own (a reason each)

Inputs.  The shapes are those of tests/test_settings_bridge_calls_gpu.py and tests/test_settings_derived_gpu.py (S1: two-pass ring, strided +
contiguous + mid8 launches and the inverse-table override; S2: the one-pass small_ntt path), batch 3 in launch groups of 2, and the argument
lists are the ones their `_all_calls` batteries pass.  The words themselves are made here with numpy, not taken from those modules' Inputs:
a closure needs TWO valid input sets, A and B, from one generator under two seeds, and no reference (those classes draw one fixed set and
compute a Python-integer reference for it, which this contract has no use for: the words are pinned there).  Valid means that a misordered call
gives wrong words, never a bad address: canonical residues, coefficients centred mod q, bytes for the samplers, int8 small slabs in range.
What a call only reads and no producer would rewrite between calls -- keys, plans, Galois elements -- is made once per shape (Env)."""
import ctypes as C
import zlib

import numpy as np

from tests import bridge_settings as bs
from tests.gemv_multi_shapes import LOGDELTA, dimpt_of

CAPTURABLE, ORDERED, REFUSES_IN_CAPTURE, NOT_A_LAUNCH = "CAPTURABLE", "ORDERED", "REFUSES_IN_CAPTURE", "NOT_A_LAUNCH"

# name -> class, in the header's order
TABLE = {
    "gpq_upload": NOT_A_LAUNCH, "gpq_download": NOT_A_LAUNCH, "gpq_copy": NOT_A_LAUNCH, "gpq_stream_sync": NOT_A_LAUNCH,
    "gpq_stream_wait": NOT_A_LAUNCH, "gpq_probe_stream": NOT_A_LAUNCH, "gpq_stream_destroy": NOT_A_LAUNCH,
    "gpq_ntt": CAPTURABLE, "gpq_invntt": CAPTURABLE, "gpq_ntt_reference": CAPTURABLE,
    "gpq_rns_mul": CAPTURABLE, "gpq_rns_add": CAPTURABLE, "gpq_poly_mul_rns": CAPTURABLE, "gpq_mulpt_rns": CAPTURABLE,
    "gpq_he_mul_tensor": CAPTURABLE, "gpq_keyswitch": CAPTURABLE,
    "gpq_rns_decompose": CAPTURABLE, "gpq_rns_decompose_limbs": CAPTURABLE, "gpq_rns_reconstruct": CAPTURABLE, "gpq_poly_mul": CAPTURABLE,
    "gpq_rns_reconstruct_general": ORDERED, "gpq_poly_mul_general": ORDERED,
    "gpq_he_rs": CAPTURABLE, "gpq_he_rescale": CAPTURABLE, "gpq_he_mul": CAPTURABLE, "gpq_he_mul_rs": CAPTURABLE,
    "gpq_relin_tail": CAPTURABLE, "gpq_big_transpose": CAPTURABLE, "gpq_big_addsub": CAPTURABLE, "gpq_relin_tail_overwriting": CAPTURABLE,
    "gpq_he_swk": CAPTURABLE, "gpq_he_mulpt": CAPTURABLE, "gpq_poly_rot": CAPTURABLE, "gpq_poly_conj": CAPTURABLE,
    "gpq_he_mulpt_const": CAPTURABLE, "gpq_he_addpt_const": CAPTURABLE,
    "gpq_he_rot_hoisted": CAPTURABLE, "gpq_he_gemv": CAPTURABLE,
    "gpq_gemv_plan_create": ORDERED, "gpq_gemv_inner": CAPTURABLE, "gpq_he_gemv_planned": CAPTURABLE,
    "gpq_gemv_multi_create": REFUSES_IN_CAPTURE, "gpq_he_gemv_multi": CAPTURABLE,
    "gpq_he_ecd": CAPTURABLE, "gpq_he_ecd_diagonals": CAPTURABLE, "gpq_gemv_plan_create_from_matrix": ORDERED,
    "gpq_he_dcd": CAPTURABLE, "gpq_he_dec": CAPTURABLE,
    "gpq_sample_zo": CAPTURABLE, "gpq_sample_error": CAPTURABLE, "gpq_sample_uniform": CAPTURABLE, "gpq_small_to_big": CAPTURABLE,
    "gpq_he_enc_pk": CAPTURABLE, "gpq_he_enc_sk": CAPTURABLE,
    "gpq_surf_bytes": CAPTURABLE, "gpq_rng_device_bytes": CAPTURABLE,
    "gpq_he_rs_general": ORDERED, "gpq_relin_tail_general": ORDERED, "gpq_he_mul_general": ORDERED, "gpq_he_mulpt_general": ORDERED,
    "gpq_he_swk_general": ORDERED,
    "gpq_big_add": CAPTURABLE, "gpq_big_sub": CAPTURABLE, "gpq_big_neg": CAPTURABLE, "gpq_evk_pack": CAPTURABLE,
    "gpq_he_genswk": ORDERED, "gpq_he_genswk_batch": CAPTURABLE,
    "gpq_timer_start": NOT_A_LAUNCH, "gpq_timer_stop": NOT_A_LAUNCH,
}

NOT_A_LAUNCH_REASON = {
    "gpq_upload": "a plain hipMemcpyAsync on the stream",
    "gpq_download": "a plain hipMemcpyAsync on the stream",
    "gpq_copy": "a plain hipMemcpyAsync on the stream",
    "gpq_stream_sync": "hipStreamSynchronize: the host waits, nothing is queued",
    "gpq_stream_wait": "an event recorded on one stream and awaited by the other (tests/test_stream_wait_gpu.py); its parameters are `waiter` and `on`",
    "gpq_probe_stream": "bench.py's copy-rate yardstick: one plain copy kernel on the stream, no context and no scratch",
    "gpq_stream_destroy": "hipStreamDestroy of a stream of gpq_stream_create",
    "gpq_timer_start": "hipEventRecord on the stream",
    "gpq_timer_stop": "hipEventRecord on the stream",
}
# in the table although no parameter of theirs is spelled `void *stream`
NAMED_OTHERWISE = ("gpq_stream_wait",)

# the bytes the generators repeat when a captured graph is replayed (seed and position are launch arguments, include/gpqhe_hip.h)
REPEATS_ON_REPLAY = ("gpq_surf_bytes", "gpq_rng_device_bytes")


def names_of(cls):
    return [name for name, c in TABLE.items() if c == cls]


SHAPES = {"S1": (13, 200), "S2": (10, 120)}          # tests/test_settings_bridge_calls_gpu.py, tests/test_settings_derived_gpu.py
ECD_SHAPE = ("E", 9, 16)                             # gpq_he_ecd / gpq_he_dcd: 16 slots at logn 9, one block (tests/test_he_ecd_gpu.py)
RING, ECD = ("S1", "S2"), ("E",)
BATCH, SLOTS, ROTS4 = 3, 4, [0, 3, 3, 40]
POISON_BYTE = 0xC3
SURF_LEN = 4096


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ok(g, rc, what):
    assert rc == 0, "%s refused (%d): %s" % (what, rc, g.lib.gpq_last_error().decode())


def _words(q):
    L = (q.bit_length() + 63) // 64
    return (C.c_uint64 * L)(*[(q >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(L)]), L


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.reshape(-1)).cuda()


class Args(dict):
    """the tensors of one input or output set by name, and the shape's fixed material as `.env`"""

    def __init__(self, env, items=()):
        super().__init__(items)
        self.env = env


# ---------------------------------------------------------------------------
# generators: numpy words of one kind under one numpy Generator
# ---------------------------------------------------------------------------
def residues(e, rng, dim, polys):
    """canonical residues [polys][dim][n] of limbs 0 .. dim-1"""
    a = np.empty((polys, dim, e.n), dtype=np.uint64)
    for d in range(dim):
        a[:, d] = rng.integers(0, e.g.p[d], size=(polys, e.n), dtype=np.uint64)
    return a


def centred(e, rng, polys, logq=None, W=None):
    """big slabs [polys][W][n] of coefficients centred mod 2^logq (tests/gemv_multi_shapes.py: MultiShape.ciphertexts)"""
    logq, W = logq or e.logq, W or e.W
    top = logq - 1 - 64 * (W - 1)
    a = np.empty((polys, W, e.n), dtype=np.uint64)
    a[:, : W - 1] = rng.integers(0, 0xFFFFFFFFFFFFFFFF, size=(polys, W - 1, e.n), dtype=np.uint64, endpoint=True)
    a[:, W - 1] = rng.integers(-(1 << top), 1 << top, size=(polys, e.n), dtype=np.int64).view(np.uint64)
    return a


def small(e, rng, polys, bits=LOGDELTA, W=None, lo=None, hi=None):
    """big slabs of coefficients in (-2^bits, 2^bits) (or [lo, hi)), sign-extended over W words"""
    W = W or e.W
    v = rng.integers(-(1 << bits) + 1 if lo is None else lo, 1 << bits if hi is None else hi, size=(polys, e.n), dtype=np.int64)
    a = np.empty((polys, W, e.n), dtype=np.int64)
    a[:, 0] = v
    a[:, 1:] = (v >> 63)[:, None, :]
    return a.view(np.uint64)


def raw(e, rng, polys, nbits, W):
    """big slabs of values in [0, 2^nbits): gpq_sample_uniform's output, not reduced and not centred"""
    a = rng.integers(0, 0xFFFFFFFFFFFFFFFF, size=(polys, W, e.n), dtype=np.uint64, endpoint=True)
    for j in range(W):
        keep = min(max(nbits - 64 * j, 0), 64)
        a[:, j] &= np.uint64((1 << keep) - 1)
    return a


def octets(rng, count):
    return rng.integers(0, 256, size=count, dtype=np.uint8)


def int8s(e, rng, polys, lo, hi):
    return rng.integers(lo, hi, size=(polys, e.n), dtype=np.int8)


class Env:
    """one ring shape on one context: the dimensions the reference derives and everything a call only reads (keys, plans), made once"""

    def __init__(self, shape, g, dims):
        import torch
        self.shape, self.g = shape, g
        self.logn, self.logq = SHAPES[shape]
        self.dimP, self.dimA, self.dimB, self.dimevk = dims
        self.n, self.W, self.batch = g.n, self.logq // 64 + 1, BATCH
        self.dim = self.dimB                                   # the RNS core calls
        self.dimpt, self.dimdec = dimpt_of(self.logq, self.logn), (self.logq + 1) // 59 + 1
        self.dimenc = self.dimP                                # hectx.dim, src/precomp.c:401
        self.per = self.batch * self.W * self.n
        assert g.nprimes >= max(self.dimevk, self.dimpt)
        rng = np.random.default_rng(zlib.crc32(("env " + shape).encode()))
        key = lambda: _dev(residues(self, rng, self.dimB, 1))
        self.rlk = (key(), key())
        self.rk = {r: (key(), key()) for r in sorted({0, 1, 2, 3} | set(ROTS4))}
        self.rots4 = (C.c_uint * len(ROTS4))(*ROTS4)
        self.rk4 = [g._key_ptrs([self.rk[r][side] for r in ROTS4]) for side in (0, 1)]
        self.gemv_keys = [g._key_ptrs([self.rk[r][side] for r in range(SLOTS)]) for side in (0, 1)]
        # a secret of weight 64 (sample_sk's), as big slabs, as an int8 slab and packed over the limbs each call multiplies in
        sk = np.zeros((1, self.n), dtype=np.int8)
        sk[0, rng.choice(self.n, 64, replace=False)] = rng.choice(np.array([-1, 1], dtype=np.int8), 64)
        self.sk_small = _dev(sk)
        P = 1
        for p in g.p[: self.dimP]:
            P *= int(p)
        self.nbitsk = (P << self.logq).bit_length()                # bits of P q_L: gpq_he_genswk's modulus (tests/genswk_model.py)
        self.Wk, self.dimmul = self.nbitsk // 64 + 1, g.he_genswk_dimmul(self.dimP, self.logq)
        wide = lambda W: _dev(np.concatenate([sk.astype(np.int64)[:, None, :], np.repeat((sk.astype(np.int64) >> 63)[:, None, :], W - 1, axis=1)], axis=1))
        self.sk_big, self.sk_wide = wide(self.W), wide(self.Wk)
        self.sk_dec, self.sk_enc, self.sk_mul = self.pack(self.sk_big, self.W, self.dimdec), self.pack(self.sk_big, self.W, self.dimenc), self.pack(self.sk_wide, self.Wk, self.dimmul)
        self.pk = [self.pack(_dev(centred(self, rng, 1)), self.W, self.dimenc) for _ in range(2)]
        self.galois = (C.c_uint64 * BATCH)(pow(5, 3, 1 << 64), 2 * self.n - 1, pow(5, self.n // 2 + 1, 1 << 64))
        # a general modulus of logq bits and its words; a Delta that is no power of two
        self.qgen = (1 << self.logq) - 0x1234567
        self.qw, self.Lq = _words(self.qgen)
        self.delta = (1 << LOGDELTA) - 35
        self.const_ab = ((3 << 20) + 1, -(5 << 19))
        assert g.he_mulpt_const_fits(*self.const_ab, self.logq, self.dimpt)
        # a 4-slot matrix (n1 = n2 = 2): the plan the planned calls run on, two more with other live sets for the set of three
        self.diag4 = _dev(small(self, rng, SLOTS))
        others = [small(self, rng, SLOTS) for _ in range(2)]
        others[0][[1, 3]] = 0
        others[1][2:] = 0
        self.d_others = [_dev(d) for d in others]
        self.plan4 = g.gemv_plan(self.diag4, SLOTS, self.W, self.logq, self.dimpt)
        self.others = [g.gemv_plan(d, SLOTS, self.W, self.logq, self.dimpt) for d in self.d_others]
        self.set = g.gemv_multi([self.plan4] + self.others)
        assert self.plan4.exact and self.plan4.live == SLOTS and [p.live for p in self.others] == [2, 2]
        self.ecd4 = g.ecd_plan(SLOTS)
        self.R = [_dev(centred(self, rng, 2 * BATCH)) for _ in range(2)]          # gpq_gemv_inner's rotations for the constructors' one inner sum
        from gpqhe_amd import Rng
        self.rng = Rng()
        torch.cuda.synchronize()

    def pack(self, big, W, dim):
        """gpq_evk_pack of ONE polynomial: rns_decompose + forward transform"""
        import torch
        out = torch.empty(dim * self.n, dtype=torch.int64, device="cuda")
        _ok(self.g, self.g.lib.gpq_evk_pack(self.g.h, _ptr(out), _ptr(big), W, dim, 1, self.g._stream()), "gpq_evk_pack")
        return out

    def close(self):
        self.set.close()
        for p in [self.plan4, self.ecd4] + self.others:
            p.close()
        self.rng.close()


class EcdEnv:
    """16 slots at logn 9: the encoder's and the decoder's one-block kernels"""

    def __init__(self, g):
        self.shape, self.g, self.logn, self.slots = ECD_SHAPE[0], g, ECD_SHAPE[1], ECD_SHAPE[2]
        self.n, self.W, self.batch, self.logDelta = g.n, 2, BATCH, 20
        self.plan = g.ecd_plan(self.slots)

    def close(self):
        self.plan.close()


# ---------------------------------------------------------------------------
# the closures
# ---------------------------------------------------------------------------
class Spec:
    """one run of an entry point: `call(g, ins, outs, ws)` with how its two input sets, its outputs and its workspace are made.
    ins(env, rng) -> {name: numpy array | host value}; outs(env) -> {name: (elements, numpy dtype)}; ws(env) -> bytes;
    inout: the inputs the call overwrites (they are results too); variant: a second run of the same entry point on other inputs"""

    def __init__(self, name, shapes, ins, outs, ws, call, inout=(), variant=""):
        self.name, self.shapes, self.ins, self.outs, self.ws, self.call, self.inout, self.variant = name, shapes, ins, outs, ws, call, tuple(inout), variant
        self.cls = TABLE[name]

    @property
    def key(self):
        return self.name + (" (%s)" % self.variant if self.variant else "")

    def seed(self, shape, which):
        return zlib.crc32(("%s %s %s" % (self.key, shape, which)).encode())


SPECS = []
CALLS = {}                              # C name -> its one closure


def spec(name, ins, outs, call, ws=lambda e: 0, shapes=RING, inout=(), variant=""):
    assert CALLS.setdefault(name, call) is call, name
    SPECS.append(Spec(name, shapes, ins, outs, ws, call, inout, variant))


U64, I8, U8, F64 = np.uint64, np.int8, np.uint8, np.float64
slab_out = lambda *names, dim=None, polys=None: (lambda e: {k: ((polys or e.batch) * (dim or e.dim) * e.n, U64) for k in names})
big_out = lambda *names, polys=None, W=None: (lambda e: {k: ((polys or e.batch) * (W or e.W) * e.n, U64) for k in names})
none_out = lambda e: {}


# --- the RNS core: gpq_ntt / gpq_invntt (also on a slab whose first polynomial has an all-zero limb: the zero flags and ref_zero_redo,
# tests/zero_cases.py "all-zero limb"), gpq_ntt_reference, the pointwise calls, the limb loops of poly_mul / he_mulpt, tensor and key switch
def _slab_ins(*names):
    return lambda e, rng: {k: residues(e, rng, e.dim, e.batch) for k in names}


def _zero_limb(e, rng):
    x = residues(e, rng, e.dim, e.batch)
    x[0, 0] = 0
    return {"x": x}


def _ntt(fn, *extra):
    def call(g, i, o, ws):
        e = i.env
        _ok(g, getattr(g.lib, fn)(g.h, _ptr(i["x"]), e.dim, e.batch, *extra, g._stream()), fn)
    return call


for _fn, _extra in (("gpq_ntt", ()), ("gpq_invntt", ()), ("gpq_ntt_reference", (0,))):
    _c = _ntt(_fn, *_extra)
    spec(_fn, _slab_ins("x"), none_out, _c, inout=("x",))
    if _fn != "gpq_ntt_reference":
        spec(_fn, _zero_limb, none_out, _c, inout=("x",), variant="all-zero limb")


def _pointwise(fn):
    def call(g, i, o, ws):
        e = i.env
        _ok(g, getattr(g.lib, fn)(g.h, _ptr(o["r"]), _ptr(i["a"]), _ptr(i["b"]), e.dim, e.batch, g._stream()), fn)
    return call


spec("gpq_rns_mul", _slab_ins("a", "b"), slab_out("r"), _pointwise("gpq_rns_mul"))
spec("gpq_rns_add", _slab_ins("a", "b"), slab_out("r"), _pointwise("gpq_rns_add"))
spec("gpq_poly_mul_rns", _slab_ins("a", "b"), slab_out("r"), _pointwise("gpq_poly_mul_rns"), inout=("a", "b"))      # a, b are scratch


def _mulpt_rns(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_mulpt_rns(g.h, _ptr(o["r0"]), _ptr(o["r1"]), _ptr(i["m"]), _ptr(i["x0"]), _ptr(i["x1"]), e.dim, e.batch, g._stream()), "gpq_mulpt_rns")


spec("gpq_mulpt_rns", _slab_ins("m", "x0", "x1"), slab_out("r0", "r1"), _mulpt_rns, inout=("m", "x0", "x1"))


def _tensor(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mul_tensor(g.h, _ptr(o["d0"]), _ptr(o["d1"]), _ptr(o["d2"]), _ptr(i["a0"]), _ptr(i["a1"]), _ptr(i["b0"]), _ptr(i["b1"]), e.dim, e.batch,
                                   _ptr(ws), g._stream()), "gpq_he_mul_tensor")


spec("gpq_he_mul_tensor", _slab_ins("a0", "a1", "b0", "b1"), slab_out("d0", "d1", "d2"), _tensor, ws=lambda e: e.g.lib.gpq_tensor_workspace_bytes(e.g.h, e.dim, e.batch))


def _keyswitch(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_keyswitch(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["x"]), _ptr(e.rlk[0]), _ptr(e.rlk[1]), e.dim, e.batch, _ptr(ws), g._stream()), "gpq_keyswitch")


spec("gpq_keyswitch", _slab_ins("x"), slab_out("c0", "c1"), _keyswitch, ws=lambda e: e.g.lib.gpq_keyswitch_workspace_bytes(e.g.h, e.dim, e.batch))


# --- the bridge on big slabs
def _big_ins(*names):
    return lambda e, rng: {k: centred(e, rng, e.batch) for k in names}


def _decompose(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_rns_decompose(g.h, _ptr(o["slab"]), _ptr(i["big"]), e.W, e.dim, e.batch, g._stream()), "gpq_rns_decompose")


def _decompose_limbs(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_rns_decompose_limbs(g.h, _ptr(o["slab"]), _ptr(i["big"]), e.W, 1, e.dim - 1, e.batch, g._stream()), "gpq_rns_decompose_limbs")


spec("gpq_rns_decompose", _big_ins("big"), slab_out("slab"), _decompose)
spec("gpq_rns_decompose_limbs", _big_ins("big"), lambda e: {"slab": (e.batch * (e.dim - 1) * e.n, U64)}, _decompose_limbs)


def _reconstruct(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_rns_reconstruct(g.h, _ptr(o["big"]), e.W, _ptr(i["slab"]), e.dimpt, e.batch, e.logq, g._stream()), "gpq_rns_reconstruct")


def _reconstruct_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_rns_reconstruct_general(g.h, _ptr(o["big"]), e.W, _ptr(i["slab"]), e.dimpt, e.batch, e.qw, e.Lq, _ptr(ws), g._stream()), "gpq_rns_reconstruct_general")


_pt_slab = lambda e, rng: {"slab": residues(e, rng, e.dimpt, e.batch)}
_general_ws = lambda e: e.g.lib.gpq_poly_mul_general_workspace_bytes(e.g.h, e.dimpt, e.batch)
spec("gpq_rns_reconstruct", _pt_slab, big_out("big"), _reconstruct)
spec("gpq_rns_reconstruct_general", _pt_slab, big_out("big"), _reconstruct_general, ws=_general_ws)


def _poly_mul(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_poly_mul(g.h, _ptr(o["r"]), _ptr(i["a"]), _ptr(i["b"]), e.W, e.dimpt, e.logq, e.batch, _ptr(ws), g._stream()), "gpq_poly_mul")


def _poly_mul_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_poly_mul_general(g.h, _ptr(o["r"]), _ptr(i["a"]), _ptr(i["b"]), e.W, e.dimpt, e.qw, e.Lq, e.batch, _ptr(ws), g._stream()), "gpq_poly_mul_general")


_ct_pt = lambda e, rng: {"a": centred(e, rng, e.batch), "b": small(e, rng, e.batch)}
spec("gpq_poly_mul", _ct_pt, big_out("r"), _poly_mul, ws=lambda e: e.g.lib.gpq_poly_mul_workspace_bytes(e.g.h, e.dimpt, e.batch))
spec("gpq_poly_mul_general", lambda e, rng: {"a": centred(e, rng, e.batch, e.logq - 1), "b": small(e, rng, e.batch)}, big_out("r"), _poly_mul_general, ws=_general_ws)


def _rs(fn):
    def call(g, i, o, ws):
        e = i.env
        _ok(g, getattr(g.lib, fn)(g.h, _ptr(i["c0"]), _ptr(i["c1"]), e.W, LOGDELTA, e.logq - LOGDELTA, e.batch, g._stream()), fn)
    return call


spec("gpq_he_rs", _big_ins("c0", "c1"), none_out, _rs("gpq_he_rs"), inout=("c0", "c1"))
spec("gpq_he_rescale", _big_ins("c0", "c1"), none_out, _rs("gpq_he_rescale"), inout=("c0", "c1"))


def _rs_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_rs_general(g.h, _ptr(i["c0"]), _ptr(i["c1"]), e.W, e.delta, e.qw, e.Lq, e.batch, _ptr(ws), g._stream()), "gpq_he_rs_general")


spec("gpq_he_rs_general", _big_ins("c0", "c1"), none_out, _rs_general, ws=lambda e: 192 * 8, inout=("c0", "c1"))

_four = ("a0", "a1", "b0", "b1")
_he_mul_ws = lambda e: e.g.lib.gpq_he_mul_workspace_bytes(e.g.h, e.W, e.dimA, e.dimB, e.dimP, e.batch)


def _he_mul(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mul(g.h, _ptr(o["c0"]), _ptr(o["c1"]), *[_ptr(i[k]) for k in _four], _ptr(e.rlk[0]), _ptr(e.rlk[1]), e.W, e.logq, e.dimA, e.dimB, e.dimP,
                            e.batch, _ptr(ws), g._stream()), "gpq_he_mul")


def _he_mul_rs(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mul_rs(g.h, _ptr(o["c0"]), _ptr(o["c1"]), *[_ptr(i[k]) for k in _four], _ptr(e.rlk[0]), _ptr(e.rlk[1]), e.W, e.logq, e.dimA, e.dimB, e.dimP,
                               LOGDELTA, e.batch, _ptr(ws), g._stream()), "gpq_he_mul_rs")


def _he_mul_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mul_general(g.h, _ptr(o["c0"]), _ptr(o["c1"]), *[_ptr(i[k]) for k in _four], _ptr(e.rlk[0]), _ptr(e.rlk[1]), e.W, e.qw, e.Lq, e.dimA, e.dimB,
                                    e.dimP, e.batch, _ptr(ws), g._stream()), "gpq_he_mul_general")


_below_q = lambda *names: (lambda e, rng: {k: centred(e, rng, e.batch, e.logq - 1) for k in names})          # centred mod the general modulus too
spec("gpq_he_mul", _big_ins(*_four), big_out("c0", "c1"), _he_mul, ws=_he_mul_ws)
spec("gpq_he_mul_rs", _big_ins(*_four), big_out("c0", "c1"), _he_mul_rs, ws=_he_mul_ws)
spec("gpq_he_mul_general", _below_q(*_four), big_out("c0", "c1"), _he_mul_general,
     ws=lambda e: e.g.lib.gpq_he_general_workspace_bytes(e.g.h, e.W, e.dimA, e.dimB, e.dimP, e.batch))

_tail_ins = lambda e, rng: {"chat": residues(e, rng, e.dimB, e.batch), "d": centred(e, rng, e.batch)}
_tail_ws = lambda e: e.g.lib.gpq_relin_tail_workspace_bytes(e.g.h, e.W, e.dimB, e.dimP, e.batch)


def _tail(fn):
    def call(g, i, o, ws):
        e = i.env
        _ok(g, getattr(g.lib, fn)(g.h, _ptr(o["out"]), _ptr(i["chat"]), _ptr(i["d"]), e.W, e.logq, e.dimB, e.dimP, e.batch, _ptr(ws), g._stream()), fn)
    return call


def _tail_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_relin_tail_general(g.h, _ptr(o["out"]), _ptr(i["chat"]), _ptr(i["d"]), e.W, e.qw, e.Lq, e.dimB, e.dimP, e.batch, _ptr(ws), g._stream()),
        "gpq_relin_tail_general")


spec("gpq_relin_tail", _tail_ins, big_out("out"), _tail("gpq_relin_tail"), ws=_tail_ws)
spec("gpq_relin_tail_overwriting", _tail_ins, big_out("out"), _tail("gpq_relin_tail_overwriting"), ws=_tail_ws, inout=("chat",))
spec("gpq_relin_tail_general", lambda e, rng: {"chat": residues(e, rng, e.dimB, e.batch), "d": centred(e, rng, e.batch, e.logq - 1)}, big_out("out"), _tail_general,
     ws=lambda e: e.batch * e.g.lib.gpq_he_general_workspace_bytes(e.g.h, e.W, 0, e.dimB, e.dimP, 1))     # (gpqhe_amd/engine.py: relin_tail_general)


def _transpose(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_big_transpose(g.h, _ptr(o["dst"]), _ptr(i["src"]), e.W, e.batch, 1, g._stream()), "gpq_big_transpose")


def _addsub(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_big_addsub(g.h, _ptr(o["out"]), _ptr(i["a"]), _ptr(i["b"]), e.W, e.batch, 1, g._stream()), "gpq_big_addsub")


def _big2(fn):
    def call(g, i, o, ws):
        e = i.env
        _ok(g, getattr(g.lib, fn)(g.h, _ptr(o["r"]), _ptr(i["a"]), _ptr(i["b"]), e.W, e.logq, e.batch, g._stream()), fn)
    return call


def _big_neg(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_big_neg(g.h, _ptr(o["r"]), _ptr(i["a"]), e.W, e.logq, e.batch, g._stream()), "gpq_big_neg")


spec("gpq_big_transpose", _big_ins("src"), big_out("dst"), _transpose)
spec("gpq_big_addsub", _big_ins("a", "b"), big_out("out"), _addsub)
spec("gpq_big_add", _big_ins("a", "b"), big_out("r"), _big2("gpq_big_add"))
spec("gpq_big_sub", _big_ins("a", "b"), big_out("r"), _big2("gpq_big_sub"))
spec("gpq_big_neg", _big_ins("a"), big_out("r"), _big_neg)

_swk_ws = lambda e: e.g.lib.gpq_he_swk_workspace_bytes(e.g.h, e.W, e.dimB, e.dimP, e.batch)


def _swk(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_swk(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["d0"]), _ptr(i["d1"]), _ptr(e.rk[0][0]), _ptr(e.rk[0][1]), e.W, e.logq, e.dimB, e.dimP,
                            e.batch, _ptr(ws), g._stream()), "gpq_he_swk")


def _swk_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_swk_general(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["d0"]), _ptr(i["d1"]), _ptr(e.rk[0][0]), _ptr(e.rk[0][1]), e.W, e.qw, e.Lq, e.dimB,
                                    e.dimP, e.batch, _ptr(ws), g._stream()), "gpq_he_swk_general")


spec("gpq_he_swk", _big_ins("d0", "d1"), big_out("c0", "c1"), _swk, ws=_swk_ws)
spec("gpq_he_swk_general", _below_q("d0", "d1"), big_out("c0", "c1"), _swk_general,
     ws=lambda e: e.g.lib.gpq_he_general_workspace_bytes(e.g.h, e.W, 0, e.dimB, e.dimP, e.batch))

_mulpt_ins = lambda e, rng: {"c0": centred(e, rng, e.batch), "c1": centred(e, rng, e.batch), "m": small(e, rng, e.batch)}
_mulpt_ws = lambda e: e.g.lib.gpq_he_mulpt_workspace_bytes(e.g.h, e.dimpt, e.batch)


def _mulpt(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mulpt(g.h, _ptr(o["o0"]), _ptr(o["o1"]), _ptr(i["c0"]), _ptr(i["c1"]), _ptr(i["m"]), e.W, e.logq, e.dimpt, e.batch, _ptr(ws), g._stream()),
        "gpq_he_mulpt")


def _mulpt_general(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mulpt_general(g.h, _ptr(o["o0"]), _ptr(o["o1"]), _ptr(i["c0"]), _ptr(i["c1"]), _ptr(i["m"]), e.W, e.qw, e.Lq, e.dimpt, e.batch, _ptr(ws),
                                      g._stream()), "gpq_he_mulpt_general")


spec("gpq_he_mulpt", _mulpt_ins, big_out("o0", "o1"), _mulpt, ws=_mulpt_ws)
spec("gpq_he_mulpt_general", lambda e, rng: {"c0": centred(e, rng, e.batch, e.logq - 1), "c1": centred(e, rng, e.batch, e.logq - 1), "m": small(e, rng, e.batch)},
     big_out("o0", "o1"), _mulpt_general, ws=lambda e: _mulpt_ws(e) + _general_ws(e))


def _rot(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_poly_rot(g.h, _ptr(o["r"]), _ptr(i["a"]), e.W, 3, e.batch, g._stream()), "gpq_poly_rot")


def _conj(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_poly_conj(g.h, _ptr(o["r"]), _ptr(i["a"]), e.W, e.batch, g._stream()), "gpq_poly_conj")


spec("gpq_poly_rot", _big_ins("a"), big_out("r"), _rot)
spec("gpq_poly_conj", _big_ins("a"), big_out("r"), _conj)


def _mulpt_const(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_mulpt_const(g.h, _ptr(o["o0"]), _ptr(o["o1"]), _ptr(i["c0"]), _ptr(i["c1"]), e.const_ab[0], e.const_ab[1], e.W, e.logq, e.dimpt, LOGDELTA,
                                    e.batch, None, g._stream()), "gpq_he_mulpt_const")


def _addpt_const(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_addpt_const(g.h, _ptr(o["o0"]), _ptr(o["o1"]), _ptr(i["c0"]), _ptr(i["c1"]), e.const_ab[0], e.const_ab[1], 0, e.W, e.logq, e.batch,
                                    g._stream()), "gpq_he_addpt_const")


spec("gpq_he_mulpt_const", _big_ins("c0", "c1"), big_out("o0", "o1"), _mulpt_const)
spec("gpq_he_addpt_const", _big_ins("c0", "c1"), big_out("o0", "o1"), _addpt_const)


# --- hoisted rotations and the he_gemv family (tests/test_settings_derived_gpu.py: _rot, _gemv, _planned, _inner, _multi)
def _rot_hoisted(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_rot_hoisted(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["c0"]), _ptr(i["c1"]), e.rots4, e.rk4[0], e.rk4[1], len(ROTS4), e.W, e.logq, e.dimB,
                                    e.dimP, e.batch, _ptr(ws), g._stream()), "gpq_he_rot_hoisted")


spec("gpq_he_rot_hoisted", _big_ins("c0", "c1"), big_out("c0", "c1", polys=len(ROTS4) * BATCH), _rot_hoisted,
     ws=lambda e: e.g.lib.gpq_he_rot_hoisted_workspace_bytes(e.g.h, e.W, e.dimB, e.dimP, len(ROTS4), e.batch))


def _gemv(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_gemv(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["c0"]), _ptr(i["c1"]), _ptr(e.diag4), e.gemv_keys[0], e.gemv_keys[1], SLOTS, e.W, e.logq,
                             LOGDELTA, e.dimB, e.dimP, e.dimpt, e.batch, _ptr(ws), g._stream()), "gpq_he_gemv")


spec("gpq_he_gemv", _big_ins("c0", "c1"), big_out("c0", "c1"), _gemv,
     ws=lambda e: e.g.lib.gpq_he_gemv_workspace_bytes(e.g.h, e.W, SLOTS, e.dimB, e.dimP, e.dimpt, e.batch))


def _planned(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_gemv_planned(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["c0"]), _ptr(i["c1"]), e.plan4.h, e.gemv_keys[0], e.gemv_keys[1], e.W, LOGDELTA,
                                     e.dimB, e.dimP, e.batch, _ptr(ws), g._stream()), "gpq_he_gemv_planned")


spec("gpq_he_gemv_planned", _big_ins("c0", "c1"), big_out("c0", "c1"), _planned,
     ws=lambda e: e.g.lib.gpq_he_gemv_planned_workspace_bytes(e.g.h, e.plan4.h, e.W, e.dimB, e.dimP, e.batch))


def _multi(g, i, o, ws):
    e = i.env
    outs0, outs1 = [g._key_ptrs([o["p%dc%d" % (t, side)] for t in range(3)]) for side in (0, 1)]
    _ok(g, g.lib.gpq_he_gemv_multi(g.h, outs0, outs1, _ptr(i["c0"]), _ptr(i["c1"]), e.set.h, e.gemv_keys[0], e.gemv_keys[1], e.W, LOGDELTA, e.dimB, e.dimP,
                                   e.batch, _ptr(ws), g._stream()), "gpq_he_gemv_multi")


spec("gpq_he_gemv_multi", _big_ins("c0", "c1"), big_out(*["p%dc%d" % (t, side) for t in range(3) for side in (0, 1)]), _multi,
     ws=lambda e: e.g.lib.gpq_he_gemv_multi_workspace_bytes(e.g.h, e.set.h, e.W, e.dimB, e.dimP, e.batch))

_inner_ws = lambda e: (2 * 2 + 2) * bs.CHUNK * e.g.nprimes * e.n * 8 + 256          # gpq_gemv_inner_workspace_bytes for n1 = 2 and any dim of the context


def _inner_call(g, e, plan_h, o, R0, R1, ws):
    need = g.lib.gpq_gemv_inner_workspace_bytes(g.h, plan_h, e.batch)
    assert 0 < need <= ws.numel() * 8, need
    _ok(g, g.lib.gpq_gemv_inner(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(R0), _ptr(R1), plan_h, 1, e.W, e.batch, _ptr(ws), g._stream()), "gpq_gemv_inner")


def _inner(g, i, o, ws):
    _inner_call(g, i.env, i.env.plan4.h, o, i["R0"], i["R1"], ws)


spec("gpq_gemv_inner", lambda e, rng: {"R0": centred(e, rng, 2 * e.batch), "R1": centred(e, rng, 2 * e.batch)}, big_out("c0", "c1"), _inner, ws=_inner_ws)


def _plan_result(g, e, h, o, ws):
    """a constructor's result: its plan's gpq_gemv_plan_info (and diag_bits) plus one gpq_gemv_inner on the shape's fixed rotations"""
    dim, nbytes, live, exact = C.c_uint(), C.c_size_t(), C.c_uint(), C.c_int()
    try:
        _ok(g, g.lib.gpq_gemv_plan_info(h, C.byref(dim), C.byref(nbytes), C.byref(live), C.byref(exact)), "gpq_gemv_plan_info")
        info = (dim.value, nbytes.value, live.value, exact.value, int(g.lib.gpq_gemv_plan_diag_bits(h)))
        _inner_call(g, e, h, o, e.R[0], e.R[1], ws)
    finally:
        g.lib.gpq_gemv_plan_destroy(h)                 # (its hipFree waits for the inner sum)
    return info


def _plan_create(g, i, o, ws):
    e, h = i.env, C.c_void_p()
    _ok(g, g.lib.gpq_gemv_plan_create(g.h, C.byref(h), _ptr(i["diag"]), SLOTS, e.W, e.logq, e.dimpt, g._stream()), "gpq_gemv_plan_create")
    return _plan_result(g, e, h, o, ws)


def _plan_from_matrix(g, i, o, ws):
    e, h = i.env, C.c_void_p()
    _ok(g, g.lib.gpq_gemv_plan_create_from_matrix(g.h, C.byref(h), e.ecd4.h, _ptr(i["A"]), LOGDELTA, e.logq, e.dimpt, g._stream()), "gpq_gemv_plan_create_from_matrix")
    return _plan_result(g, e, h, o, ws)


def _diag_ins(e, rng):
    """diagonals whose measurement differs between two draws: 23 .. 30 bits by the seed, one zero diagonal"""
    bits = 23 + int(rng.integers(0, 8))
    d = small(e, rng, SLOTS, bits)
    d[:, 0, 0] = (1 << bits) - 1
    d[:, 1:, 0] = 0
    d[int(rng.integers(0, 2))] = 0
    return {"diag": d}


def _matrix_ins(e, rng):
    scale = 2.0 ** -int(rng.integers(0, 8))
    return {"A": (rng.uniform(-1, 1, (SLOTS, SLOTS)) + 1j * rng.uniform(-1, 1, (SLOTS, SLOTS))) * scale}


spec("gpq_gemv_plan_create", _diag_ins, big_out("c0", "c1"), _plan_create, ws=_inner_ws)
spec("gpq_gemv_plan_create_from_matrix", _matrix_ins, big_out("c0", "c1"), _plan_from_matrix, ws=_inner_ws)


# --- decryption, the samplers and encryption (tests/test_settings_bridge_calls_gpu.py: _all_calls)
def _dec(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_dec(g.h, _ptr(o["m"]), _ptr(i["c0"]), _ptr(i["c1"]), _ptr(e.sk_dec), e.W, e.logq, e.dimdec, e.batch, _ptr(ws), g._stream()), "gpq_he_dec")


spec("gpq_he_dec", _big_ins("c0", "c1"), big_out("m"), _dec, ws=lambda e: e.g.lib.gpq_he_dec_workspace_bytes(e.g.h, e.dimdec, e.batch))


def _sampler(fn):
    def call(g, i, o, ws):
        _ok(g, getattr(g.lib, fn)(g.h, _ptr(o["out"]), _ptr(i["bytes"]), i.env.batch, g._stream()), fn)
    return call


def _uniform(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_sample_uniform(g.h, _ptr(o["big"]), _ptr(i["bytes"]), e.logq + 1, e.W, e.batch, g._stream()), "gpq_sample_uniform")


def _small_to_big(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_small_to_big(g.h, _ptr(o["big"]), _ptr(i["small"]), e.W, e.batch, g._stream()), "gpq_small_to_big")


_small_out = lambda e: {"out": (e.batch * e.n, I8)}
spec("gpq_sample_zo", lambda e, rng: {"bytes": octets(rng, e.batch * e.n // 4)}, _small_out, _sampler("gpq_sample_zo"))
spec("gpq_sample_error", lambda e, rng: {"bytes": octets(rng, e.batch * e.n)}, _small_out, _sampler("gpq_sample_error"))
spec("gpq_sample_uniform", lambda e, rng: {"bytes": octets(rng, e.batch * e.n * ((e.logq + 1) // 8 + 1))}, big_out("big"), _uniform)
spec("gpq_small_to_big", lambda e, rng: {"small": int8s(e, rng, e.batch, -11, 12)}, big_out("big"), _small_to_big)


def _enc_pk(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_enc_pk(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["m"]), _ptr(i["v"]), _ptr(i["e0"]), _ptr(i["e1"]), _ptr(e.pk[0]), _ptr(e.pk[1]), e.W, e.logq,
                               e.dimenc, e.batch, _ptr(ws), g._stream()), "gpq_he_enc_pk")


def _enc_sk(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_enc_sk(g.h, _ptr(o["c0"]), _ptr(o["c1"]), _ptr(i["m"]), _ptr(i["a"]), _ptr(i["e"]), _ptr(e.sk_enc), e.W, e.logq, e.dimenc, e.batch, _ptr(ws),
                               g._stream()), "gpq_he_enc_sk")


spec("gpq_he_enc_pk", lambda e, rng: {"m": small(e, rng, e.batch, 40), "v": int8s(e, rng, e.batch, -1, 2), "e0": int8s(e, rng, e.batch, -11, 12),
                                      "e1": int8s(e, rng, e.batch, -11, 12)}, big_out("c0", "c1"), _enc_pk,
     ws=lambda e: e.g.lib.gpq_he_enc_workspace_bytes(e.g.h, e.dimenc, e.batch, 1))
spec("gpq_he_enc_sk", lambda e, rng: {"m": small(e, rng, e.batch, 40), "a": raw(e, rng, e.batch, e.logq + 1, e.W), "e": int8s(e, rng, e.batch, -11, 12)},
     big_out("c0", "c1"), _enc_sk, ws=lambda e: e.g.lib.gpq_he_enc_workspace_bytes(e.g.h, e.dimenc, e.batch, 0))


# --- key generation: gpq_evk_pack, gpq_he_genswk (key 0 from big slabs), gpq_he_genswk_batch (three keys from the secret's Galois images)
def _evk_pack(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_evk_pack(g.h, _ptr(o["evk"]), _ptr(i["big"]), e.W, e.dimevk, e.batch, g._stream()), "gpq_evk_pack")


spec("gpq_evk_pack", _big_ins("big"), lambda e: {"evk": (e.batch * e.dimevk * e.n, U64)}, _evk_pack)
_key_out = lambda count: (lambda e: {k: (count * e.dimevk * e.n, U64) for k in ("evk0", "evk1")})


def _genswk(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_genswk(g.h, _ptr(o["evk0"]), _ptr(o["evk1"]), _ptr(i["p1"]), _ptr(e.sk_wide), _ptr(i["e"]), _ptr(i["sp"]), e.Wk, e.dimP, e.logq, e.dimevk,
                               _ptr(ws), g._stream()), "gpq_he_genswk")


def _genswk_batch(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_genswk_batch(g.h, _ptr(o["evk0"]), _ptr(o["evk1"]), _ptr(i["p1"]), _ptr(i["e"]), _ptr(e.sk_mul), _ptr(e.sk_small), e.galois, None, 0, e.Wk,
                                     e.dimP, e.logq, e.dimevk, e.batch, _ptr(ws), g._stream()), "gpq_he_genswk_batch")


spec("gpq_he_genswk", lambda e, rng: {"p1": raw(e, rng, 1, e.nbitsk, e.Wk), "e": small(e, rng, 1, W=e.Wk, lo=-11, hi=12), "sp": small(e, rng, 1, W=e.Wk, lo=-1, hi=2)},
     _key_out(1), _genswk, ws=lambda e: e.g.lib.gpq_he_genswk_workspace_bytes(e.g.h, e.Wk, e.dimP, e.logq))
spec("gpq_he_genswk_batch", lambda e, rng: {"p1": raw(e, rng, e.batch, e.nbitsk, e.Wk), "e": int8s(e, rng, e.batch, -11, 12)}, _key_out(BATCH), _genswk_batch,
     ws=lambda e: e.g.lib.gpq_he_genswk_batch_workspace_bytes(e.g.h, e.Wk, e.dimP, e.logq, e.dimevk, e.batch))


# --- the byte generators: no device input, so the two input sets are two odd stream positions (host arguments); SURF_LEN bytes to an odd address
def _surf(g, i, o, ws):
    _ok(g, g.lib.gpq_surf_bytes(g.h, o["bytes"].data_ptr() + 3, SURF_LEN, None, i["pos"] & 0xFFFFFFFFFFFFFFFF, i["pos"] >> 64, g._stream()), "gpq_surf_bytes")


def _rng_bytes(g, i, o, ws):
    i.env.rng.seek(i["pos"])                        # host only: the object's position, which the call reads and advances
    _ok(g, g.lib.gpq_rng_device_bytes(g.h, i.env.rng.h, o["bytes"].data_ptr() + 3, SURF_LEN, g._stream()), "gpq_rng_device_bytes")


_pos_ins = lambda e, rng: {"pos": (int(rng.integers(1, 1 << 62)) << 3) | 1 | (int(rng.integers(0, 4)) << 64)}
_bytes_out = lambda e: {"bytes": (SURF_LEN + 16, U8)}
spec("gpq_surf_bytes", _pos_ins, _bytes_out, _surf, shapes=("S2",))
spec("gpq_rng_device_bytes", _pos_ins, _bytes_out, _rng_bytes, shapes=("S2",))


# --- encoder and decoder, one block: 16 slots at logn 9
def _ecd(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_ecd(g.h, e.plan.h, _ptr(o["out"]), _ptr(i["z"]), e.logDelta, e.W, e.batch, None, g._stream()), "gpq_he_ecd")


def _ecd_diagonals(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_ecd_diagonals(g.h, e.plan.h, _ptr(o["out"]), _ptr(i["A"]), e.logDelta, e.W, None, g._stream()), "gpq_he_ecd_diagonals")


def _dcd(g, i, o, ws):
    e = i.env
    _ok(g, g.lib.gpq_he_dcd(g.h, e.plan.h, _ptr(o["z"]), _ptr(i["in"]), 1.5 * 2.0 ** e.logDelta, e.W, e.batch, g._stream()), "gpq_he_dcd")


_complex = lambda rng, *shape: np.stack([rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)], axis=-1)
spec("gpq_he_ecd", lambda e, rng: {"z": _complex(rng, e.batch, e.slots)}, lambda e: {"out": (e.batch * e.W * e.n, U64)}, _ecd, shapes=ECD)
spec("gpq_he_ecd_diagonals", lambda e, rng: {"A": _complex(rng, e.slots, e.slots)}, lambda e: {"out": (e.slots * e.W * e.n, U64)}, _ecd_diagonals, shapes=ECD)
spec("gpq_he_dcd", lambda e, rng: {"in": small(e, rng, e.batch, 40, e.W)}, lambda e: {"z": (e.batch * e.slots * 2, F64)}, _dcd, shapes=ECD)


def to_tensors(env, made):
    """a generator's numpy arrays on the device (complex as (re, im) pairs); host values stay as they are"""
    out = Args(env)
    for k, v in made.items():
        if isinstance(v, np.ndarray):
            v = _dev(np.stack([v.real, v.imag], axis=-1) if np.iscomplexobj(v) else v)
        out[k] = v
    return out
