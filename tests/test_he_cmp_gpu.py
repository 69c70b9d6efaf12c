"""gpq_he_cmp / gpq_he_cmppt (include/gpqhe_hip_algo.h): the reference's he_cmp and he_cmppt (src/he-algo.c:460-548) as single calls.

Every result is compared, without a tolerance,
  * with the SAME sequence (tests/cmp_model.py, the reference's calls one by one, the nested he_inv being tests/algo_model.py's) issued as
    separate public calls that existed before (tests/cmp_device.py's CmpDeviceOps);
  * with that sequence on the restated reference (oracle/bigint_ref.py) on the first and the last ciphertext of the batch.
Shapes: the cases of tests/test_cmp_model.py at logn 7, q_L = 2^200, Delta = 2^20, batch 2, at the top level and two levels below it; batch 3
in launch groups of 2; a two-pass ring (logn 13); W = 1; Delta at the largest scale he_inv's constant 2 allows and the first it does not.
Also: inputs untouched, a workspace of exactly the declared size with a guard behind it, in place on the first input, every refusal with
poisoned outputs left alone, each call behind a sleeping producer on a non-blocking side stream and inside a captured graph replayed on
other inputs (the protocol of tests/test_he_algo_gpu.py), and the launch classes."""
import ctypes as C
import time

import pytest

from gpqhe_amd import big_to_ints, to_host
from tests import algo_model as am
from tests import bridge_settings as bs
from tests import cmp_model as cm
from tests.cmp_device import PAIRS, CmpDeviceOps, CmpEnv
from tests.test_cmp_model import CASES, IDS
from tests.test_he_algo_gpu import _overtaken
from tests.test_he_algo_shapes_gpu import Constants, Products

pytestmark = pytest.mark.gpu

LOGN, LOGQ, LOGDELTA, BATCH = 7, 200, 20, 2
GPQ_ERR_INVALID = -1
POISON = 0x5A5A5A5A5A5A5A5A
INT64_MAX = (1 << 63) - 1
FNS = ("cmp", "cmppt")


def _torch():
    import torch
    return torch


_ENVS = {}


def _env(engine_ctx, oracle_ctx, key, *args, **kw):
    if key not in _ENVS:
        _ENVS[key] = CmpEnv(engine_ctx, oracle_ctx, *args, **kw)
    return _ENVS[key]


def _small(engine_ctx, oracle_ctx, down=0):
    return _env(engine_ctx, oracle_ctx, ("small", down), LOGN, LOGQ, LOGDELTA, BATCH, 21 + down, down)


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    _torch().cuda.synchronize()
    _ENVS.clear()


def _run(env, fn, iter, t, pair="AB", pt=None, in_place=False):
    """the call on fresh copies of the pair's first input -> (out0, out1, the inputs it was given, the workspace and its declared words)"""
    torch = _torch()
    c0, c1 = (x.clone() for x in env.dev[PAIRS[pair][0]])
    o0, o1 = (c0, c1) if in_place else (torch.full_like(c0, POISON), torch.full_like(c1, POISON))
    ws, words = env.cmp_workspace(fn, iter, t)
    rc = env.cmp_call(fn, iter, t, c0, c1, env.other(fn, pair, pt), o0, o1, ws)
    assert rc == 0, env.g.lib.gpq_last_error().decode()
    torch.cuda.synchronize()
    return o0, o1, (c0, c1), ws, words


def _assert_cell(env, fn, iter, t, pair="AB", pt=None, restated=(0, -1)):
    torch = _torch()
    a, b, m = PAIRS[pair]
    before = [x.clone() for x in env.dev[b]] + [env.pt[pt or m].clone()]
    o0, o1, ins, ws, words = _run(env, fn, iter, t, pair, pt)
    want = env.separate(fn, iter, t, pair, pt)
    assert torch.equal(o0, want[0]) and torch.equal(o1, want[1]), "not the words of the separate calls"
    assert torch.equal(ins[0], env.dev[a][0]) and torch.equal(ins[1], env.dev[a][1]), "the first input changed"
    assert torch.equal(before[0], env.dev[b][0]) and torch.equal(before[1], env.dev[b][1]) and torch.equal(before[2], env.pt[pt or m]), "the second input changed"
    assert bool((ws[words:] == 0x6B6B6B6B).all()), "the call wrote behind its declared workspace"
    got = [big_to_ints(to_host(x), env.W, env.g.n) for x in (o0, o1)]
    for k in sorted(set(range(env.batch)[i] for i in restated)):
        c = env.restated(fn, iter, t, k, pair, pt)
        assert got[0][k] == c[0] and got[1][k] == c[1], "ciphertext %d differs from the restated reference" % k
    return o0, o1


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("down,iter,t", CASES, ids=IDS)
def test_one_call_equals_the_separate_calls_and_the_restated_reference(engine_ctx, oracle_ctx, down, iter, t, fn):
    env = _small(engine_ctx, oracle_ctx, down)
    o0, _ = _assert_cell(env, fn, iter, t)
    assert env.g.he_cmp_depth(iter, t) == cm.depth(iter, t)
    assert bool((o0 != 0).any())
    if fn == "cmppt" and (iter, t) in ((0, 0), (1, 1)):     # he_const_pt(1) as the dense plaintext
        _assert_cell(env, fn, iter, t, pt="one", restated=(0,))


def test_another_pair_gives_other_words(engine_ctx, oracle_ctx):
    torch = _torch()
    env = _small(engine_ctx, oracle_ctx)
    for fn in FNS:
        assert not torch.equal(_assert_cell(env, fn, 1, 0, "AB")[0], _assert_cell(env, fn, 1, 0, "CD")[0])


@pytest.mark.parametrize("fn", FNS)
def test_in_place_on_the_first_input(engine_ctx, oracle_ctx, fn):
    torch = _torch()
    env = _small(engine_ctx, oracle_ctx)
    for iter, t in ((0, 0), (1, 1)):
        c0, c1, _, ws, words = _run(env, fn, iter, t, in_place=True)
        want = env.separate(fn, iter, t)
        assert torch.equal(c0, want[0]) and torch.equal(c1, want[1]), (iter, t)
        assert bool((ws[words:] == 0x6B6B6B6B).all())


@pytest.mark.parametrize("fn", FNS)
def test_batch_three_in_launch_groups_of_two(engine_ctx, oracle_ctx, fn):
    env = _env(engine_ctx, oracle_ctx, "three", LOGN, LOGQ, LOGDELTA, 3, 31)
    env.g.set_chunk(2)
    try:
        _assert_cell(env, fn, 1, 1)
    finally:
        _torch().cuda.synchronize()
        env.g.set_chunk(32)


@pytest.mark.parametrize("fn", FNS)
def test_two_pass_ring(engine_ctx, oracle_ctx, fn):
    env = _env(engine_ctx, oracle_ctx, "big", 13, 200, 30, 3, 41)
    _assert_cell(env, fn, 1, 0, restated=())


@pytest.mark.parametrize("fn", FNS)
def test_one_word(engine_ctx, oracle_ctx, fn):
    env = _env(engine_ctx, oracle_ctx, "w1", LOGN, 200, 4, BATCH, 51, 40, 1)       # q_l = 2^40, six levels of 2^4
    assert env.W == 1 and env.logql0 == 40
    _assert_cell(env, fn, 0, 1)


# ---------------------------------------------------------------------------
# the largest Delta the constants allow, and the first they do not
# ---------------------------------------------------------------------------
class CmpConstants(Constants):
    def addpt_dense(self, dst, src, m, pt_nu):
        dst.l = src.l


EDGE_SPARE = 20


def _accepted(iter, t, logdelta, logq, primes):
    """every he_const_pt of the sequence is an int64_t, and every constant FACTOR a keeps he_mulpt's words: a 2^(logql - 1) < floor(P / 2) over
    the reference's limb count at the operand's level (the rule above gpq_he_mulpt_const_fits, include/gpqhe_hip.h)"""
    L = logq // logdelta
    ops = CmpConstants(L)
    cm.he_cmp(ops, am.Ct(None, L), am.Ct(None, L), iter, t)
    for re, l, factor in ops.seen:
        a = abs(am.const_int(re, logdelta))
        if a > INT64_MAX:
            return False
        if factor:
            logql = logq - (L - l) * logdelta
            P = 1
            for p in primes[:(logql + 1 + logdelta + LOGN) // 59 + 1]:
                P *= int(p)
            if not a << (logql - 1) < P // 2:
                return False
    return True


@pytest.mark.parametrize("fn", FNS)
def test_constant_edges(engine_ctx, oracle_ctx, fn):
    torch = _torch()
    iter, t = 0, 0
    depth = cm.depth(iter, t)
    logq_for = lambda d: depth * d + EDGE_SPARE
    primes = oracle_ctx(LOGN, am.primes_for(LOGN, logq_for(63))).p
    ok = [d for d in range(1, 64) if _accepted(iter, t, d, logq_for(d + 1), primes)]
    top = ok[-1]
    print("he_%s: logDelta accepted up to %d" % (fn, top))
    assert ok == list(range(1, top + 1)) and EDGE_SPARE + depth < top < 63
    assert am.const_int(2, top) <= INT64_MAX < am.const_int(2, top + 1)               # he_inv's constant 2 decides
    logq = logq_for(top + 1)
    assert logq // top == depth == logq // (top + 1)
    env = _env(engine_ctx, oracle_ctx, "edge", LOGN, logq, top, 2, 61)
    o0, _ = _assert_cell(env, fn, iter, t)
    assert bool((o0 != 0).any())
    g, W = env.g, env.W
    assert g.he_cmp_workspace_bytes(fn == "cmppt", W, logq, logq, top + 1, iter, t, env.batch) == 0
    assert "constant" in g.lib.gpq_last_error().decode()
    o0, o1 = bs.Guarded(8 * env.dev["A"][0].numel()), bs.Guarded(8 * env.dev["A"][1].numel())
    ws, _ = env.cmp_workspace(fn, iter, t)
    rc = g.he_cmp_call(o0.t, o1.t, env.dev["A"][0], env.dev["A"][1], env.other(fn), env.rlk[0], env.rlk[1], W, logq, logq, top + 1, iter, t, ws)
    torch.cuda.synchronize()
    assert rc == GPQ_ERR_INVALID and "constant" in g.lib.gpq_last_error().decode(), (rc, g.lib.gpq_last_error().decode())
    assert o0.untouched() and o1.untouched() and o0.guards_intact() and o1.guards_intact()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FNS)
def test_refusals_leave_the_outputs_alone(engine_ctx, oracle_ctx, fn):
    torch = _torch()
    env = _small(engine_ctx, oracle_ctx)
    g, W, n = env.g, env.W, env.g.n
    c0, c1 = env.dev["A"]
    words = c0.numel()
    arena = torch.full((2 * words + 3 * 512,), POISON, dtype=torch.int64, device="cuda")         # band | out0 | band | out1 | band
    o0, o1 = arena[512:512 + words], arena[1024 + words:1024 + 2 * words]
    ws = torch.empty(1 << 17, dtype=torch.int64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(None)

    def refused(logql=LOGQ, logdelta=LOGDELTA, iter=1, t=0, W=W, o0=o0, o1=o1, rlk0=env.rlk[0], m=env.pt["m1"], sizing=True):
        if sizing:
            assert g.he_cmp_workspace_bytes(fn == "cmppt", W, LOGQ, logql, logdelta, iter, t, BATCH) == 0, (logql, logdelta, iter, t)
        head = [g.h, p(o0), p(o1), p(c0), p(c1)]
        tail = [p(rlk0), p(env.rlk[1]), W, LOGQ, logql, logdelta, iter, t, BATCH, p(ws), g._stream()]
        if fn == "cmp":
            rc = g.lib.gpq_he_cmp(*head, p(env.dev["B"][0]), p(env.dev["B"][1]), *tail)
        else:
            rc = g.lib.gpq_he_cmppt(*head, p(m), *tail)
        torch.cuda.synchronize()
        assert rc == GPQ_ERR_INVALID, (logql, logdelta, iter, t, rc)
        assert bool((arena == POISON).all()), (logql, logdelta, iter, t)
        return g.lib.gpq_last_error().decode()

    for iter, t in ((0, 0), (1, 0), (1, 1), (0, 2)):
        d = cm.depth(iter, t)
        assert "level" in refused(d * LOGDELTA, iter=iter, t=t)                     # depth one beyond the last level: it would be q = 1
        assert g.he_cmp_workspace_bytes(fn == "cmppt", W, LOGQ, d * LOGDELTA + 1, LOGDELTA, iter, t, BATCH) > 0      # one bit more and it runs
    assert "level" in refused(iter=0, t=3)                                           # depth 12 from a chain of 10 levels
    assert "level" in refused(iter=0xFFFFFFFF, t=0xFFFFFFFF) and "level" in refused(iter=65533, t=65535)
    for bad in (0, 64, 200):
        assert "logDelta" in refused(logdelta=bad)
    assert "constant" in refused(logdelta=62, iter=0, t=0)                           # he_const_pt(two) at Delta = 2^62 is no int64_t
    refused(W=W - 1, sizing=False)                                                   # W too small for logql
    refused(rlk0=None, sizing=False)                                                 # a NULL key
    refused(o1=o0[n:], sizing=False)                                                 # overlapping outputs
    refused(o0=c1, sizing=False)                                                     # c0's output on the first input's c1
    if fn == "cmp":
        refused(o0=env.dev["B"][0], o1=env.dev["B"][1], sizing=False)                # in place on the SECOND input
    else:
        refused(m=o1[(BATCH - 1) * W * n:], sizing=False)                            # the plaintext inside an output
    few = engine_ctx(LOGN, 5)                                                        # he_mul at q = 2^200 needs 7 and 11 limbs
    assert few.he_cmp_workspace_bytes(fn == "cmppt", W, LOGQ, LOGQ, LOGDELTA, 1, 0, BATCH) == 0 and "primes" in few.lib.gpq_last_error().decode()


# ---------------------------------------------------------------------------
# streams: the protocol of tests/test_he_algo_gpu.py
# ---------------------------------------------------------------------------
STREAM_CASES = [("cmp", 1, 1), ("cmppt", 0, 1)]
_SLEEP = {}


def _calibration(env):
    """cycles of a sleep four times the longest host-side duration of a warm call (at least 20 ms), and a non-blocking side stream on which
    null-stream work overtakes such a sleep"""
    torch = _torch()
    if not _SLEEP:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        torch.cuda.synchronize()
        start.record()
        torch.cuda._sleep(20000000)
        stop.record()
        torch.cuda.synchronize()
        per_ms = 20000000 / start.elapsed_time(stop)
        longest = 0.0
        for fn, iter, t in STREAM_CASES:
            _run(env, fn, iter, t)                                                   # warm
            c0, c1 = (x.clone() for x in env.dev["A"])
            o0, o1 = torch.empty_like(c0), torch.empty_like(c1)
            ws, _ = env.cmp_workspace(fn, iter, t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.cmp_call(fn, iter, t, c0, c1, env.other(fn), o0, o1, ws)
            longest = max(longest, (time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
        sleep_ms = max(4 * longest, 20.0)
        _SLEEP.update(per_ms=per_ms, longest=longest, sleep_ms=sleep_ms, cycles=int(sleep_ms * per_ms))
        tried = []
        for _ in range(40):
            side = torch.cuda.Stream()
            seen = _overtaken(side, _SLEEP["cycles"] // 8)
            torch.cuda.synchronize()
            tried.append(int(seen))
            if tried[-1] == 0:
                _SLEEP["side"] = side
                break
        assert "side" in _SLEEP, "no side stream on which the null stream's work overtakes a sleep: %s" % tried
        print("longest host-side comparison call %.2f ms; sleep %.1f ms" % (longest, sleep_ms))
    return _SLEEP


def _late(env, fn):
    """buffers holding pair AB's inputs, and a producer that overwrites them with pair CD's"""
    a = [x.clone() for x in env.dev["A"]]
    other = tuple(x.clone() for x in env.dev["B"]) if fn == "cmp" else env.pt["m1"].clone()

    def producer():
        a[0].copy_(env.dev["C"][0])
        a[1].copy_(env.dev["C"][1])
        if fn == "cmp":
            other[0].copy_(env.dev["D"][0])
            other[1].copy_(env.dev["D"][1])
        else:
            other.copy_(env.pt["m2"])

    return a, other, producer


@pytest.mark.parametrize("fn,iter,t", STREAM_CASES)
def test_behind_a_sleeping_producer_on_a_side_stream(engine_ctx, oracle_ctx, fn, iter, t):
    torch = _torch()
    env = _small(engine_ctx, oracle_ctx)
    cal = _calibration(env)
    env.g.set_overlap(-1)
    want = {pair: env.separate(fn, iter, t, pair) for pair in PAIRS}
    _run(env, fn, iter, t)                                                           # warm
    (c0, c1), other, producer = _late(env, fn)
    o0, o1 = torch.full_like(c0, POISON), torch.full_like(c1, POISON)
    ws, words = env.cmp_workspace(fn, iter, t)
    side = cal["side"]
    seen = _overtaken(side, cal["cycles"], producer)
    with torch.cuda.stream(side):
        rc = env.cmp_call(fn, iter, t, c0, c1, other, o0, o1, ws)
        busy = not side.query()
        r0, r1 = o0.clone(), o1.clone()
    torch.cuda.synchronize()
    assert rc == 0
    assert int(seen) == 0, "the null stream was held back behind the side stream's sleep: this run would show nothing"
    is_ab = torch.equal(r0, want["AB"][0]) and torch.equal(r1, want["AB"][1])
    assert torch.equal(r0, want["CD"][0]) and torch.equal(r1, want["CD"][1]), "not f(C, D)%s" % (" but f(A, B): the call did not wait for the producer" if is_ab else "")
    assert torch.equal(c0, env.dev["C"][0]) and torch.equal(c1, env.dev["C"][1])
    assert busy, "the call returned only after the producer's %.1f ms sleep: a host synchronisation" % cal["sleep_ms"]
    assert bool((ws[words:] == 0x6B6B6B6B).all())


@pytest.mark.parametrize("fn,iter,t", STREAM_CASES)
def test_capture_and_replay_on_other_inputs(engine_ctx, oracle_ctx, fn, iter, t):
    torch = _torch()
    env = _small(engine_ctx, oracle_ctx)
    g = env.g
    want = {pair: env.separate(fn, iter, t, pair) for pair in PAIRS}
    g.set_overlap(0)
    try:
        _run(env, fn, iter, t)                                                       # warm
        (c0, c1), other, producer = _late(env, fn)
        o0, o1 = torch.full_like(c0, POISON), torch.full_like(c1, POISON)
        ws, words = env.cmp_workspace(fn, iter, t)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = env.cmp_call(fn, iter, t, c0, c1, other, o0, o1, ws)
        assert rc == 0, g.lib.gpq_last_error().decode()
        producer()                                                                   # C, D and m2 arrive
        o0.fill_(POISON)
        o1.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o0, want["CD"][0]) and torch.equal(o1, want["CD"][1]), "replay on the other inputs"
        assert bool((ws[words:] == 0x6B6B6B6B).all())
        del graph
    finally:
        torch.cuda.synchronize()
        g.set_overlap(-1)


# ---------------------------------------------------------------------------
# launch classes
# ---------------------------------------------------------------------------
class CmpProducts(Products):
    """... in which two squarings in a row -- a round's an^2 and bn^2, src/he-algo.c:489-492; he_inv's own squaring is always followed by another
    product -- count as the library issues them: ONE gpq_he_mul_rs over both operands' slabs, 2 batch ciphertexts"""
    addpt_dense = CmpDeviceOps.addpt_dense

    def __init__(self, env):
        Products.__init__(self, env)
        self.pairs, self.first = 0, None

    def rs(self, ct):
        torch = _torch()
        what, x, y, l = self.pending[id(ct)]
        square = what == "mul" and x is y
        before = dict(self.counts)
        Products.rs(self, ct)
        delta = {name: v - before.get(name, 0) for name, v in self.counts.items() if v - before.get(name, 0)}
        if square and self.first is not None:
            first_x, first_out, first_delta = self.first
            for d in (delta, first_delta):                                           # not the two products of batch ciphertexts ...
                for name, v in d.items():
                    self.counts[name] -= v
            both = tuple(torch.cat([p, q]) for p, q in zip(first_x, x))              # ... but one of 2 batch
            out = (torch.empty_like(both[0]), torch.empty_like(both[0]))
            dimP, dimA, dimB, _ = self.g.he_dims(self.logqL, self.logql(l))
            self._counted(lambda: self.g.he_mul_rs(out[0], out[1], both[0], both[1], both[0], both[1], self.e.rlk[0], self.e.rlk[1], self.W, self.logql(l),
                                                   dimA, dimB, dimP, self.s))
            assert all(torch.equal(o, torch.cat([p, q])) for o, p, q in zip(out, first_out, ct.c)), "the product of 2 batch ciphertexts is not the two products"
            self.pairs += 1
            self.first = None                                                        # (pairs do not chain)
        else:
            self.first = (x, ct.c, delta) if square else None


@pytest.mark.parametrize("fn,iter,t", STREAM_CASES)
def test_launch_classes(engine_ctx, oracle_ctx, fn, iter, t):
    """The call launches what its products launch when called separately with the same arguments -- the two squarings of a round being ONE
    gpq_he_mul_rs over 2 batch ciphertexts, one sequence of launches where two separate products show two -- and he_lin_const (with or without the plaintext term: one class): nothing else is recorded, and he_lin_const at most once per sum that
    tests/cmp_model.py's LazyOps materialises, plus one for the result's copy."""
    torch = _torch()
    env = _small(engine_ctx, oracle_ctx)
    g = env.g
    want = env.separate(fn, iter, t)
    _run(env, fn, iter, t)                                                           # warm
    g.profile(True)
    try:
        g.profile_collect()
        o0, o1, _, _, _ = _run(env, fn, iter, t)
        prof = {name: int(v[1]) for name, v in g.profile_collect().items()}
        ops = CmpProducts(env)
        out = env._run(ops, fn, iter, t, tuple(x.clone() for x in env.dev["A"]), tuple(x.clone() for x in env.dev["B"]), env.pt["m1"])
        torch.cuda.synchronize()
    finally:
        g.profile(False)
    assert not ops.pending
    assert torch.equal(o0, want[0]) and torch.equal(out.c[0], want[0]) and torch.equal(out.c[1], want[1])
    print("he_%s-%d-%d: the call %s; its products alone %s" % (fn, iter, t, prof, ops.counts))
    lin = prof.pop("he_lin_const", 0)
    assert "big_addsub" not in prof
    assert "he_lin_const" not in ops.counts and ops.pairs == t
    assert prof == {name: v for name, v in ops.counts.items() if v}
    lazy = cm.LazyOps(env.o, env.logn, env.logq, env.logdelta, env.rlk_host)
    lazy.value(env._run(lazy, fn, iter, t, tuple(env.cts["A"][0]), tuple(env.cts["B"][0]), env.pt_host["m1"]))
    assert 1 <= lin <= lazy.sums + 1, (lin, lazy.sums)
