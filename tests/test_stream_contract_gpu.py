"""Where and when the work of every entry point with a `void *stream` runs (tests/stream_contract.py has the table and one closure per
entry point).  The words themselves are pinned to the reference by the numeric tests; nothing here has a reference or a tolerance.  Expected
words are the same closure run eagerly on the default stream between two torch.cuda.synchronize(), on the same context and on buffers of its
own, once for input set A and once for B; every comparison is torch.equal, and f(A) != f(B) is asserted for every entry.

(a) delayed producer, every CAPTURABLE and ORDERED entry: after a warm call on A, with A in the inputs and poison in the outputs, a
    NON-BLOCKING side stream gets, without any host synchronisation in between, a sleep, the copies of B into the same input buffers, the
    call, and clones of its outputs.  A piece of the call that went to the null stream ran during the sleep: it read A, or what it wrote was
    overwritten, and the clones are not f(B).  CAPTURABLE entries must also return while the sleep is still running (side.query() is
    False): an unannounced host synchronisation would have waited for the producer.  The two byte generators have no device input (their
    sets are two stream positions), so for them the outputs are poisoned once more on the side stream behind the sleep.
(b) capture and replay, every CAPTURABLE entry, one lane (gpq_set_overlap(0): the graph is one chain; the two-lane graph is
    tests/test_overlap_gpu.py's): warm on A, capture on static buffers, B into them and poison into the outputs, replay: f(B); A back,
    replay: f(A).  gpq_surf_bytes / gpq_rng_device_bytes repeat the captured position's bytes instead (include/gpqhe_hip.h).
    gpq_gemv_multi_create (REFUSES_IN_CAPTURE) returns GPQ_ERR_INVALID inside a capture, allocates nothing, and the capture still ends
    in a graph that replays.
    Streams share a few hardware queues (four by default), and work on the null stream is serialised behind a side stream that sits on
    the null stream's queue: behind such a stream a misplaced launch is invisible (with a fresh torch.cuda.Stream() per case, a library
    whose launch_decompose went to the null stream passed a quarter of its cases).  So ONE side stream is chosen once, by trying, on which
    null-stream work overtakes a sleep (_side_stream), and every run checks it again for itself: a copy queued on the null stream right
    before the call must have run during the sleep (_overtaken), else the case fails as blind.
(c) control: protocol (a) with a closure that hands gpq_rns_add NULL for the stream while the side stream is current must report a
    mismatch, the result being f(A).  If it does not, the sleep is too short or the side stream is not non-blocking, and (a) shows nothing.

The sleep is four times the longest host-side duration of any closure at these shapes, measured at the start of the module with
perf_counter around a warm call, and torch.cuda._sleep's cycles are calibrated to milliseconds with events (both printed by
test_calibration), with a floor of 20 ms so that a loaded host does not end a short sleep early.  Measured on an MI355X: 2394 cycles per
microsecond; the longest closure is gpq_he_gemv_multi at S2 with 1.00 ms on the host (4 ms), so the floor applies: 20.0 ms = 47 888 164
cycles.  The 218 cases of the module take 5.6 s together, most of it the 115 sleeps."""
import time

import pytest
import torch

from tests import bridge_settings as bs
from tests import stream_contract as sc

pytestmark = pytest.mark.gpu

SLEEP_FACTOR, SLEEP_FLOOR_MS = 4, 20.0

_contexts = bs.Cells()
_ENVS, _EXPECT, _SLEEP = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    torch.cuda.synchronize()
    _EXPECT.clear()
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    _contexts.close()


def _env(shape, engine_ctx):
    if shape not in _ENVS:
        if shape == sc.ECD_SHAPE[0]:
            _ENVS[shape] = sc.EcdEnv(_contexts.get(sc.ECD_SHAPE[1], 2, "default"))
        else:
            logn, logq = sc.SHAPES[shape]
            dims = engine_ctx(logn, 12).he_dims(logq, logq)
            _ENVS[shape] = sc.Env(shape, _contexts.get(logn, max(dims[3], sc.dimpt_of(logq, logn)), "default"), dims)
    return _ENVS[shape]


CASES = [(s, shape) for s in sc.SPECS for shape in s.shapes]
_id = lambda case: "%s-%s" % (case[0].key.replace(" ", "_"), case[1])
LAUNCHING = [pytest.param(c, id=_id(c)) for c in CASES]
CAPTURED = [pytest.param(c, id=_id(c)) for c in CASES if c[0].cls == sc.CAPTURABLE]


# ---------------------------------------------------------------------------
# buffers and results
# ---------------------------------------------------------------------------
def _inputs(spec, env, which):
    return sc.to_tensors(env, spec.ins(env, sc.np.random.default_rng(spec.seed(env.shape, which))))


def _poison(t):
    t.view(torch.uint8).fill_(sc.POISON_BYTE)


def _outputs(spec, env):
    outs = sc.Args(env)
    for name, (count, dtype) in spec.outs(env).items():
        raw = torch.empty(count * sc.np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
        outs[name] = raw.view({sc.U64: torch.int64, sc.I8: torch.int8, sc.U8: torch.uint8, sc.F64: torch.float64}[dtype])
        _poison(outs[name])
    return outs


def _workspace(spec, env):
    nbytes = spec.ws(env)
    ws =torch.empty(nbytes // 8 + 8, dtype=torch.int64, device="cuda")
    _poison(ws)
    return ws


def _tensors(ins):
    return {k: v for k, v in ins.items() if torch.is_tensor(v)}


def _load(dst, src):
    """the device words of set `src` into the buffers of `dst` (queued on the current stream); host values are taken over"""
    for k, v in src.items():
        if torch.is_tensor(v):
            dst[k].copy_(v)
        else:
            dst[k] = v


def _results(spec, ins, outs, info=None):
    """what a call left: clones of its outputs and of the inputs it overwrites (queued on the current stream), and what it returned"""
    res = {"out " + k: v.clone() for k, v in outs.items()}
    res.update({"inout " + k: ins[k].clone() for k in spec.inout})
    return res, info


def _same(a, b):
    return a[1] == b[1] and set(a[0]) == set(b[0]) and all(torch.equal(a[0][k], b[0][k]) for k in a[0])


def _differences(got, want):
    lines = [] if got[1] == want[1] else ["returned %s, expected %s" % (got[1], want[1])]
    for k in want[0]:
        bad = torch.nonzero(got[0][k].view(torch.uint8) != want[0][k].view(torch.uint8)).flatten()
        if bad.numel():
            lines.append("%s: %d of %d bytes differ, first at %s" % (k, bad.numel(), want[0][k].view(torch.uint8).numel(), bad[:4].tolist()))
    return "; ".join(lines)


def _expected(spec, env):
    """{which: (inputs, results)} of the closure run eagerly on the default stream, on buffers of its own; made once and never changed"""
    key = (spec.key, env.shape)
    if key not in _EXPECT:
        g, got = env.g, {}
        for which in "AB":
            ins, outs, ws = _inputs(spec, env, which), _outputs(spec, env), _workspace(spec, env)
            pristine = {k: v.clone() for k, v in _tensors(ins).items()}
            torch.cuda.synchronize()
            info = spec.call(g, ins, outs, ws)
            torch.cuda.synchronize()
            res = _results(spec, ins, outs, info)
            for k, v in pristine.items():
                assert k in spec.inout or torch.equal(ins[k], v), "%s wrote to its input `%s`" % (spec.key, k)
            pristine.update({k: v for k, v in ins.items() if not torch.is_tensor(v)})
            got[which] = (pristine, res)
        torch.cuda.synchronize()
        assert not _same(got["A"][1], got["B"][1]), "%s at %s: f(A) == f(B): nothing could be detected" % (spec.key, env.shape)
        for which in "AB":
            assert all(bool((t.view(torch.uint8) != sc.POISON_BYTE).any()) for t in got[which][1][0].values()), "%s: an output was never written" % spec.key
        _EXPECT[key] = got
    return _EXPECT[key]


# ---------------------------------------------------------------------------
# the sleep
# ---------------------------------------------------------------------------
def _calibration(engine_ctx):
    """(cycles per millisecond of torch.cuda._sleep, the longest host-side duration of a warm closure in ms and its name, the sleep in cycles)"""
    if not _SLEEP:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        torch.cuda.synchronize()
        probe = 20000000
        start.record()
        torch.cuda._sleep(probe)
        stop.record()
        torch.cuda.synchronize()
        per_ms = probe / start.elapsed_time(stop)
        longest, who = 0.0, ""
        for spec, shape in CASES:
            env = _env(shape, engine_ctx)
            ins, outs, ws = _inputs(spec, env, "A"), _outputs(spec, env), _workspace(spec, env)
            spec.call(env.g, ins, outs, ws)                          # warm: first-use tables, scratch, attributes
            for k, v in _inputs(spec, env, "A").items():
                if torch.is_tensor(v):
                    ins[k].copy_(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spec.call(env.g, ins, outs, ws)
            ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            if ms > longest:
                longest, who = ms, "%s at %s" % (spec.key, shape)
        sleep_ms = max(SLEEP_FACTOR * longest, SLEEP_FLOOR_MS)
        _SLEEP.update(per_ms=per_ms, longest=longest, who=who, sleep_ms=sleep_ms, cycles=int(sleep_ms * per_ms))
    return _SLEEP


def test_calibration(engine_ctx):
    cal = _calibration(engine_ctx)
    print("torch.cuda._sleep: %.1f cycles per microsecond; longest host-side closure: %s, %.2f ms; sleep %.1f ms = %d cycles"
          % (cal["per_ms"] / 1e3, cal["who"], cal["longest"], cal["sleep_ms"], cal["cycles"]))
    assert cal["per_ms"] > 0 and cal["longest"] > 0
    # the sleep really keeps a stream busy that long, and the host does not wait for it
    side = _side_stream(cal)
    print("side streams tried until the null stream's work overtook a sleep (0 = it did): %s" % cal["tried"])
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(cal["cycles"])
        queued_ms = (time.perf_counter() - t0) * 1e3
        busy = not side.query()
    torch.cuda.synchronize()
    waited_ms = (time.perf_counter() - t0) * 1e3
    assert busy and queued_ms < cal["sleep_ms"] / 2 and waited_ms > 0.8 * cal["sleep_ms"], (queued_ms, waited_ms, cal)


# ---------------------------------------------------------------------------
# (a) delayed producer on a non-blocking side stream
# ---------------------------------------------------------------------------
def _overtaken(side, cycles, between=lambda: None):
    """Queues a sleep and `flag = 1` on `side`, then whatever between() queues, then a copy of the flag on the NULL stream -- what a misplaced
    launch of a call would be.  -> a one-word tensor that reads 0 after the next synchronisation when the null stream's work ran during the
    sleep, 1 when it was held back behind it.  Streams share a few hardware queues (four by default): work on the null stream is
    serialised behind a side stream that happens to sit on the null stream's queue, and behind such a stream a misplaced launch is invisible."""
    flag, seen = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        flag.fill_(1)
        between()
    with torch.cuda.stream(torch.cuda.default_stream()):
        seen.copy_(flag)
    return seen


def _side_stream(cal):
    """a non-blocking stream that does not share its hardware queue with the null stream, found once by trying: the one every case uses"""
    if "side" not in _SLEEP:
        tried = []
        for _ in range(40):                                          # torch hands out the 32 streams of its pool in turn
            side = torch.cuda.Stream()
            seen = _overtaken(side, cal["cycles"] // 8)
            torch.cuda.synchronize()
            tried.append(int(seen))
            if tried[-1] == 0:
                _SLEEP["side"] = side
                break
        assert "side" in _SLEEP, "no side stream on which the null stream's work overtakes a sleep: %s" % tried
        _SLEEP["tried"] = tried
    return _SLEEP["side"]


def _delayed_producer(spec, env, cal, call=None, repoison=False):
    """protocol (a) -> (results the side stream left, the input buffers afterwards, was the side stream still busy when the call returned)"""
    call = call or spec.call
    g, want = env.g, _expected(spec, env)
    ins, outs, ws = _inputs(spec, env, "A"), _outputs(spec, env), _workspace(spec, env)
    spec.call(g, ins, outs, ws)                                      # 1. warm, eagerly, on these very buffers
    torch.cuda.synchronize()
    _load(ins, want["A"][0])                                         # 2. A in the inputs, poison in the outputs
    for t in outs.values():
        _poison(t)
    side = _side_stream(cal)

    def producer():
        if repoison:
            for t in outs.values():
                _poison(t)
        _load(ins, want["B"][0])

    seen = _overtaken(side, cal["cycles"], producer)                 # 3. (synchronises first) the sleep and the copies of B; nothing below waits on the host
    with torch.cuda.stream(side):
        info = call(g, ins, outs, ws)
        busy = not side.query()
        res = _results(spec, ins, outs, info)
    torch.cuda.synchronize()                                         # 4.
    # this very run could have shown a misplaced launch: work queued on the null stream right before the call ran during the sleep
    assert int(seen) == 0, "the null stream was held back behind the side stream's sleep: this run would show nothing"
    return res, ins, busy


@pytest.mark.parametrize("case", LAUNCHING)
def test_delayed_producer_on_a_side_stream(engine_ctx, case):
    spec, shape = case
    env, cal = _env(shape, engine_ctx), _calibration(engine_ctx)
    env.g.set_overlap(-1)                                            # the default: two lanes where the call takes them
    want = _expected(spec, env)
    res, ins, busy = _delayed_producer(spec, env, cal, repoison=spec.name in sc.REPEATS_ON_REPLAY)
    diff = _differences(res, want["B"][1])
    assert not diff, "%s at %s behind a delayed producer: not f(B)%s: %s" % (
        spec.key, shape, " but f(A): the call did not wait for the producer" if _same(res, want["A"][1]) else "", diff)
    for k, v in want["B"][0].items():                               # 5. the inputs are B (those the call overwrites are results above)
        if torch.is_tensor(v) and k not in spec.inout:
            assert torch.equal(ins[k], v), "%s at %s: input `%s` is not set B after the call" % (spec.key, shape, k)
    if spec.cls == sc.CAPTURABLE:
        assert busy, "%s at %s returned only after the producer's %.1f ms sleep: a host synchronisation in a CAPTURABLE call" % (spec.key, shape, cal["sleep_ms"])


# ---------------------------------------------------------------------------
# (b) capture and replay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CAPTURED)
def test_capture_and_replay(engine_ctx, case):
    spec, shape = case
    env = _env(shape, engine_ctx)
    g, want = env.g, _expected(spec, env)
    g.set_overlap(0)
    try:
        ins, outs, ws = _inputs(spec, env, "A"), _outputs(spec, env), _workspace(spec, env)
        spec.call(g, ins, outs, ws)                                  # 1. warm on A
        torch.cuda.synchronize()
        _load(ins, want["A"][0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                # 2. on static buffers
            spec.call(g, ins, outs, ws)
        repeats = spec.name in sc.REPEATS_ON_REPLAY
        for which in "BA":                                           # 3.-5.
            _load(ins, want[which][0])
            for t in outs.values():
                _poison(t)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            expect = want["A" if repeats else which][1]             # (the generators' position is a captured launch argument)
            diff = _differences(_results(spec, ins, outs, expect[1]), expect)
            assert not diff, "%s at %s, replay on set %s: %s" % (spec.key, shape, which, diff)
        del graph
    finally:
        torch.cuda.synchronize()
        g.set_overlap(-1)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_the_set_constructor_refuses_a_capturing_stream(engine_ctx, shape):
    assert sc.names_of(sc.REFUSES_IN_CAPTURE) == ["gpq_gemv_multi_create"]
    env = _env(shape, engine_ctx)
    g = env.g
    plans = (sc.C.c_void_p * 3)(*[p.h.value for p in [env.plan4] + env.others])
    x = torch.arange(4096, dtype=torch.int64, device="cuda")
    y = torch.zeros_like(x)
    handle = sc.C.c_void_p()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # (an allocation or a synchronous copy here would invalidate the capture)
        rc = g.lib.gpq_gemv_multi_create(g.h, sc.C.byref(handle), plans, 3, g._stream())
        message = g.lib.gpq_last_error().decode()
        y.copy_(x)
    assert rc == -1 and "capture" in message and not handle.value, (rc, message, handle.value)      # GPQ_ERR_INVALID, and no set was made
    assert not bool(y.any())                                         # nothing ran, nothing was written
    graph.replay()                                                   # the capture ended in a usable graph
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    with g.gemv_multi([env.plan4] + env.others) as made:             # ... and outside a capture the same arguments make a set
        assert made.count == 3


# ---------------------------------------------------------------------------
# (c) the protocol can fail
# ---------------------------------------------------------------------------
def test_control_a_call_on_the_null_stream_is_detected(engine_ctx):
    """gpq_rns_add only: pointwise, no context scratch, and both input sets are valid memory, so the planted fault is wrong words, never a
    bad address"""
    spec = next(s for s in sc.SPECS if s.name == "gpq_rns_add")
    env, cal = _env("S1", engine_ctx), _calibration(engine_ctx)
    want = _expected(spec, env)

    def on_the_null_stream(g, i, o, ws):
        e = i.env
        assert g._stream().value                                     # the side stream is current, and is not the null stream
        assert g.lib.gpq_rns_add(g.h, o["r"].data_ptr(), i["a"].data_ptr(), i["b"].data_ptr(), e.dim, e.batch, None) == 0

    res, ins, busy = _delayed_producer(spec, env, cal, call=on_the_null_stream)
    assert busy
    assert _differences(res, want["B"][1]), "a call on the null stream went unnoticed: the sleep is too short or the side stream is blocking"
    assert _same(res, want["A"][1]), "the planted call should have read set A during the sleep: " + _differences(res, want["A"][1])
    for k, v in want["B"][0].items():
        assert torch.equal(ins[k], v)
