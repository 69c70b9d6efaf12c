"""gpq_he_inv / gpq_he_sqrt / gpq_he_sigmoid / gpq_he_log / gpq_he_exp (include/gpqhe_hip_algo.h): the reference's evaluators as single calls.

Every evaluator's words are compared, without a tolerance,
  * with the SAME sequence (tests/algo_model.py, the reference's calls one by one) issued as separate public calls that existed before:
    gpq_he_mul + gpq_he_rs, gpq_he_mulpt with the constant as a dense plaintext + gpq_he_rs, gpq_big_addsub + gpq_he_rs(.., 0, .) for every
    he_add / he_addpt / he_subpt / he_neg, gpq_he_rs(.., 0, .) for he_moddown, device copies for he_copy_ct (DeviceOps, tests/algo_device.py);
  * with that sequence on the restated reference (oracle/bigint_ref.py), which tests/test_algo_model.py pins to the executed reference.
Shapes: logn 7, q_L = 2^200, Delta = 2^30, batch 2, iter 1 and 2 (he_exp with iter 2 ends at q = 2^20); one run at logn 13, batch 3, in launch
groups of 2.  Also: inputs untouched, a workspace of exactly the declared size with a guard behind it, every refusal with 0x5A-filled outputs
left alone, and each call behind a sleeping producer on a non-blocking side stream and inside a captured graph replayed on other inputs
(the protocol of tests/test_stream_contract_gpu.py)."""
import time

import pytest

from gpqhe_amd import big_to_ints, to_host
from tests import algo_model as am
from tests.algo_device import Env

pytestmark = pytest.mark.gpu

LOGN, LOGQ, LOGDELTA, BATCH = 7, 200, 30, 2
CASES = [("inv", 1), ("inv", 2), ("sqrt", 1), ("sqrt", 2), ("sigmoid", 0), ("log", 0), ("exp", 1), ("exp", 2)]
IDS = ["%s-%d" % c for c in CASES]
GPQ_ERR_INVALID = -1
POISON = 0x5A5A5A5A5A5A5A5A


def _torch():
    import torch
    return torch


_ENVS = {}


@pytest.fixture
def env(engine_ctx, oracle_ctx):
    if "small" not in _ENVS:
        _ENVS["small"] = Env(engine_ctx, oracle_ctx, LOGN, LOGQ, LOGDELTA, BATCH, 5)
    return _ENVS["small"]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    _torch().cuda.synchronize()
    _ENVS.clear()


def _run(env, kind, iter, which):
    """the evaluator on fresh copies of set `which` -> (out0, out1, the inputs it was given, the workspace and its declared words)"""
    torch = _torch()
    c0, c1 = (t.clone() for t in env.dev[which])
    o0, o1 = torch.full_like(c0, POISON), torch.full_like(c1, POISON)
    ws, words = env.workspace(kind, iter)
    rc = env.call(kind, iter, c0, c1, o0, o1, ws)
    assert rc == 0, env.g.lib.gpq_last_error().decode()
    torch.cuda.synchronize()
    return o0, o1, (c0, c1), ws, words


@pytest.mark.parametrize("kind,iter", CASES, ids=IDS)
def test_one_call_equals_the_separate_calls_and_the_restated_reference(env, kind, iter):
    torch = _torch()
    outs = {}
    for which in "AB":
        o0, o1, ins, ws, words = _run(env, kind, iter, which)
        want = env.separate(kind, iter, which)
        assert torch.equal(o0, want[0]) and torch.equal(o1, want[1]), "set %s: not the words of the separate calls" % which
        assert torch.equal(ins[0], env.dev[which][0]) and torch.equal(ins[1], env.dev[which][1]), "the inputs changed"
        assert bool((ws[words:] == 0x6B6B6B6B).all()), "the call wrote behind its declared workspace"
        outs[which] = (o0, o1)
    assert not torch.equal(outs["A"][0], outs["B"][0])
    assert env.g.he_algo_depth(kind, iter) == am.depth(kind, iter)
    # ... and the restated reference, on set A
    ops = am.BigintOps(env.o, env.logn, env.logq, env.logdelta, env.rlk_host)
    n, W = env.g.n, env.W
    got = [big_to_ints(to_host(t), W, n) for t in outs["A"]]
    for k, ct in enumerate(env.cts["A"]):
        out = am.run(kind, ops, am.Ct((ct[0], ct[1]), ops.L), iter, env.m_host)
        c = ops.value(out)
        assert got[0][k] == list(c[0]) and got[1][k] == list(c[1]), "ciphertext %d differs from the restated reference" % k


def test_in_place_and_no_iterations(env):
    torch = _torch()
    for kind, iter in (("inv", 1), ("sigmoid", 0), ("sqrt", 0), ("inv", 0)):       # sqrt with 0 iterations is he_copy_ct; inv with 0 is 2 - ct one level down
        c0, c1 = (t.clone() for t in env.dev["A"])
        ws, words = env.workspace(kind, iter)
        assert env.call(kind, iter, c0, c1, c0, c1, ws) == 0, env.g.lib.gpq_last_error().decode()
        torch.cuda.synchronize()
        want = env.separate(kind, iter, "A")
        assert torch.equal(c0, want[0]) and torch.equal(c1, want[1]), (kind, iter)
        assert bool((ws[words:] == 0x6B6B6B6B).all())


def test_refusals_leave_the_outputs_alone(env, engine_ctx):
    torch = _torch()
    g, W = env.g, env.W
    c0, c1 = env.dev["A"]
    o0, o1 = torch.full_like(c0, POISON), torch.full_like(c1, POISON)
    ws = torch.empty(1 << 16, dtype=torch.int64, device="cuda")

    def refused(ctx, kind, logql, logdelta, iter, W=W, logqL=LOGQ):
        assert ctx.he_algo_workspace_bytes(kind, W, logqL, logql, logdelta, iter, BATCH) == 0, (kind, logql, logdelta, iter)
        rc = ctx.he_algo_call(kind, o0, o1, c0, c1, env.rlk[0], env.rlk[1], W, logqL, logql, logdelta, iter, ws, env.m, env.dimpt)
        torch.cuda.synchronize()
        assert rc == GPQ_ERR_INVALID, (kind, logql, logdelta, iter, rc)
        assert bool((o0 == POISON).all()) and bool((o1 == POISON).all()), (kind, logql, logdelta, iter)
        return ctx.lib.gpq_last_error().decode()

    for kind in am.KINDS:
        it = 1 if kind in ("inv", "sqrt", "exp") else 0
        d = am.depth(kind, it)
        assert "level" in refused(g, kind, d * LOGDELTA, LOGDELTA, it)              # the last level would be q = 1
        assert "level" in refused(g, kind, d * LOGDELTA - 7, LOGDELTA, it)
        assert g.he_algo_workspace_bytes(kind, W, LOGQ, d * LOGDELTA + 1, LOGDELTA, it, BATCH) > 0      # one bit more and it runs
        for bad in (0, 64, 200):
            assert "logDelta" in refused(g, kind, LOGQ, bad, it)
    assert "level" in refused(g, "inv", LOGQ, LOGDELTA, 6)                           # depth 7 from a chain of 6 levels
    assert "level" in refused(g, "exp", LOGQ, LOGDELTA, 0xFFFFFFFF)
    # he_const_pt(two) at Delta = 2^62 is no int64_t.  (The other functions' constants pass gpq_he_mulpt_const_fits wherever their depth fits
    # these four words: |re| <= 12 against a basis that holds n q_l Delta.)
    assert "constant" in refused(g, "inv", LOGQ, 62, 1)
    few = engine_ctx(LOGN, 5)                                                        # he_mul at q = 2^200 needs 7 and 11 limbs
    assert "primes" in refused(few, "inv", LOGQ, LOGDELTA, 1)
    assert "primes" in refused(few, "sqrt", LOGQ, LOGDELTA, 1)
    rc = g.he_algo_call("inv", o0, o1, c0, c1, env.rlk[0], env.rlk[1], W - 1, LOGQ, LOGQ, LOGDELTA, 1, ws, env.m, env.dimpt)     # W too small for logql
    torch.cuda.synchronize()
    assert rc == GPQ_ERR_INVALID and bool((o0 == POISON).all()) and bool((o1 == POISON).all())
    rc = g.he_algo_call("exp", o0, o1, c0, c1, env.rlk[0], env.rlk[1], W, LOGQ, LOGQ, LOGDELTA, 1, ws, env.m, env.dimpt + 1)     # more limbs than the reference's he_mulpt
    torch.cuda.synchronize()
    assert rc == GPQ_ERR_INVALID and bool((o0 == POISON).all()) and bool((o1 == POISON).all())


# ---------------------------------------------------------------------------
# streams: the protocol of tests/test_stream_contract_gpu.py
# ---------------------------------------------------------------------------
_SLEEP = {}


def _overtaken(side, cycles, between=lambda: None):
    """a sleep and `flag = 1` on `side`, whatever between() queues, then a copy of the flag on the NULL stream: the copy reads 0 when null-stream
    work runs during the sleep (what a misplaced launch would do), 1 when this side stream holds the null stream back and shows nothing"""
    torch = _torch()
    flag, seen = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        flag.fill_(1)
        between()
    with torch.cuda.stream(torch.cuda.default_stream()):
        seen.copy_(flag)
    return seen


def _calibration(env):
    """cycles of a sleep four times the longest host-side duration of a warm evaluator call (at least 20 ms), and a non-blocking side stream on
    which null-stream work overtakes such a sleep"""
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
        for kind, iter in CASES:
            _run(env, kind, iter, "A")                                               # warm
            c0, c1 = (t.clone() for t in env.dev["A"])
            o0, o1 = torch.empty_like(c0), torch.empty_like(c1)
            ws, _ = env.workspace(kind, iter)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.call(kind, iter, c0, c1, o0, o1, ws)
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
        print("longest host-side evaluator call %.2f ms; sleep %.1f ms" % (longest, sleep_ms))
    return _SLEEP


@pytest.mark.parametrize("kind,iter", CASES, ids=IDS)
def test_behind_a_sleeping_producer_on_a_side_stream(env, kind, iter):
    torch = _torch()
    cal = _calibration(env)
    env.g.set_overlap(-1)
    want = {w: env.separate(kind, iter, w) for w in "AB"}
    _run(env, kind, iter, "A")                                                       # warm
    c0, c1 = (t.clone() for t in env.dev["A"])                                       # A in the inputs, poison in the outputs
    o0, o1 = torch.full_like(c0, POISON), torch.full_like(c1, POISON)
    ws, words = env.workspace(kind, iter)
    side = cal["side"]

    def producer():                                                                  # behind the sleep: B arrives
        c0.copy_(env.dev["B"][0])
        c1.copy_(env.dev["B"][1])

    seen = _overtaken(side, cal["cycles"], producer)
    with torch.cuda.stream(side):
        rc = env.call(kind, iter, c0, c1, o0, o1, ws)
        busy = not side.query()
        r0, r1 = o0.clone(), o1.clone()
    torch.cuda.synchronize()
    assert rc == 0
    assert int(seen) == 0, "the null stream was held back behind the side stream's sleep: this run would show nothing"
    is_a = torch.equal(r0, want["A"][0]) and torch.equal(r1, want["A"][1])
    assert torch.equal(r0, want["B"][0]) and torch.equal(r1, want["B"][1]), "not f(B)%s" % (" but f(A): the call did not wait for the producer" if is_a else "")
    assert torch.equal(c0, env.dev["B"][0]) and torch.equal(c1, env.dev["B"][1])
    assert busy, "the call returned only after the producer's %.1f ms sleep: a host synchronisation" % cal["sleep_ms"]
    assert bool((ws[words:] == 0x6B6B6B6B).all())


@pytest.mark.parametrize("kind,iter", CASES, ids=IDS)
def test_capture_and_replay_on_other_inputs(env, kind, iter):
    torch = _torch()
    g = env.g
    want = {w: env.separate(kind, iter, w) for w in "AB"}
    g.set_overlap(0)
    try:
        _run(env, kind, iter, "A")                                                   # warm
        c0, c1 = (t.clone() for t in env.dev["A"])
        o0, o1 = torch.full_like(c0, POISON), torch.full_like(c1, POISON)
        ws, words = env.workspace(kind, iter)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = env.call(kind, iter, c0, c1, o0, o1, ws)
        assert rc == 0, g.lib.gpq_last_error().decode()
        for which in "BA":
            c0.copy_(env.dev[which][0])
            c1.copy_(env.dev[which][1])
            o0.fill_(POISON)
            o1.fill_(POISON)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(o0, want[which][0]) and torch.equal(o1, want[which][1]), "replay on set %s" % which
        assert bool((ws[words:] == 0x6B6B6B6B).all())
        del graph
    finally:
        torch.cuda.synchronize()
        g.set_overlap(-1)


# ---------------------------------------------------------------------------
# a two-pass ring, several launch groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,iter", [("inv", 1), ("exp", 1)])
def test_two_pass_ring_in_launch_groups_of_two(engine_ctx, oracle_ctx, kind, iter):
    torch = _torch()
    if "big" not in _ENVS:
        _ENVS["big"] = Env(engine_ctx, oracle_ctx, 13, LOGQ, LOGDELTA, 3, 9)
    e = _ENVS["big"]
    e.g.set_chunk(2)
    try:
        o0, o1, ins, ws, words = _run(e, kind, iter, "A")
        want = e.separate(kind, iter, "A")
        assert torch.equal(o0, want[0]) and torch.equal(o1, want[1])
        assert torch.equal(ins[0], e.dev["A"][0]) and torch.equal(ins[1], e.dev["A"][1])
        assert bool((ws[words:] == 0x6B6B6B6B).all())
    finally:
        torch.cuda.synchronize()
        e.g.set_chunk(32)
